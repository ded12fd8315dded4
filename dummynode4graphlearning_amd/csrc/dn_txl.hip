// The TransformerXL count model's attention (DESIGN.md "SI count models: TXL"): relative-position multi-head attention over a
// sliding memory as a block-banded attention over the whole padded sequence, fp32, gfx950.
//
// Rows layout: q, k, v, k_mem, v_mem [B, Lp, n, D] (Lp a multiple of seg), rk [P, n, D] indexed by RELATIVE POSITION, r_w_bias and
// r_r_bias [n, D].  The queries of segment s (rows s seg .. (s + 1) seg - 1, qlen = seg) attend the window of klen = seg + mlen keys
// from row k0 = s seg - mlen, mlen = min(mem, s seg); window row j < mlen is a MEMORY row (read from k_mem / v_mem), the others are
// the segment's own rows (read from k / v).  With AC[i, j] = (q_i + r_w_bias) . K_j and BD[i, j] = (q_i + r_r_bias) . rk[klen - 1 - j]:
//
//   f = i klen + j + qlen,  row = f / (klen + 1),  col = f % (klen + 1)            (the reference's pad-and-view rel_shift, flat)
//   score[i, j] = scale (AC[i, j] + (col == 0 ? 0 : BD[row, col - 1]))            row is i or i + 1 and never reaches qlen
//   out[i] = softmax_j(score[i, :]) V                                             over the WHOLE window: no causal mask
//
// One workgroup owns one (sequence, segment, head); wave w owns query rows 16 w .. 16 w + 15.  The products run on
// mfma_f32_16x16x4f32 (exact f32) with the operands read straight from memory (a window is shared by at most four waves); the BD
// tile of the whole segment crosses the waves through LDS, because the shifted read of row i needs BD's row i + 1.  The forward
// launch writes out, and per (row, head) the row max and the log of the sum: nothing of size qlen x klen leaves the chip.
//
// Backward, ONE workgroup per (sequence, segment, head) again: the probabilities are recomputed from the saved statistics,
// dS = scale P (dP - delta); dS and P of the whole segment go to LDS and the waves share out the key tiles of dK = dS^T (q + r_w_bias)
// and dV = P^T dO; the shift is undone by scattering dS into the BD tile's coordinates (a bijection onto every entry but
// BD[0, 0 .. qlen - 2], which get zero), which gives the BD part of dq and d rk.  The gradients at the window's memory rows and at
// rk are written per workgroup and summed by two small launches in a fixed order: no atomics, bit-identical from run to run.
#include "dn_common.h"

namespace {

constexpr int kMaxSeg = 64, kMaxWin = 128, kLd = kMaxWin + 4, kMaxTiles = kMaxWin / 16;

#define DN_MFMA4(acc, a, b)                                                     \
    do {                                                                        \
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32((a).x, (b).x, acc, 0, 0, 0); \
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32((a).y, (b).y, acc, 0, 0, 0); \
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32((a).z, (b).z, acc, 0, 0, 0); \
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32((a).w, (b).w, acc, 0, 0, 0); \
    } while (0)

struct Geo {
    int32_t Lp, n, seg, mem, P;
    float scale;
};

struct Win {
    int mlen, klen, k0, nt;
};

__device__ __forceinline__ Win window(const Geo& g, int s) {
    Win w;
    w.mlen = min(g.mem, s * g.seg);
    w.klen = g.seg + w.mlen;
    w.k0 = s * g.seg - w.mlen;
    w.nt = w.klen >> 4;
    return w;
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return float4{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}; }

// The wave's 16 x klen tiles of AC (kept in registers) and BD (written to bd[] at the segment's row); lane (i, g) supplies query row
// i0 + i and, per key tile, key 16 jt + i, four features 16 kc + 4 g .. + 3 at a time.
template <int D>
__device__ __forceinline__ void score_tiles(const Geo& ge, const Win& w, size_t seq, int h, int i0, int i, int g, const float* __restrict__ q,
                                            const float* __restrict__ k, const float* __restrict__ km, const float* __restrict__ rk,
                                            const float* __restrict__ rwb, const float* __restrict__ rrb, int qrow0, f32x4 (&ac)[kMaxTiles],
                                            float* bd) {
    constexpr int KC = D / 16;
    const size_t rs = (size_t)ge.n * D;
    const float* qp = q + (seq + qrow0 + i0 + i) * rs + (size_t)h * D + 4 * g;
    float4 qw[KC], qr[KC];
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
        const float4 qv = ld4(qp + 16 * kc);
        qw[kc] = add4(qv, ld4(rwb + (size_t)h * D + 16 * kc + 4 * g));
        qr[kc] = add4(qv, ld4(rrb + (size_t)h * D + 16 * kc + 4 * g));
    }
#pragma unroll
    for (int jt = 0; jt < kMaxTiles; ++jt) {
        ac[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (jt < w.nt) {
            const int j = 16 * jt + i;
            const float* kp = (j < w.mlen ? km : k) + (seq + w.k0 + j) * rs + (size_t)h * D + 4 * g;
            const float* rp = rk + ((size_t)(w.klen - 1 - j) * ge.n + h) * D + 4 * g;
            f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f}, b = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) {
                const float4 kv = ld4(kp + 16 * kc), rv = ld4(rp + 16 * kc);
                DN_MFMA4(a, qw[kc], kv);
                DN_MFMA4(b, qr[kc], rv);
            }
            ac[jt] = a;
#pragma unroll
            for (int r = 0; r < 4; ++r) bd[(i0 + 4 * g + r) * kLd + 16 * jt + i] = b[r];
        }
    }
}

// the shifted BD entry of (row ii of the segment, window key j)
__device__ __forceinline__ float shifted(const float* bd, int ii, int j, int qlen, int klen) {
    const int f = ii * klen + j + qlen, row = f / (klen + 1), col = f - row * (klen + 1);
    return col == 0 ? 0.f : bd[row * kLd + col - 1];
}

__device__ __forceinline__ float row_max16(float v) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ float row_sum16(float v) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

// grid (B, S, n), block 64 (seg / 16)
template <int D>
__global__ __launch_bounds__(256) void txl_fwd_kernel(Geo ge, const float* __restrict__ q, const float* __restrict__ k,
                                                     const float* __restrict__ v, const float* __restrict__ km,
                                                     const float* __restrict__ vm, const float* __restrict__ rk,
                                                     const float* __restrict__ rwb, const float* __restrict__ rrb, float* __restrict__ out,
                                                     float* __restrict__ stats) {
    constexpr int DT = D / 16;
    __shared__ float sb[kMaxSeg * kLd];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, g = lane >> 4;
    const int s = blockIdx.y, h = blockIdx.z, i0 = 16 * wave, qlen = ge.seg;
    const size_t seq = (size_t)blockIdx.x * ge.Lp, rs = (size_t)ge.n * D;
    const Win w = window(ge, s);

    f32x4 sc[kMaxTiles];
    score_tiles<D>(ge, w, seq, h, i0, i, g, q, k, km, rk, rwb, rrb, s * qlen, sc, sb);
    __syncthreads();
    float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY}, sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int jt = 0; jt < kMaxTiles; ++jt)
        if (jt < w.nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                sc[jt][r] = (sc[jt][r] + shifted(sb, i0 + 4 * g + r, 16 * jt + i, qlen, w.klen)) * ge.scale;
                mx[r] = fmaxf(mx[r], sc[jt][r]);
            }
#pragma unroll
    for (int r = 0; r < 4; ++r) mx[r] = row_max16(mx[r]);
#pragma unroll
    for (int jt = 0; jt < kMaxTiles; ++jt)
        if (jt < w.nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                sc[jt][r] = expf(sc[jt][r] - mx[r]);
                sum[r] += sc[jt][r];
            }
#pragma unroll
    for (int r = 0; r < 4; ++r) sum[r] = row_sum16(sum[r]);
    __syncthreads();                                              // every wave has read BD: the tile now takes the probabilities
#pragma unroll
    for (int jt = 0; jt < kMaxTiles; ++jt)
        if (jt < w.nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) sb[(i0 + 4 * g + r) * kLd + 16 * jt + i] = sc[jt][r] / sum[r];
    __syncthreads();

    f32x4 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int jt = 0; jt < w.nt; ++jt) {
        const float4 pv = ld4(sb + (i0 + i) * kLd + 16 * jt + 4 * g);
        const int j = 16 * jt + 4 * g;                             // keys j .. j + 3 (one side of the memory boundary: mlen % 16 == 0)
        const float* vp = (j < w.mlen ? vm : v) + (seq + w.k0 + j) * rs + (size_t)h * D + i;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            const float4 vv = float4{vp[16 * dt], vp[rs + 16 * dt], vp[2 * rs + 16 * dt], vp[3 * rs + 16 * dt]};
            DN_MFMA4(o[dt], pv, vv);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const size_t row = seq + (size_t)s * qlen + i0 + 4 * g + r;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) out[row * rs + (size_t)h * D + 16 * dt + i] = o[dt][r];
        if (i == 0) {
            stats[(row * ge.n + h) * 2] = mx[r];
            stats[(row * ge.n + h) * 2 + 1] = logf(sum[r]);
        }
    }
}

// grid (B, S, n), block 64 (seg / 16).  kpart / vpart [B, S, n, mem, D]: the gradients at the window's memory rows; rpart
// [B, S, n, P, D]: the gradient at rk's rows 0 .. klen - 1 (the rows past klen are not written and not read).
template <int D>
__global__ __launch_bounds__(256) void txl_bwd_kernel(Geo ge, const float* __restrict__ dout, const float* __restrict__ q,
                                                     const float* __restrict__ k, const float* __restrict__ v,
                                                     const float* __restrict__ km, const float* __restrict__ vm,
                                                     const float* __restrict__ rk, const float* __restrict__ rwb,
                                                     const float* __restrict__ rrb, const float* __restrict__ out,
                                                     const float* __restrict__ stats, float* __restrict__ dqw, float* __restrict__ dqr,
                                                     float* __restrict__ dk, float* __restrict__ dv, float* __restrict__ kpart,
                                                     float* __restrict__ vpart, float* __restrict__ rpart) {
    constexpr int DT = D / 16, KC = D / 16;
    __shared__ float s0[kMaxSeg * kLd];                            // BD, then P, then dBD (dS in BD's coordinates)
    __shared__ float s1[kMaxSeg * kLd];                            // dS
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, g = lane >> 4;
    const int s = blockIdx.y, h = blockIdx.z, i0 = 16 * wave, qlen = ge.seg, nw = qlen >> 4, S = ge.Lp / qlen;
    const size_t seq = (size_t)blockIdx.x * ge.Lp, rs = (size_t)ge.n * D, hd = (size_t)h * D;
    const size_t q0 = seq + (size_t)s * qlen;                      // the segment's first row
    const Win w = window(ge, s);
    const size_t wg = ((size_t)blockIdx.x * S + s) * ge.n + h;     // this workgroup's slot of the partial buffers

    // ---- the probabilities again, from the saved row statistics
    f32x4 p[kMaxTiles], ds[kMaxTiles];
    score_tiles<D>(ge, w, seq, h, i0, i, g, q, k, km, rk, rwb, rrb, s * qlen, p, s0);
    __syncthreads();
    float lse[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const size_t row = q0 + i0 + 4 * g + r;
        lse[r] = stats[(row * ge.n + h) * 2] + stats[(row * ge.n + h) * 2 + 1];
    }
#pragma unroll
    for (int jt = 0; jt < kMaxTiles; ++jt)
        if (jt < w.nt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                p[jt][r] = expf((p[jt][r] + shifted(s0, i0 + 4 * g + r, 16 * jt + i, qlen, w.klen)) * ge.scale - lse[r]);

    // ---- dP = dO V^T, delta = dO . out, dS = scale P (dP - delta)
    float4 dov[KC];
    float dpart = 0.f;
    {
        const float* dp = dout + (q0 + i0 + i) * rs + hd + 4 * g;
        const float* op = out + (q0 + i0 + i) * rs + hd + 4 * g;
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) {
            dov[kc] = ld4(dp + 16 * kc);
            const float4 ov = ld4(op + 16 * kc);
            dpart += dov[kc].x * ov.x + dov[kc].y * ov.y + dov[kc].z * ov.z + dov[kc].w * ov.w;
        }
    }
    dpart += __shfl_xor(dpart, 16);
    dpart += __shfl_xor(dpart, 32);                                // delta of row i0 + i, in every lane with this i
    float delta[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) delta[r] = __shfl(dpart, 4 * g + r);
#pragma unroll
    for (int jt = 0; jt < kMaxTiles; ++jt) {
        ds[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (jt < w.nt) {
            const int j = 16 * jt + i;
            const float* vp = (j < w.mlen ? vm : v) + (seq + w.k0 + j) * rs + hd + 4 * g;
            f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) {
                const float4 vv = ld4(vp + 16 * kc);
                DN_MFMA4(a, dov[kc], vv);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) ds[jt][r] = ge.scale * p[jt][r] * (a[r] - delta[r]);
        }
    }
    __syncthreads();                                              // every wave has read BD
#pragma unroll
    for (int jt = 0; jt < kMaxTiles; ++jt)
        if (jt < w.nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s0[(i0 + 4 * g + r) * kLd + 16 * jt + i] = p[jt][r];
                s1[(i0 + 4 * g + r) * kLd + 16 * jt + i] = ds[jt][r];
            }
    __syncthreads();

    // ---- dV = P^T dO and dK = dS^T (q + r_w_bias): the key tiles shared out over the waves, summed over the segment's rows
    for (int jt = wave; jt < w.nt; jt += nw) {
        f32x4 av[DT], ak[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) av[dt] = ak[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int qc = 0; qc < qlen / 4; ++qc) {
            const int row = 4 * qc + g;
            const float pa = s0[row * kLd + 16 * jt + i], da = s1[row * kLd + 16 * jt + i];
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const float dob = dout[(q0 + row) * rs + hd + 16 * dt + i];
                const float qb = q[(q0 + row) * rs + hd + 16 * dt + i] + rwb[hd + 16 * dt + i];
                av[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa, dob, av[dt], 0, 0, 0);
                ak[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(da, qb, ak[dt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = 16 * jt + 4 * g + r;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                if (j >= w.mlen) {
                    const size_t o = (seq + w.k0 + j) * rs + hd + 16 * dt + i;
                    dv[o] = av[dt][r];
                    dk[o] = ak[dt][r];
                } else {
                    const size_t o = (wg * ge.mem + j) * D + 16 * dt + i;
                    vpart[o] = av[dt][r];
                    kpart[o] = ak[dt][r];
                }
            }
        }
    }
    // ---- the AC part of dq: dS K, the wave's own rows
    {
        f32x4 a[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) a[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int jt = 0; jt < w.nt; ++jt) {
            const float4 dsv = ld4(s1 + (i0 + i) * kLd + 16 * jt + 4 * g);
            const int j = 16 * jt + 4 * g;
            const float* kp = (j < w.mlen ? km : k) + (seq + w.k0 + j) * rs + hd + i;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const float4 kv = float4{kp[16 * dt], kp[rs + 16 * dt], kp[2 * rs + 16 * dt], kp[3 * rs + 16 * dt]};
                DN_MFMA4(a[dt], dsv, kv);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) dqw[(q0 + i0 + 4 * g + r) * rs + hd + 16 * dt + i] = a[dt][r];
    }
    __syncthreads();                                              // P has been read: s0 takes dS in BD's coordinates

    // ---- undo the shift: dBD[row, col - 1] = dS[i, j]; BD[0, 0 .. qlen - 2] is read by nobody
    for (int c = tid; c < qlen - 1; c += 64 * nw) s0[c] = 0.f;
#pragma unroll
    for (int jt = 0; jt < kMaxTiles; ++jt)
        if (jt < w.nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = (i0 + 4 * g + r) * w.klen + 16 * jt + i + qlen, row = f / (w.klen + 1), col = f - row * (w.klen + 1);
                if (col > 0) s0[row * kLd + col - 1] = ds[jt][r];
            }
    __syncthreads();
    // the BD part of dq: dBD rk[klen - 1 - c], the wave's own rows
    {
        f32x4 a[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) a[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int ct = 0; ct < w.nt; ++ct) {
            const float4 dbv = ld4(s0 + (i0 + i) * kLd + 16 * ct + 4 * g);
            const int c = 16 * ct + 4 * g;
            const float* rp = rk + ((size_t)(w.klen - 1 - c) * ge.n + h) * D + i;      // rows c .. c + 3 walk DOWN the table
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const float4 rv = float4{rp[16 * dt], rp[16 * dt - (ptrdiff_t)rs], rp[16 * dt - 2 * (ptrdiff_t)rs],
                                         rp[16 * dt - 3 * (ptrdiff_t)rs]};
                DN_MFMA4(a[dt], dbv, rv);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) dqr[(q0 + i0 + 4 * g + r) * rs + hd + 16 * dt + i] = a[dt][r];
    }
    // d rk[klen - 1 - c] = sum over the segment's rows of dBD[row, c] (q_row + r_r_bias): the column tiles shared out over the waves
    for (int ct = wave; ct < w.nt; ct += nw) {
        f32x4 a[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) a[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int qc = 0; qc < qlen / 4; ++qc) {
            const int row = 4 * qc + g;
            const float da = s0[row * kLd + 16 * ct + i];
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const float qb = q[(q0 + row) * rs + hd + 16 * dt + i] + rrb[hd + 16 * dt + i];
                a[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(da, qb, a[dt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int pos = w.klen - 1 - (16 * ct + 4 * g + r);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) rpart[(wg * ge.P + pos) * D + 16 * dt + i] = a[dt][r];
        }
    }
}

// dk_mem / dv_mem [B, Lp, n, D]: row `pos` is a memory row of every later segment whose window starts at or before it; summed in
// segment order.  One thread per element.
__global__ void txl_fold_mem_kernel(int64_t total, Geo ge, int32_t D, const float* __restrict__ kpart, const float* __restrict__ vpart,
                                    float* __restrict__ dkm, float* __restrict__ dvm) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % D), h = (int)((idx / D) % ge.n), pos = (int)((idx / ((int64_t)D * ge.n)) % ge.Lp);
    const int64_t b = idx / ((int64_t)D * ge.n * ge.Lp);
    const int S = ge.Lp / ge.seg;
    float ak = 0.f, av = 0.f;
    for (int s = pos / ge.seg + 1; s < S; ++s) {
        const int mlen = min(ge.mem, s * ge.seg), k0 = s * ge.seg - mlen;
        if (pos < k0) break;
        const size_t o = ((((size_t)b * S + s) * ge.n + h) * ge.mem + (pos - k0)) * D + c;
        ak += kpart[o];
        av += vpart[o];
    }
    dkm[idx] = ak;
    dvm[idx] = av;
}

// d rk [P, n, D] = the sum of rpart over (sequence, segment) in a fixed order.  grid (P, n), block (D, 1024 / D).
__global__ __launch_bounds__(1024) void txl_reduce_rk_kernel(int64_t B, Geo ge, int32_t D, const float* __restrict__ rpart,
                                                            float* __restrict__ drk) {
    __shared__ float red[1024];
    const int pos = blockIdx.x, h = blockIdx.y, c = threadIdx.x, ty = threadIdx.y, ny = blockDim.y;
    const int S = ge.Lp / ge.seg;
    const int64_t T = B * S;
    float acc = 0.f;
    for (int64_t t = ty; t < T; t += ny) {
        const int s = (int)(t % S);
        if (pos < ge.seg + min(ge.mem, s * ge.seg)) acc += rpart[(((size_t)t * ge.n + h) * ge.P + pos) * D + c];
    }
    red[ty * D + c] = acc;
    __syncthreads();
    if (ty == 0) {
        float sum = 0.f;
        for (int y = 0; y < ny; ++y) sum += red[y * D + c];
        drk[((size_t)pos * ge.n + h) * D + c] = sum;
    }
}

int check_txl(const char* what, int64_t B, int32_t Lp, int32_t n, int32_t D, int32_t seg, int32_t mem, int32_t P) {
    DN_REQUIRE(B >= 1 && Lp >= 1 && n >= 1 && P >= 1, "%s: bad sizes (B = %lld, Lp = %d, heads = %d, P = %d)", what, (long long)B, Lp, n, P);
    DN_REQUIRE(D == 16 || D == 32 || D == 64, "%s: the head width must be 16, 32 or 64 (got %d)", what, D);
    DN_REQUIRE(seg >= 16 && seg <= kMaxSeg && seg % 16 == 0, "%s: the segment length must be 16, 32, 48 or 64 (got %d)", what, seg);
    DN_REQUIRE(mem >= 0 && mem % 16 == 0 && seg + mem <= kMaxWin,
               "%s: the memory length must be a multiple of 16 with seg + mem <= %d (seg = %d, mem = %d)", what, kMaxWin, seg, mem);
    DN_REQUIRE(Lp % seg == 0, "%s: Lp = %d is no multiple of the segment length %d", what, Lp, seg);
    DN_REQUIRE(P >= seg + mem, "%s: rk needs seg + mem = %d rows (got %d)", what, seg + mem, P);
    DN_REQUIRE(Lp / seg <= 65535 && n <= 65535, "%s: at most 65535 segments and heads (got %d, %d)", what, Lp / seg, n);
    DN_REQUIRE(B * (int64_t)Lp * n * D < 0x7fffffffLL && B * (int64_t)(Lp / seg) * n * P * D < 0x7fffffffLL,
               "%s: B Lp n D and B S n P D must stay below 2^31 (B = %lld, Lp = %d)", what, (long long)B, Lp);
    return DN_OK;
}

}  // namespace

extern "C" {

int dn_txl_attn_fwd_f32(int64_t B, int32_t Lp, int32_t n, int32_t D, int32_t seg, int32_t mem, int32_t P, float scale, const float* q,
                        const float* k, const float* v, const float* k_mem, const float* v_mem, const float* rk, const float* r_w_bias,
                        const float* r_r_bias, float* out, float* stats, dn_stream_t stream) {
    if (int rc = check_txl("dn_txl_attn_fwd", B, Lp, n, D, seg, mem, P)) return rc;
    DN_REQUIRE(q && k && v && rk && r_w_bias && r_r_bias && out && stats, "dn_txl_attn_fwd: NULL pointer");
    DN_REQUIRE(mem == 0 || (k_mem && v_mem), "dn_txl_attn_fwd: a memory needs k_mem and v_mem");
    const Geo ge{Lp, n, seg, mem, P, scale};
    const dim3 grid((unsigned)B, (unsigned)(Lp / seg), (unsigned)n), block(64 * (seg / 16));
    if (mem == 0) k_mem = k, v_mem = v;
#define DN_TXL_FWD(DD) \
    hipLaunchKernelGGL((txl_fwd_kernel<DD>), grid, block, 0, (hipStream_t)stream, ge, q, k, v, k_mem, v_mem, rk, r_w_bias, r_r_bias, out, stats)
    if (D == 16) DN_TXL_FWD(16);
    else if (D == 32) DN_TXL_FWD(32);
    else DN_TXL_FWD(64);
#undef DN_TXL_FWD
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_txl_attn_bwd_f32(int64_t B, int32_t Lp, int32_t n, int32_t D, int32_t seg, int32_t mem, int32_t P, float scale, const float* dout,
                        const float* q, const float* k, const float* v, const float* k_mem, const float* v_mem, const float* rk,
                        const float* r_w_bias, const float* r_r_bias, const float* out, const float* stats, float* dq_ac, float* dq_bd,
                        float* dk, float* dv, float* k_part, float* v_part, float* rk_part, dn_stream_t stream) {
    if (int rc = check_txl("dn_txl_attn_bwd", B, Lp, n, D, seg, mem, P)) return rc;
    DN_REQUIRE(dout && q && k && v && rk && r_w_bias && r_r_bias && out && stats && dq_ac && dq_bd && dk && dv && rk_part,
               "dn_txl_attn_bwd: NULL pointer");
    DN_REQUIRE(mem == 0 || (k_mem && v_mem && k_part && v_part), "dn_txl_attn_bwd: a memory needs k_mem, v_mem, k_part and v_part");
    const Geo ge{Lp, n, seg, mem, P, scale};
    const dim3 grid((unsigned)B, (unsigned)(Lp / seg), (unsigned)n), block(64 * (seg / 16));
    if (mem == 0) k_mem = k, v_mem = v;
#define DN_TXL_BWD(DD)                                                                                                                  \
    hipLaunchKernelGGL((txl_bwd_kernel<DD>), grid, block, 0, (hipStream_t)stream, ge, dout, q, k, v, k_mem, v_mem, rk, r_w_bias, r_r_bias, \
                       out, stats, dq_ac, dq_bd, dk, dv, k_part, v_part, rk_part)
    if (D == 16) DN_TXL_BWD(16);
    else if (D == 32) DN_TXL_BWD(32);
    else DN_TXL_BWD(64);
#undef DN_TXL_BWD
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_txl_fold_mem_f32(int64_t B, int32_t Lp, int32_t n, int32_t D, int32_t seg, int32_t mem, const float* k_part, const float* v_part,
                        float* dk_mem, float* dv_mem, dn_stream_t stream) {
    if (int rc = check_txl("dn_txl_fold_mem", B, Lp, n, D, seg, mem, seg + mem)) return rc;
    DN_REQUIRE(mem > 0, "dn_txl_fold_mem: no memory to fold (mem = 0)");
    DN_REQUIRE(k_part && v_part && dk_mem && dv_mem, "dn_txl_fold_mem: NULL pointer");
    const Geo ge{Lp, n, seg, mem, seg + mem, 0.f};
    const int64_t total = B * (int64_t)Lp * n * D;
    hipLaunchKernelGGL(txl_fold_mem_kernel, dim3((unsigned)dn_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, total, ge, D, k_part,
                       v_part, dk_mem, dv_mem);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_txl_reduce_rk_f32(int64_t B, int32_t Lp, int32_t n, int32_t D, int32_t seg, int32_t mem, int32_t P, const float* rk_part, float* drk,
                         dn_stream_t stream) {
    if (int rc = check_txl("dn_txl_reduce_rk", B, Lp, n, D, seg, mem, P)) return rc;
    DN_REQUIRE(rk_part && drk, "dn_txl_reduce_rk: NULL pointer");
    const Geo ge{Lp, n, seg, mem, P, 0.f};
    hipLaunchKernelGGL(txl_reduce_rk_kernel, dim3((unsigned)P, (unsigned)n), dim3((unsigned)D, (unsigned)(1024 / D)), 0, (hipStream_t)stream,
                       B, ge, D, rk_part, drk);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

}  // extern "C"
