// The CNN count model's layer on edge sequences in rows layout x [B, L, C] (DESIGN.md "SI count models: CNN"), fp32, gfx950:
//
//   x0 = x * gate_in          conv[b, s] = sum_j x0[b, s - p + j] @ W[:, :, j]^T + bias        s in [0, L1), L1 = L + 2p - k + 1
//   pooled[b, t] = max_j act(conv)[b, t - p + j]   (positions outside [0, L1) skipped)         t in [0, L2), L2 = L1 + 2p - k + 1
//   gate_out[b, t] = max of gate_in[b, r] over r in [t - 2p, t - 2p + 2k - 2] inside [0, L)    (the two max pools of the gate)
//   y = pooled * gate_out (+ x0 when residual and L2 == L)
//
// Sequences are right-aligned: lo[b] is the first position of sequence b that may carry a non-zero gate (host data, planned from
// the lengths).  An output tile left of the support of its sequence is never computed: its rows are zero (pooled there is act(bias),
// its gate is 0, and x0 is 0).  A live tile computes 64 conv rows on the exact-f32 matrix cores (mfma_f32_16x16x4f32: the products
// are an fmaf chain in k order, so results are bit-identical from run to run) from an LDS image of its 64 + k - 1 input rows, writes
// the conv values back over that image and pools them.  The same tile routine, with the weights flipped and transposed and padding
// k - 1 - p, is the input gradient.  The weight gradient sums x0^T dconv over the live conv rows of a fixed slice of the batch per
// workgroup (the partials), and a combine adds the partials in slice order: no atomics anywhere.
#include "dn_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kRows = 64;             // conv rows of a tile
constexpr int kMaxC = 128;
constexpr int kMaxK = 5;
constexpr int kLd = kMaxC + 4;        // LDS row stride bound (rows are C + 4 floats apart: 16-byte aligned, spread over the banks)
constexpr int kWgRows = 32;           // conv rows per step of the weight gradient
constexpr int kFilterCap = 4096;      // labels the filter's bit sets hold

struct ConvArgs {
    int32_t L_src, L_out;             // rows of the source / of the conv result, per sequence
    int32_t C, k, pad;                // pad: the conv's zero padding on the source
    const float* src;                 // [B, L_src, C]
    const float* src_gate;            // [B, L_src] or NULL: the source rows are multiplied by it
    const float* w;                   // [k][C (summed)][C (result)]
};

// conv rows s0 .. s0 + 63 of sequence b -> tile[row * ld + col] (without bias); every thread of the workgroup calls it
__device__ __forceinline__ void conv_tile(const ConvArgs& a, int64_t b, int s0, float* tile) {
    const int C = a.C, ld = C + 4, c4n = C >> 2, tid = threadIdx.x;
    const int r0 = s0 - a.pad, nsrc = kRows + a.k - 1;
    for (int idx = tid; idx < nsrc * c4n; idx += kBlock) {
        const int row = idx / c4n, c4 = idx - row * c4n, r = r0 + row;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r >= 0 && r < a.L_src) {
            v = *reinterpret_cast<const float4*>(a.src + ((size_t)b * a.L_src + r) * C + 4 * c4);
            if (a.src_gate != nullptr) {
                const float g = a.src_gate[(size_t)b * a.L_src + r];
                v.x *= g; v.y *= g; v.z *= g; v.w *= g;
            }
        }
        *reinterpret_cast<float4*>(tile + row * ld + 4 * c4) = v;
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63, i = lane & 15, g = lane >> 4;
    const int NT = C >> 4, nsplit = NT >= 4 ? 4 : (NT >= 2 ? 2 : 1), msplit = 4 / nsplit;
    const int nw = wave % nsplit, mw = wave / nsplit;
    f32x4 acc[4][2];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < a.k; ++j)
        for (int kc = 0; kc < NT; ++kc) {
            const int kk = kc * 16 + 4 * g;                      // this lane's four summed channels (MFMA k index g <-> channel kk + e)
            float bq[2][4];
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const int n = nw + ni * nsplit;
#pragma unroll
                for (int e = 0; e < 4; ++e) bq[ni][e] = n < NT ? a.w[((size_t)j * C + kk + e) * C + n * 16 + i] : 0.f;
            }
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
                if (mi >= nsplit) continue;
                const int m = mw + mi * msplit;
                const float4 av = *reinterpret_cast<const float4*>(tile + (m * 16 + i + j) * ld + kk);
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) {
                    if (nw + ni * nsplit >= NT) continue;
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bq[ni][0], acc[mi][ni], 0, 0, 0);
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bq[ni][1], acc[mi][ni], 0, 0, 0);
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bq[ni][2], acc[mi][ni], 0, 0, 0);
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bq[ni][3], acc[mi][ni], 0, 0, 0);
                }
            }
        }
    __syncthreads();                                              // every wave has read its source rows: the image is free
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
        if (mi >= nsplit) continue;
        const int m = mw + mi * msplit;
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const int n = nw + ni * nsplit;
            if (n >= NT) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) tile[(m * 16 + 4 * g + r) * ld + n * 16 + i] = acc[mi][ni][r];
        }
    }
    __syncthreads();
}

__device__ __forceinline__ int first_live_output(int lo, int k, int p) {     // first t whose receptive field reaches position lo
    const int t = lo - 2 * (k - 1) + 2 * p;
    return t > 0 ? t : 0;
}

// grid (tiles of 64 - (k - 1) outputs, B)
__global__ __launch_bounds__(kBlock) void eseq_fwd_kernel(int32_t L, int32_t C, int32_t k, int32_t p, int32_t act, float slope, int32_t residual,
                                                         const float* __restrict__ x, const float* __restrict__ gate_in,
                                                         const float* __restrict__ wt, const float* __restrict__ bias,
                                                         const int32_t* __restrict__ lo, float* __restrict__ y,
                                                         float* __restrict__ gate_out, uint8_t* __restrict__ arg) {
    __shared__ float tile[(kRows + kMaxK - 1) * kLd];
    __shared__ float gout[kRows];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.y;
    const int L1 = L + 2 * p - k + 1, L2 = L1 + 2 * p - k + 1, step = kRows - (k - 1);
    const int t0 = blockIdx.x * step, nt = min(step, L2 - t0);
    if (t0 + nt <= first_live_output(lo[b], k, p)) {              // left of the support: zero rows, zero gate
        for (int idx = tid; idx < nt * C; idx += kBlock) y[((size_t)b * L2 + t0) * C + idx] = 0.f;
        for (int idx = tid; idx < nt; idx += kBlock) gate_out[(size_t)b * L2 + t0 + idx] = 0.f;
        return;
    }
    if (tid < nt) {
        const int t = t0 + tid;
        float g = 0.f;
        for (int r = max(t - 2 * p, 0); r <= min(t - 2 * p + 2 * k - 2, L - 1); ++r) g = fmaxf(g, gate_in[(size_t)b * L + r]);
        gout[tid] = g;
        gate_out[(size_t)b * L2 + t] = g;
    }
    ConvArgs a{L, L1, C, k, p, x, gate_in, wt};
    const int s0 = t0 - p;
    conv_tile(a, b, s0, tile);                                    // (its barriers also publish gout)
    const int ld = C + 4;
    for (int idx = tid; idx < nt * C; idx += kBlock) {
        const int tl = idx / C, c = idx - tl * C, t = t0 + tl;
        const float bc = bias[c];
        float best = 0.f, vbest = 0.f;
        int slot = -1;
        for (int j = 0; j < k; ++j) {
            const int s = t - p + j;
            if (s < 0 || s >= L1) continue;
            const float v = tile[(tl + j) * ld + c] + bc;
            const float av = act == 0 ? v : dn_act(v, slope);
            if (slot < 0 || av > best) { best = av; vbest = v; slot = j; }
        }
        const float g = gout[tl];
        float out = g != 0.f ? best * g : 0.f;
        if (residual) out += x[((size_t)b * L + t) * C + c] * gate_in[(size_t)b * L + t];
        const size_t o = ((size_t)b * L2 + t) * C + c;
        y[o] = out;
        arg[o] = (uint8_t)(slot | (vbest > 0.f ? 0x80 : 0));
    }
}

// dconv[b, s, c] = sum over the outputs t = s + p - j that chose slot j of dy * gate_out * act'(conv); one thread per element
__global__ __launch_bounds__(kBlock) void eseq_dconv_kernel(int64_t total, int32_t L1, int32_t L2, int32_t C, int32_t k, int32_t p,
                                                           int32_t act, float slope, const float* __restrict__ dy,
                                                           const float* __restrict__ gate_out, const uint8_t* __restrict__ arg,
                                                           float* __restrict__ dconv) {
    const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    const int64_t bs = idx / C;
    const int s = (int)(bs % L1);
    const int64_t b = bs / L1;
    float sum = 0.f;
    for (int j = 0; j < k; ++j) {
        const int t = s + p - j;
        if (t < 0 || t >= L2) continue;
        const float g = gate_out[b * L2 + t];
        if (g == 0.f) continue;
        const size_t o = ((size_t)b * L2 + t) * C + c;
        const uint8_t a = arg[o];
        if ((a & 7) != j) continue;
        const float d = dy[o] * g;
        sum += (act == 0 || (a & 0x80)) ? d : dn_neg(d, slope);
    }
    dconv[idx] = sum;
}

// dx[b, r] = (sum_j dconv[b, r + p - j] @ W[:, :, j] (+ dy[b, r])) * gate_in[b, r]; grid (tiles of 64 positions, B)
__global__ __launch_bounds__(kBlock) void eseq_dgrad_kernel(int32_t L, int32_t C, int32_t k, int32_t p, int32_t residual,
                                                           const float* __restrict__ dconv, const float* __restrict__ dy,
                                                           const float* __restrict__ gate_in, const float* __restrict__ wd,
                                                           const int32_t* __restrict__ lo, float* __restrict__ dx) {
    __shared__ float tile[(kRows + kMaxK - 1) * kLd];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.y;
    const int L1 = L + 2 * p - k + 1;
    const int r0 = blockIdx.x * kRows, nt = min(kRows, L - r0);
    if (r0 + nt <= lo[b]) {
        for (int idx = tid; idx < nt * C; idx += kBlock) dx[((size_t)b * L + r0) * C + idx] = 0.f;
        return;
    }
    ConvArgs a{L1, L, C, k, k - 1 - p, dconv, nullptr, wd};
    conv_tile(a, b, r0, tile);
    const int ld = C + 4;
    for (int idx = tid; idx < nt * C; idx += kBlock) {
        const int tl = idx / C, c = idx - tl * C, r = r0 + tl;
        const float g = gate_in[(size_t)b * L + r];
        const size_t o = ((size_t)b * L + r) * C + c;
        float v = tile[tl * ld + c];
        if (residual) v += dy[o];
        dx[o] = g != 0.f ? v * g : 0.f;
    }
}

// grid (G, k): workgroup (g, j) sums x0[b, s - p + j]^T dconv[b, s] over the live conv rows of the 32-row tiles q in its slice of
// [0, B * nper) -> part[g][j][ci][co]; the j == 0 workgroups also sum dconv's columns -> part_b[g][co]
__global__ __launch_bounds__(kBlock) void eseq_wgrad_kernel(int64_t B, int32_t L, int32_t C, int32_t k, int32_t p,
                                                           const float* __restrict__ x, const float* __restrict__ gate_in,
                                                           const float* __restrict__ dconv, const int32_t* __restrict__ lo,
                                                           float* __restrict__ part, float* __restrict__ part_b) {
    __shared__ float xs[kWgRows * kMaxC];
    __shared__ float ds[kWgRows * kMaxC];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, g4 = lane >> 4;
    const int G = gridDim.x, gi = blockIdx.x, j = blockIdx.y;
    const int L1 = L + 2 * p - k + 1, nper = (L1 + kWgRows - 1) / kWgRows, NT = C >> 4, c4n = C >> 2;
    const int64_t Q = B * nper, q_beg = Q * gi / G, q_end = Q * (gi + 1) / G;
    f32x4 acc[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    float colsum = 0.f;
    for (int64_t q = q_beg; q < q_end; ++q) {
        const int64_t b = q / nper;
        const int s0 = (int)(q - b * nper) * kWgRows;
        const int s_lo = first_live_output(lo[b], k, p) - p;      // conv rows left of it feed dead outputs only
        if (s0 + kWgRows <= s_lo) continue;                       // (uniform over the workgroup)
        for (int idx = tid; idx < kWgRows * c4n; idx += kBlock) {
            const int row = idx / c4n, c4 = idx - row * c4n, s = s0 + row, r = s - p + j;
            float4 xv = make_float4(0.f, 0.f, 0.f, 0.f), dv = xv;
            if (s < L1) {
                dv = *reinterpret_cast<const float4*>(dconv + ((size_t)b * L1 + s) * C + 4 * c4);
                if (r >= 0 && r < L) {
                    const float gt = gate_in[(size_t)b * L + r];
                    xv = *reinterpret_cast<const float4*>(x + ((size_t)b * L + r) * C + 4 * c4);
                    xv.x *= gt; xv.y *= gt; xv.z *= gt; xv.w *= gt;
                }
            }
            *reinterpret_cast<float4*>(xs + row * C + 4 * c4) = xv;
            *reinterpret_cast<float4*>(ds + row * C + 4 * c4) = dv;
        }
        __syncthreads();
        if (j == 0 && tid < C)
            for (int row = 0; row < kWgRows; ++row) colsum += ds[row * C + tid];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int blk = wave + 4 * u;
            if (blk >= NT * NT) continue;
            const int mb = blk / NT, nb = blk - mb * NT;
#pragma unroll
            for (int kc = 0; kc < kWgRows / 16; ++kc)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int row = kc * 16 + 4 * g4 + e;
                    acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(xs[row * C + mb * 16 + i], ds[row * C + nb * 16 + i], acc[u], 0, 0, 0);
                }
        }
        __syncthreads();
    }
    float* out = part + ((size_t)gi * k + j) * C * C;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int blk = wave + 4 * u;
        if (blk >= NT * NT) continue;
        const int mb = blk / NT, nb = blk - mb * NT;
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(size_t)(mb * 16 + 4 * g4 + r) * C + nb * 16 + i] = acc[u][r];
    }
    if (j == 0 && tid < C) part_b[(size_t)gi * C + tid] = colsum;
}

// dW[co][ci][j] = sum over g, in order, of part[g][j][ci][co]; db[co] likewise
__global__ __launch_bounds__(kBlock) void eseq_wgrad_combine_kernel(int32_t C, int32_t k, int32_t G, const float* __restrict__ part,
                                                                   const float* __restrict__ part_b, float* __restrict__ dW,
                                                                   float* __restrict__ db) {
    const int idx = blockIdx.x * kBlock + threadIdx.x, n = k * C * C;
    if (idx < n) {
        float s = 0.f;
        for (int g = 0; g < G; ++g) s += part[(size_t)g * n + idx];
        const int j = idx / (C * C), ci = (idx / C) % C, co = idx % C;
        dW[((size_t)co * C + ci) * k + j] = s;
    }
    if (idx < C) {
        float s = 0.f;
        for (int g = 0; g < G; ++g) s += part_b[(size_t)g * C + idx];
        db[idx] = s;
    }
}

// grid (chunks of the graph row, B): the three label sets of pattern row b (padded zeros included) as LDS bit sets, then a lane per
// graph position
__global__ __launch_bounds__(kBlock) void eseq_filter_kernel(int32_t Lp, int32_t Lg, const int64_t* __restrict__ p_ul,
                                                            const int64_t* __restrict__ p_el, const int64_t* __restrict__ p_vl,
                                                            const int64_t* __restrict__ g_ul, const int64_t* __restrict__ g_el,
                                                            const int64_t* __restrict__ g_vl, uint8_t* __restrict__ out) {
    __shared__ uint32_t bits[3][kFilterCap / 32];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.y;
    for (int w = tid; w < 3 * (kFilterCap / 32); w += kBlock) (&bits[0][0])[w] = 0u;
    __syncthreads();
    const int64_t* ps[3] = {p_ul, p_el, p_vl};
    for (int idx = tid; idx < 3 * Lp; idx += kBlock) {
        const int s = idx / Lp;
        const int64_t v = ps[s][b * Lp + (idx - s * Lp)];
        if (v >= 0 && v < kFilterCap) atomicOr(&bits[s][v >> 5], 1u << (v & 31));
    }
    __syncthreads();
    const int pos = blockIdx.x * kBlock + tid;
    if (pos >= Lg) return;
    const int64_t v0 = g_ul[b * Lg + pos], v1 = g_el[b * Lg + pos], v2 = g_vl[b * Lg + pos];
    const bool in = v0 >= 0 && v0 < kFilterCap && v1 >= 0 && v1 < kFilterCap && v2 >= 0 && v2 < kFilterCap;
    out[b * Lg + pos] = in && ((bits[0][v0 >> 5] >> (v0 & 31)) & 1u) && ((bits[1][v1 >> 5] >> (v1 & 31)) & 1u) &&
                        ((bits[2][v2 >> 5] >> (v2 & 31)) & 1u);
}

int check_shape(const char* what, int64_t B, int32_t L, int32_t C, int32_t k, int32_t p) {
    DN_REQUIRE(B > 0 && L > 0 && B <= 65535 && (int64_t)B * (L + 2 * kMaxK) * kMaxC < 0x7fffffffLL, "%s: bad sizes (B = %lld, L = %d)",
               what, (long long)B, L);
    DN_REQUIRE(C >= 16 && C <= kMaxC && C % 16 == 0, "%s: C must be a multiple of 16 in 16 .. %d (got %d)", what, kMaxC, C);
    DN_REQUIRE(k >= 2 && k <= kMaxK, "%s: k must be in 2 .. %d (got %d)", what, kMaxK, k);
    DN_REQUIRE(p >= 0 && p <= k / 2, "%s: padding must be in 0 .. k / 2 (got %d for k = %d)", what, p, k);
    DN_REQUIRE(L + 4 * p - 2 * k + 2 >= 1, "%s: the sequence is too short for the two windows (L = %d, k = %d, padding %d)", what, L, k, p);
    return DN_OK;
}

int check_act(const char* what, int32_t act) {
    DN_REQUIRE(act >= 0 && act <= 2, "%s: act must be 0 (none), 1 (relu) or 2 (leaky_relu), got %d", what, act);
    return DN_OK;
}

}  // namespace

extern "C" {

int32_t dn_eseq_filter_max_labels(void) { return kFilterCap; }

int dn_eseq_conv_pool_fwd_f32(int64_t B, int32_t L, int32_t C, int32_t k, int32_t padding, int32_t act, float slope, int32_t residual,
                              const float* x, const float* gate_in, const float* wt, const float* bias, const int32_t* lo, float* y,
                              float* gate_out, uint8_t* arg, dn_stream_t stream) {
    if (int rc = check_shape("dn_eseq_conv_pool_fwd", B, L, C, k, padding)) return rc;
    if (int rc = check_act("dn_eseq_conv_pool_fwd", act)) return rc;
    DN_REQUIRE(x && gate_in && wt && bias && lo && y && gate_out && arg, "dn_eseq_conv_pool_fwd: NULL pointer");
    const int L2 = L + 4 * padding - 2 * k + 2;
    DN_REQUIRE(!residual || L2 == L, "dn_eseq_conv_pool_fwd: the residual needs a layer that keeps the length");
    const int step = kRows - (k - 1);
    hipLaunchKernelGGL(eseq_fwd_kernel, dim3((unsigned)dn_cdiv(L2, step), (unsigned)B), dim3(kBlock), 0, (hipStream_t)stream, L, C, k,
                       padding, act, act == 2 ? slope : 0.f, residual, x, gate_in, wt, bias, lo, y, gate_out, arg);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_eseq_dconv_f32(int64_t B, int32_t L, int32_t C, int32_t k, int32_t padding, int32_t act, float slope, const float* dy,
                      const float* gate_out, const uint8_t* arg, float* dconv, dn_stream_t stream) {
    if (int rc = check_shape("dn_eseq_dconv", B, L, C, k, padding)) return rc;
    if (int rc = check_act("dn_eseq_dconv", act)) return rc;
    DN_REQUIRE(dy && gate_out && arg && dconv, "dn_eseq_dconv: NULL pointer");
    const int L1 = L + 2 * padding - k + 1, L2 = L1 + 2 * padding - k + 1;
    const int64_t total = B * L1 * C;
    hipLaunchKernelGGL(eseq_dconv_kernel, dim3((unsigned)dn_cdiv(total, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, total, L1, L2, C, k,
                       padding, act, act == 2 ? slope : 0.f, dy, gate_out, arg, dconv);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_eseq_dgrad_f32(int64_t B, int32_t L, int32_t C, int32_t k, int32_t padding, int32_t residual, const float* dconv, const float* dy,
                      const float* gate_in, const float* wd, const int32_t* lo, float* dx, dn_stream_t stream) {
    if (int rc = check_shape("dn_eseq_dgrad", B, L, C, k, padding)) return rc;
    DN_REQUIRE(dconv && gate_in && wd && lo && dx && (!residual || dy), "dn_eseq_dgrad: NULL pointer");
    DN_REQUIRE(!residual || L + 4 * padding - 2 * k + 2 == L, "dn_eseq_dgrad: the residual needs a layer that keeps the length");
    hipLaunchKernelGGL(eseq_dgrad_kernel, dim3((unsigned)dn_cdiv(L, kRows), (unsigned)B), dim3(kBlock), 0, (hipStream_t)stream, L, C, k,
                       padding, residual, dconv, dy, gate_in, wd, lo, dx);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_eseq_wgrad_f32(int64_t B, int32_t L, int32_t C, int32_t k, int32_t padding, const float* x, const float* gate_in,
                      const float* dconv, const int32_t* lo, int32_t num_slices, float* part, float* part_b, dn_stream_t stream) {
    if (int rc = check_shape("dn_eseq_wgrad", B, L, C, k, padding)) return rc;
    DN_REQUIRE(num_slices >= 1 && num_slices <= 65535, "dn_eseq_wgrad: num_slices must be in 1 .. 65535 (got %d)", num_slices);
    DN_REQUIRE(x && gate_in && dconv && lo && part && part_b, "dn_eseq_wgrad: NULL pointer");
    hipLaunchKernelGGL(eseq_wgrad_kernel, dim3((unsigned)num_slices, (unsigned)k), dim3(kBlock), 0, (hipStream_t)stream, B, L, C, k, padding,
                       x, gate_in, dconv, lo, part, part_b);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_eseq_wgrad_combine_f32(int32_t C, int32_t k, int32_t num_slices, const float* part, const float* part_b, float* dW, float* db,
                              dn_stream_t stream) {
    DN_REQUIRE(C >= 16 && C <= kMaxC && C % 16 == 0, "dn_eseq_wgrad_combine: C must be a multiple of 16 in 16 .. %d (got %d)", kMaxC, C);
    DN_REQUIRE(k >= 2 && k <= kMaxK, "dn_eseq_wgrad_combine: k must be in 2 .. %d (got %d)", kMaxK, k);
    DN_REQUIRE(num_slices >= 1, "dn_eseq_wgrad_combine: num_slices must be positive (got %d)", num_slices);
    DN_REQUIRE(part && part_b && dW && db, "dn_eseq_wgrad_combine: NULL pointer");
    hipLaunchKernelGGL(eseq_wgrad_combine_kernel, dim3((unsigned)dn_cdiv((int64_t)k * C * C, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, C,
                       k, num_slices, part, part_b, dW, db);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_eseq_filter_gate_i64(int64_t B, int32_t Lp, int32_t Lg, const int64_t* p_ul, const int64_t* p_el, const int64_t* p_vl,
                            const int64_t* g_ul, const int64_t* g_el, const int64_t* g_vl, uint8_t* out, dn_stream_t stream) {
    DN_REQUIRE(B > 0 && B <= 65535 && Lp > 0 && Lg > 0 && B * (int64_t)Lg < 0x7fffffffLL && B * (int64_t)Lp < 0x7fffffffLL,
               "dn_eseq_filter_gate: bad sizes (B = %lld, Lp = %d, Lg = %d)", (long long)B, Lp, Lg);
    DN_REQUIRE(p_ul && p_el && p_vl && g_ul && g_el && g_vl && out, "dn_eseq_filter_gate: NULL pointer");
    hipLaunchKernelGGL(eseq_filter_kernel, dim3((unsigned)dn_cdiv(Lg, kBlock), (unsigned)B), dim3(kBlock), 0, (hipStream_t)stream, Lp, Lg,
                       p_ul, p_el, p_vl, g_ul, g_el, g_vl, out);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

}  // extern "C"
