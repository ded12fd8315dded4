// Ragged multi-head attention with sparsemax or softmax weights, and DIAMNet's window pooling (the SI count heads of
// subgraph_isomorphism/models/pred.py: DotAttention inside Mean / Sum / MaxAttnPredictNet and DIAMNet).
//
// B pairs; pair b owns the query rows q_ptr[b] .. q_ptr[b + 1] and the key / value rows k_ptr[b] .. k_ptr[b + 1] of already
// projected fp32 rows [N, H]; head h owns the columns h dk .. (h + 1) dk, dk = H / heads.  Per (query row i, head h):
//
//     z_j   = scale <q_i[h], k_j[h]>                     over the keys j of the pair with k_skip[j] == 0
//     p     = sparsemax(z)  or  softmax(z)                sparsemax: p_j = max(z_j - mx - tau, 0), mx = max z,
//     out_i[h] = sum_j p_j v_j[h]                                     tau from the sorted z - mx (Martins & Astudillo 2016)
//
// A row with q_skip[i] != 0, or whose pair has no live key, is a zero row.  The reference computes the same on padded
// [B, qlen, klen, heads] tensors with the masked keys at -1e30: such a key never enters the support and weighs exp(-1e30) = 0.
//
// Saved for the backward: stat [Nq, heads, 2] = {mx, tau} (softmax: {mx, sum exp(z - mx)}); nothing of size Nq x klen.
//
// Forward, one launch, the class picked on the host from the batch's largest key count:
//   * wave class (<= 64 keys): grid (B, query tiles of 32 rows), the pair's k and v rows staged in LDS with row stride H + 1 (a lane
//     per key reads its row with ds_read_b32: stride odd -> the 32 lanes of a group hit 32 banks).  A wavefront per (row, head):
//     the scores sorted by a 64-lane bitonic network of xor shuffles, an inclusive scan by up shuffles, the support size from a
//     ballot, tau from the scan value at that lane; the output columns are summed over the set bits of the support ballot only.
//   * block class (<= 1024 keys): grid (B, query tiles of 8 rows), one row at a time by the whole workgroup: the scores of all
//     heads and a copy sorted by a bitonic network sit in LDS, k and v are read from global memory (L2) as they are needed.
//   Softmax needs no sort: the maximum and the sum are reductions.
// Backward, two launches, no atomics (two runs give the same bits):
//   * dq: a wavefront per (row, head) recomputes z and p from stat, forms dP_j = <dOut_i[h], v_j[h]>, applies the Jacobian
//     (sparsemax: dz_j = [p_j > 0] (dP_j - mean of dP over the support); softmax: dz_j = p_j (dP_j - sum p dP)), writes dq and the
//     row term (the mean, or the sum) to rterm [Nq, heads] (fp64);
//   * dk / dv: min(dk, 64) lanes per (key, head) hold the key's k and v slices in registers, walk the pair's query rows in order
//     and accumulate dv_j = sum_i p_ij dOut_i and dk_j = scale sum_i dz_ij q_i in registers.
// Window pooling (DIAMNet's init_mem for mean | sum | max): see dn_seg_window_pool_fwd_f32 in include/dn_hip.h.
#include <hip/hip_runtime.h>
#include <math.h>

#include "dn_common.h"
#include "dn_hip.h"
#include "dn_rows.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxH = 256;
constexpr int kMaxHeads = 8;
constexpr int kWaveKeys = 64;
constexpr int kBlockKeys = 1024;
constexpr int kWaveQTile = 32;
constexpr int kBlockQTile = 8;
constexpr int kBwdQTile = 8;
constexpr int kMaxMem = 64;

// <a, b> over n floats, products and sum in fp64 (a product of two floats is exact there).  A score of +-80 carries an absolute error
// of 1e-5 when it is summed in fp32, which the exponential turns into a relative error of the weight; and the two backward launches
// recompute the scores in different orders, which fp64 makes agree to the last float bit in all but rare ties.
__device__ __forceinline__ double dot64(const float* a, const float* b, int n) {
    double s = 0.0;
    for (int d = 0; d < n; ++d) s = fma((double)a[d], (double)b[d], s);
    return s;
}

__device__ __forceinline__ float weight_of(bool soft, bool live, float z, float mx, float t) {
    if (!live) return 0.f;
    return soft ? expf(z - mx) / t : fmaxf(z - mx - t, 0.f);
}

// ---------------------------------------------------------------------------------------------- forward, <= 64 keys
template <bool kSoft>
__global__ __launch_bounds__(kBlock) void seg_attn_fwd_wave_kernel(int32_t H, int32_t heads, int32_t kcap, const int32_t* __restrict__ q_ptr,
                                                                   const int32_t* __restrict__ k_ptr, const uint8_t* __restrict__ q_skip,
                                                                   const uint8_t* __restrict__ k_skip, const float* __restrict__ q,
                                                                   const float* __restrict__ k, const float* __restrict__ v, float scale,
                                                                   float* __restrict__ out, float* __restrict__ stat) {
    extern __shared__ __attribute__((aligned(16))) char dn_seg_smem[];
    const int ld = H + 1;
    float* kL = reinterpret_cast<float*>(dn_seg_smem);
    float* vL = kL + (size_t)kcap * ld;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int32_t b = blockIdx.x;
    const int32_t k0 = k_ptr[b];
    const int klen = min(k_ptr[b + 1] - k0, kcap);                    // (the host picked this class from the largest key count)
    const int32_t q0 = q_ptr[b] + (int32_t)blockIdx.y * kWaveQTile;
    const int32_t q1 = min(q_ptr[b + 1], q0 + kWaveQTile);
    if (q0 >= q1) return;
    for (int i = t; i < klen * H; i += kBlock) {
        const int r = i / H, c = i - r * H;
        kL[r * ld + c] = k[(size_t)(k0 + r) * H + c];
        vL[r * ld + c] = v[(size_t)(k0 + r) * H + c];
    }
    __syncthreads();
    const int dk = H / heads;
    const bool live = lane < klen && !(k_skip != nullptr && k_skip[k0 + lane] != 0);
    const int nitems = (q1 - q0) * heads;
    for (int it = w; it < nitems; it += kWaves) {
        const int32_t row = q0 + it / heads;
        const int h = it % heads;
        float* orow = out + (size_t)row * H + h * dk;
        float* st = stat + ((size_t)row * heads + h) * 2;
        float z = -INFINITY;
        if (live) {
            const float* qr = q + (size_t)row * H + h * dk;
            const float* kr = kL + lane * ld + h * dk;
            z = (float)(dot64(qr, kr, dk) * (double)scale);
        }
        const float mx = dn_wave_max(z);
        if ((q_skip != nullptr && q_skip[row] != 0) || mx == -INFINITY) {
            for (int d = lane; d < dk; d += 64) orow[d] = 0.f;
            if (lane == 0) { st[0] = 0.f; st[1] = kSoft ? 1.f : 0.f; }
            continue;
        }
        float p, t1;
        if (kSoft) {
            const float e = live ? expf(z - mx) : 0.f;
            t1 = dn_wave_sum(e);
            p = e / t1;
        } else {
            const float zc = z - mx;                                   // (-inf on the lanes without a live key)
            t1 = dn_sparsemax_tau_wave(zc, lane, DnSupportAct());
            p = live ? fmaxf(zc - t1, 0.f) : 0.f;
        }
        if (lane == 0) { st[0] = mx; st[1] = t1; }
        const unsigned long long support = __ballot(p > 0.f);
        for (int d0 = 0; d0 < dk; d0 += 64) {
            const int d = d0 + lane;
            float acc = 0.f;
            unsigned long long m = support;
            while (m) {                                                // (wave-uniform: every lane runs the shuffle)
                const int j = __ffsll((long long)m) - 1;
                m &= m - 1;
                const float pj = __shfl(p, j, 64);
                if (d < dk) acc = fmaf(pj, vL[j * ld + h * dk + d], acc);
            }
            if (d < dk) orow[d] = acc;
        }
    }
}

// ---------------------------------------------------------------------------------------------- forward, <= 1024 keys
// LDS: sc [heads][n2] the scores, then the weights; srt [heads][n2] the sorted copy; hm / ht [kMaxHeads] mx and tau / sum per head
template <bool kSoft>
__global__ __launch_bounds__(kBlock) void seg_attn_fwd_block_kernel(int32_t H, int32_t heads, int32_t n2, const int32_t* __restrict__ q_ptr,
                                                                    const int32_t* __restrict__ k_ptr, const uint8_t* __restrict__ q_skip,
                                                                    const uint8_t* __restrict__ k_skip, const float* __restrict__ q,
                                                                    const float* __restrict__ k, const float* __restrict__ v, float scale,
                                                                    float* __restrict__ out, float* __restrict__ stat) {
    extern __shared__ __attribute__((aligned(16))) char dn_seg_smem[];
    float* sc = reinterpret_cast<float*>(dn_seg_smem);
    float* srt = sc + (size_t)heads * n2;
    float* hm = srt + (size_t)heads * n2;
    float* ht = hm + kMaxHeads;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int32_t b = blockIdx.x;
    const int32_t k0 = k_ptr[b];
    const int klen = min(k_ptr[b + 1] - k0, n2);
    const int32_t q0 = q_ptr[b] + (int32_t)blockIdx.y * kBlockQTile;
    const int32_t q1 = min(q_ptr[b + 1], q0 + kBlockQTile);
    const int dk = H / heads;
    const int total = heads * n2;
    for (int32_t row = q0; row < q1; ++row) {
        if (q_skip != nullptr && q_skip[row] != 0) {
            for (int c = t; c < H; c += kBlock) out[(size_t)row * H + c] = 0.f;
            if (t < heads) { stat[((size_t)row * heads + t) * 2] = 0.f; stat[((size_t)row * heads + t) * 2 + 1] = kSoft ? 1.f : 0.f; }
            continue;
        }
        for (int i = t; i < total; i += kBlock) {
            const int h = i / n2, j = i - h * n2;
            float z = -INFINITY;
            if (j < klen && !(k_skip != nullptr && k_skip[k0 + j] != 0)) {
                const float* qr = q + (size_t)row * H + h * dk;
                const float* kr = k + (size_t)(k0 + j) * H + h * dk;
                z = (float)(dot64(qr, kr, dk) * (double)scale);
            }
            sc[i] = z;
            if (!kSoft) srt[i] = z;
        }
        __syncthreads();
        if (!kSoft) dn_sort_desc_lists<kBlock>(srt, heads, n2, t);
        // threshold (or maximum and sum) per head: wave w takes the heads w, w + kWaves
        for (int h = w; h < heads; h += kWaves) {
            if (kSoft) {
                float m = -INFINITY;
                for (int j = lane; j < n2; j += 64) m = fmaxf(m, sc[h * n2 + j]);
                m = dn_wave_max(m);
                float s = 0.f;
                if (m > -INFINITY)
                    for (int j = lane; j < n2; j += 64) {
                        const float z = sc[h * n2 + j];
                        if (z > -INFINITY) s += expf(z - m);
                    }
                s = dn_wave_sum(s);
                if (lane == 0) { hm[h] = m; ht[h] = s; }
            } else {
                float m, tau;
                dn_sparsemax_tau_sorted(srt + (size_t)h * n2, n2, lane, DnSupportAct(), m, tau);
                if (lane == 0) { hm[h] = m; ht[h] = tau; }
            }
        }
        __syncthreads();
        for (int i = t; i < total; i += kBlock) {
            const int h = i / n2;
            const float z = sc[i];
            sc[i] = weight_of(kSoft, z > -INFINITY, z, hm[h], ht[h]);
        }
        __syncthreads();
        for (int c = t; c < H; c += kBlock) {
            const int h = c / dk;
            const float* p = sc + (size_t)h * n2;
            float acc = 0.f;
            for (int j = 0; j < klen; ++j) {
                const float pj = p[j];
                if (pj > 0.f) acc = fmaf(pj, v[(size_t)(k0 + j) * H + c], acc);
            }
            out[(size_t)row * H + c] = acc;
        }
        if (t < heads) {
            const bool none = !(hm[t] > -INFINITY);
            stat[((size_t)row * heads + t) * 2] = none ? 0.f : hm[t];
            stat[((size_t)row * heads + t) * 2 + 1] = none ? (kSoft ? 1.f : 0.f) : ht[t];
        }
        __syncthreads();                                               // (sc, hm, ht are rewritten by the next row)
    }
}

// ---------------------------------------------------------------------------------------------- backward: dq and the row terms
// LDS: dw [kWaves][kcap] fp64, pw [kWaves][kcap]: dP and the weights of the wave's current (row, head).  dP and the row term stay in
// fp64 up to their difference: where one key holds nearly all the weight, dP - term is a thousandth of either, and rounding both to
// fp32 first costs the gradient four digits.
template <bool kSoft>
__global__ __launch_bounds__(kBlock) void seg_attn_bwd_q_kernel(int32_t H, int32_t heads, int32_t kcap, const int32_t* __restrict__ q_ptr,
                                                                const int32_t* __restrict__ k_ptr, const uint8_t* __restrict__ q_skip,
                                                                const uint8_t* __restrict__ k_skip, const float* __restrict__ q,
                                                                const float* __restrict__ k, const float* __restrict__ v, float scale,
                                                                const float* __restrict__ stat, const float* __restrict__ dout,
                                                                float* __restrict__ dq, double* __restrict__ rterm) {
    extern __shared__ __attribute__((aligned(16))) char dn_seg_smem[];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    double* dw = reinterpret_cast<double*>(dn_seg_smem) + (size_t)w * kcap;
    float* pw = reinterpret_cast<float*>(reinterpret_cast<double*>(dn_seg_smem) + (size_t)kWaves * kcap) + (size_t)w * kcap;
    const int32_t b = blockIdx.x;
    const int32_t k0 = k_ptr[b];
    const int klen = min(k_ptr[b + 1] - k0, kcap);
    const int32_t q0 = q_ptr[b] + (int32_t)blockIdx.y * kBwdQTile;
    const int32_t q1 = min(q_ptr[b + 1], q0 + kBwdQTile);
    const int dk = H / heads;
    const int nitems = (q1 - q0) * heads;
    for (int base = 0; base < nitems; base += kWaves) {                // (workgroup-uniform trip count: the barriers below)
        const int it = base + w;
        const bool active = it < nitems;
        const int32_t row = q0 + (active ? it / heads : 0);
        const int h = active ? it % heads : 0;
        const bool skipped = !active || (q_skip != nullptr && q_skip[row] != 0);
        double s1 = 0.0;
        float cnt = 0.f;
        if (!skipped) {
            const float mx = stat[((size_t)row * heads + h) * 2], t1 = stat[((size_t)row * heads + h) * 2 + 1];
            const float* qr = q + (size_t)row * H + h * dk;
            const float* gr = dout + (size_t)row * H + h * dk;
            for (int j = lane; j < klen; j += 64) {
                const bool live = !(k_skip != nullptr && k_skip[k0 + j] != 0);
                const float* kr = k + (size_t)(k0 + j) * H + h * dk;
                const float* vr = v + (size_t)(k0 + j) * H + h * dk;
                const double dp = dot64(gr, vr, dk);
                const float p = weight_of(kSoft, live, (float)(dot64(qr, kr, dk) * (double)scale), mx, t1);
                pw[j] = p;
                dw[j] = dp;
                if (kSoft) s1 = fma((double)p, dp, s1);
                else if (p > 0.f) { s1 += dp; cnt += 1.f; }
            }
        }
        s1 = dn_wave_sum(s1);
        cnt = dn_wave_sum(cnt);
        const double term = kSoft ? s1 : (cnt > 0.f ? s1 / (double)cnt : 0.0);
        __syncthreads();                                               // pw / dw of the wave are written
        if (active) {
            if (lane == 0) rterm[(size_t)row * heads + h] = skipped ? 0.0 : term;
            for (int d = lane; d < dk; d += 64) {
                float acc = 0.f;
                if (!skipped)
                    for (int j = 0; j < klen; ++j) {
                        const float p = pw[j];
                        const float dz = dn_score_dz(kSoft, p, (float)(dw[j] - term));
                        if (dz != 0.f) acc = fmaf(dz, k[(size_t)(k0 + j) * H + h * dk + d], acc);
                    }
                dq[(size_t)row * H + h * dk + d] = acc * scale;
            }
        }
        __syncthreads();                                               // (the next item overwrites pw / dw)
    }
}

// ---------------------------------------------------------------------------------------------- backward: dk and dv
// G = min(dk, 64) lanes (a power of two) per (key, head); a lane owns the columns gl, gl + G, ... of the head (at most 4)
template <bool kSoft>
__global__ __launch_bounds__(kBlock) void seg_attn_bwd_kv_kernel(int32_t H, int32_t heads, int32_t G, const int32_t* __restrict__ q_ptr,
                                                                 const int32_t* __restrict__ k_ptr, const uint8_t* __restrict__ q_skip,
                                                                 const uint8_t* __restrict__ k_skip, const float* __restrict__ q,
                                                                 const float* __restrict__ k, const float* __restrict__ v, float scale,
                                                                 const float* __restrict__ stat, const double* __restrict__ rterm,
                                                                 const float* __restrict__ dout, float* __restrict__ dk_out,
                                                                 float* __restrict__ dv_out) {
    const int t = threadIdx.x;
    const int32_t b = blockIdx.x;
    const int32_t k0 = k_ptr[b];
    const int klen = k_ptr[b + 1] - k0;
    const int dk = H / heads, cpl = dk / G;
    const int item = (int)blockIdx.y * (kBlock / G) + t / G, gl = t % G;
    const bool valid = item < klen * heads;
    const int j = valid ? item / heads : 0, h = valid ? item % heads : 0;
    const size_t krow = (size_t)(k0 + j) * H + h * dk;
    const bool live = valid && !(k_skip != nullptr && k_skip[k0 + j] != 0);
    float kr[4] = {0.f, 0.f, 0.f, 0.f}, vr[4] = {0.f, 0.f, 0.f, 0.f}, ak[4] = {0.f, 0.f, 0.f, 0.f}, av[4] = {0.f, 0.f, 0.f, 0.f};
    if (valid)
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < cpl) { kr[c] = k[krow + c * G + gl]; vr[c] = v[krow + c * G + gl]; }
    const int32_t q0 = q_ptr[b], q1 = q_ptr[b + 1];
    for (int32_t i = q0; i < q1; ++i) {                                // (fixed order; workgroup-uniform: the shuffles below)
        if (q_skip != nullptr && q_skip[i] != 0) continue;
        float qv[4] = {0.f, 0.f, 0.f, 0.f}, gv[4] = {0.f, 0.f, 0.f, 0.f};
        double z = 0.0, dp = 0.0;
        if (valid) {
            const size_t qrow = (size_t)i * H + h * dk;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < cpl) {
                    qv[c] = q[qrow + c * G + gl];
                    gv[c] = dout[qrow + c * G + gl];
                    z = fma((double)qv[c], (double)kr[c], z);
                    dp = fma((double)gv[c], (double)vr[c], dp);
                }
        }
        for (int o = G >> 1; o >= 1; o >>= 1) {
            z += __shfl_xor(z, o, 64);
            dp += __shfl_xor(dp, o, 64);
        }
        if (!live) continue;
        const size_t s = (size_t)i * heads + h;
        const float p = weight_of(kSoft, true, (float)(z * (double)scale), stat[s * 2], stat[s * 2 + 1]);
        const float dz = dn_score_dz(kSoft, p, (float)(dp - rterm[s]));
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            av[c] = fmaf(p, gv[c], av[c]);
            ak[c] = fmaf(dz, qv[c], ak[c]);
        }
    }
    if (valid)
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < cpl) { dk_out[krow + c * G + gl] = ak[c] * scale; dv_out[krow + c * G + gl] = av[c]; }
}

// ---------------------------------------------------------------------------------------------- window pooling
// span [b] = {first live row, number of rows first .. last live} (0 rows: no live row)
__device__ __forceinline__ void pool_window(int L, int mem_len, int m, int* lo, int* n) {
    if (L <= mem_len) {
        const int r = m - (mem_len - L);
        *lo = r;
        *n = r >= 0 ? 1 : 0;
    } else {
        const int stride = L / mem_len;
        *lo = m * stride;
        *n = L - (mem_len - 1) * stride;
    }
}

__global__ __launch_bounds__(kBlock) void seg_window_pool_fwd_kernel(int32_t D, int32_t mem_len, int32_t mode, const int32_t* __restrict__ ptr,
                                                                     const uint8_t* __restrict__ skip, const float* __restrict__ rows,
                                                                     float* __restrict__ mem, uint8_t* __restrict__ mem_mask,
                                                                     int32_t* __restrict__ arg, int32_t* __restrict__ span) {
    __shared__ int s_lo[kWaves], s_hi[kWaves];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int32_t b = blockIdx.x;
    const int32_t r0 = ptr[b], r1 = ptr[b + 1];
    int lo = 0x7fffffff, hi = -1;
    for (int32_t r = r0 + t; r < r1; r += kBlock)
        if (skip == nullptr || skip[r] == 0) { lo = min(lo, r); hi = max(hi, r); }
    for (int o = 32; o >= 1; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o, 64));
        hi = max(hi, __shfl_xor(hi, o, 64));
    }
    if (lane == 0) { s_lo[w] = lo; s_hi[w] = hi; }
    __syncthreads();
    for (int i = 0; i < kWaves; ++i) { lo = min(lo, s_lo[i]); hi = max(hi, s_hi[i]); }
    const int L = hi >= 0 ? hi - lo + 1 : 0;
    const int32_t first = hi >= 0 ? lo : r0;
    if (t == 0) { span[2 * b] = first; span[2 * b + 1] = L; }
    for (int m = t; m < mem_len; m += kBlock) {
        int wl, wn;
        pool_window(L, mem_len, m, &wl, &wn);
        bool any = false;
        for (int i = 0; i < wn; ++i) any = any || skip == nullptr || skip[first + wl + i] == 0;
        mem_mask[(size_t)b * mem_len + m] = any ? 1 : 0;
    }
    for (int i = t; i < mem_len * D; i += kBlock) {
        const int m = i / D, c = i - m * D;
        int wl, wn;
        pool_window(L, mem_len, m, &wl, &wn);
        float acc = mode == DN_POOL_MAX ? -INFINITY : 0.f;
        int32_t best = -1;
        for (int r = 0; r < wn; ++r) {
            const int32_t rr = first + wl + r;
            const bool live = skip == nullptr || skip[rr] == 0;
            const float x = live ? rows[(size_t)rr * D + c] : 0.f;       // (a skipped row inside the span is a zero row)
            if (mode == DN_POOL_MAX) {
                if (x > acc) { acc = x; best = live ? rr : -1; }
            } else {
                acc += x;
            }
        }
        if (wn == 0) acc = 0.f;
        if (mode == DN_POOL_MEAN && wn > 1) acc /= (float)wn;
        const size_t o = ((size_t)b * mem_len + m) * D + c;
        mem[o] = acc;
        if (mode == DN_POOL_MAX) arg[o] = best;
    }
}

__global__ __launch_bounds__(kBlock) void seg_window_pool_bwd_kernel(int32_t D, int32_t mem_len, int32_t mode, const int32_t* __restrict__ ptr,
                                                                     const uint8_t* __restrict__ skip, const int32_t* __restrict__ span,
                                                                     const int32_t* __restrict__ arg, const float* __restrict__ dmem,
                                                                     float* __restrict__ drows) {
    const int32_t b = blockIdx.x;
    const int32_t r0 = ptr[b], r1 = ptr[b + 1];
    const int32_t first = span[2 * b];
    const int L = span[2 * b + 1];
    const int stride = L > mem_len ? L / mem_len : 1;
    const int kernel = L > mem_len ? L - (mem_len - 1) * stride : 1;
    const int64_t total = (int64_t)(r1 - r0) * D;
    for (int64_t i = threadIdx.x; i < total; i += kBlock) {
        const int32_t r = r0 + (int32_t)(i / D);
        const int c = (int)(i % D);
        const int rr = r - first;
        float g = 0.f;
        if (rr >= 0 && rr < L && (skip == nullptr || skip[r] == 0)) {
            if (L <= mem_len) {
                g = dmem[((size_t)b * mem_len + rr + (mem_len - L)) * D + c];
            } else {
                const int m_lo = rr >= kernel ? (rr - kernel) / stride + 1 : 0;
                const int m_hi = min(mem_len - 1, rr / stride);
                for (int m = m_lo; m <= m_hi; ++m) {                   // the at most ceil(kernel / stride) windows that hold the row
                    const size_t o = ((size_t)b * mem_len + m) * D + c;
                    if (mode == DN_POOL_MAX) {
                        if (arg[o] == r) g += dmem[o];
                    } else {
                        g += mode == DN_POOL_MEAN ? dmem[o] / (float)kernel : dmem[o];
                    }
                }
            }
        }
        drows[(size_t)r * D + c] = g;
    }
}

// ---------------------------------------------------------------------------------------------- host checks
bool pow2(int x) { return x > 0 && (x & (x - 1)) == 0; }

int check_attn(const char* what, int64_t B, int64_t Nq, int64_t Nk, int32_t H, int32_t heads, int32_t max_q, int32_t max_k, int32_t score) {
    DN_REQUIRE(B >= 1 && Nq >= 1 && Nk >= 1 && B < 0x7fffffffLL && Nq < 0x7fffffffLL / kMaxH && Nk < 0x7fffffffLL / kMaxH,
               "%s: bad sizes (B = %lld, Nq = %lld, Nk = %lld; all must be positive)", what, (long long)B, (long long)Nq, (long long)Nk);
    DN_REQUIRE(heads >= 1 && heads <= kMaxHeads && pow2(heads), "%s: heads must be 1, 2, 4 or 8 (got %d)", what, heads);
    DN_REQUIRE(H >= 1 && H <= kMaxH && H % heads == 0, "%s: 1 <= hidden <= %d with hidden %% heads == 0 (got hidden = %d, heads = %d)",
               what, kMaxH, H, heads);
    DN_REQUIRE(pow2(H / heads), "%s: the head width hidden / heads must be a power of two (got %d)", what, H / heads);
    DN_REQUIRE(max_k >= 1 && max_k <= kBlockKeys, "%s: key count over the class limit: 1 <= max_k <= %d (got %d)", what, kBlockKeys, max_k);
    DN_REQUIRE(max_q >= 1 && dn_cdiv(max_q, kBwdQTile) <= 65535, "%s: bad max_q (got %d)", what, max_q);
    return dn_check_score(what, score);
}

}  // namespace

extern "C" {

int32_t dn_seg_attn_max_keys(void) { return kBlockKeys; }
int32_t dn_seg_attn_wave_keys(void) { return kWaveKeys; }

int dn_seg_attn_fwd_f32(int64_t B, int64_t Nq, int64_t Nk, int32_t H, int32_t heads, int32_t max_q, int32_t max_k, int32_t score,
                        const int32_t* q_ptr, const int32_t* k_ptr, const uint8_t* q_skip, const uint8_t* k_skip, const float* q,
                        const float* k, const float* v, float scale, float* out, float* stat, dn_stream_t stream) {
    if (int rc = check_attn("dn_seg_attn_fwd", B, Nq, Nk, H, heads, max_q, max_k, score)) return rc;
    DN_REQUIRE(q_ptr && k_ptr && q && k && v && out && stat, "dn_seg_attn_fwd: NULL pointer");
    const bool soft = score == DN_SCORE_SOFTMAX;
    hipStream_t st = (hipStream_t)stream;
    if (max_k <= kWaveKeys) {
        const size_t lds = (size_t)2 * max_k * (H + 1) * sizeof(float);
        const dim3 grid((unsigned)B, (unsigned)dn_cdiv(max_q, kWaveQTile));
        auto kern = soft ? seg_attn_fwd_wave_kernel<true> : seg_attn_fwd_wave_kernel<false>;
        if (int rc = dn_allow_lds(kern, lds)) return rc;
        hipLaunchKernelGGL(kern, grid, dim3(kBlock), lds, st, H, heads, max_k, q_ptr, k_ptr, q_skip, k_skip, q, k, v, scale, out, stat);
    } else {
        const int n2 = dn_pow2_at_least(128, max_k);
        const size_t lds = ((size_t)2 * heads * n2 + 2 * kMaxHeads) * sizeof(float);
        const dim3 grid((unsigned)B, (unsigned)dn_cdiv(max_q, kBlockQTile));
        auto kern = soft ? seg_attn_fwd_block_kernel<true> : seg_attn_fwd_block_kernel<false>;
        if (int rc = dn_allow_lds(kern, lds)) return rc;
        hipLaunchKernelGGL(kern, grid, dim3(kBlock), lds, st, H, heads, n2, q_ptr, k_ptr, q_skip, k_skip, q, k, v, scale, out, stat);
    }
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_seg_attn_bwd_q_f32(int64_t B, int64_t Nq, int64_t Nk, int32_t H, int32_t heads, int32_t max_q, int32_t max_k, int32_t score,
                          const int32_t* q_ptr, const int32_t* k_ptr, const uint8_t* q_skip, const uint8_t* k_skip, const float* q,
                          const float* k, const float* v, float scale, const float* stat, const float* dout, float* dq, double* rterm,
                          dn_stream_t stream) {
    if (int rc = check_attn("dn_seg_attn_bwd_q", B, Nq, Nk, H, heads, max_q, max_k, score)) return rc;
    DN_REQUIRE(q_ptr && k_ptr && q && k && v && stat && dout && dq && rterm, "dn_seg_attn_bwd_q: NULL pointer");
    const size_t lds = (size_t)kWaves * max_k * (sizeof(double) + sizeof(float));
    const dim3 grid((unsigned)B, (unsigned)dn_cdiv(max_q, kBwdQTile));
    auto kern = score == DN_SCORE_SOFTMAX ? seg_attn_bwd_q_kernel<true> : seg_attn_bwd_q_kernel<false>;
    hipLaunchKernelGGL(kern, grid, dim3(kBlock), lds, (hipStream_t)stream, H, heads, max_k, q_ptr, k_ptr, q_skip, k_skip, q, k, v, scale,
                       stat, dout, dq, rterm);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_seg_attn_bwd_kv_f32(int64_t B, int64_t Nq, int64_t Nk, int32_t H, int32_t heads, int32_t max_q, int32_t max_k, int32_t score,
                           const int32_t* q_ptr, const int32_t* k_ptr, const uint8_t* q_skip, const uint8_t* k_skip, const float* q,
                           const float* k, const float* v, float scale, const float* stat, const double* rterm, const float* dout,
                           float* dk, float* dv, dn_stream_t stream) {
    if (int rc = check_attn("dn_seg_attn_bwd_kv", B, Nq, Nk, H, heads, max_q, max_k, score)) return rc;
    DN_REQUIRE(q_ptr && k_ptr && q && k && v && stat && rterm && dout && dk && dv, "dn_seg_attn_bwd_kv: NULL pointer");
    const int dkw = H / heads, G = dkw < 64 ? dkw : 64;
    const dim3 grid((unsigned)B, (unsigned)dn_cdiv((int64_t)max_k * heads, kBlock / G));
    auto kern = score == DN_SCORE_SOFTMAX ? seg_attn_bwd_kv_kernel<true> : seg_attn_bwd_kv_kernel<false>;
    hipLaunchKernelGGL(kern, grid, dim3(kBlock), 0, (hipStream_t)stream, H, heads, G, q_ptr, k_ptr, q_skip, k_skip, q, k, v, scale, stat,
                       rterm, dout, dk, dv);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

static int check_pool(const char* what, int64_t B, int64_t N, int32_t D, int32_t mem_len, int32_t mode) {
    DN_REQUIRE(B >= 1 && N >= 1 && B < 0x7fffffffLL && D >= 1 && N < 0x7fffffffLL / D, "%s: bad sizes (B = %lld, N = %lld, D = %d)", what,
               (long long)B, (long long)N, D);
    DN_REQUIRE(mem_len >= 1 && mem_len <= kMaxMem, "%s: 1 <= mem_len <= %d (got %d)", what, kMaxMem, mem_len);
    DN_REQUIRE(mode == DN_POOL_MEAN || mode == DN_POOL_SUM || mode == DN_POOL_MAX, "%s: bad mode %d", what, mode);
    return DN_OK;
}

int dn_seg_window_pool_fwd_f32(int64_t B, int64_t N, int32_t D, int32_t mem_len, int32_t mode, const int32_t* ptr, const uint8_t* skip,
                               const float* rows, float* mem, uint8_t* mem_mask, int32_t* arg, int32_t* span, dn_stream_t stream) {
    if (int rc = check_pool("dn_seg_window_pool_fwd", B, N, D, mem_len, mode)) return rc;
    DN_REQUIRE(ptr && rows && mem && mem_mask && span, "dn_seg_window_pool_fwd: NULL pointer");
    DN_REQUIRE(mode != DN_POOL_MAX || arg, "dn_seg_window_pool_fwd: max needs the arg buffer");
    hipLaunchKernelGGL(seg_window_pool_fwd_kernel, dim3((unsigned)B), dim3(kBlock), 0, (hipStream_t)stream, D, mem_len, mode, ptr, skip, rows,
                       mem, mem_mask, arg, span);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_seg_window_pool_bwd_f32(int64_t B, int64_t N, int32_t D, int32_t mem_len, int32_t mode, const int32_t* ptr, const uint8_t* skip,
                               const int32_t* span, const int32_t* arg, const float* dmem, float* drows, dn_stream_t stream) {
    if (int rc = check_pool("dn_seg_window_pool_bwd", B, N, D, mem_len, mode)) return rc;
    DN_REQUIRE(ptr && span && dmem && drows, "dn_seg_window_pool_bwd: NULL pointer");
    DN_REQUIRE(mode != DN_POOL_MAX || arg, "dn_seg_window_pool_bwd: max needs the arg buffer");
    hipLaunchKernelGGL(seg_window_pool_bwd_kernel, dim3((unsigned)B), dim3(kBlock), 0, (hipStream_t)stream, D, mem_len, mode, ptr, skip, span,
                       arg, dmem, drows);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

}  // extern "C"
