// HGP-SL pooling on ragged per-graph blocks (graph_classification/hgpsl.py; reference: models/hgpsl.py + models/sparse_softmax.py, which
// allocate a dense [N', N'] matrix over the whole pooled batch and fill its diagonal blocks in a Python loop over the graphs).
//
// B graphs; graph g owns the rows graph_ptr[g] .. graph_ptr[g + 1] of the batch and, after the pooling, the kept rows
// pooled_ptr[g] .. pooled_ptr[g + 1] (k_g = their number, computed on the host).  The per-pair storage is the ragged blocks: graph g's
// k_g x k_g block, row-major, starts at blk_ptr[g] (int64) of a [sum k_g^2] float array.  fp32, no atomics: the same bits on every run.
//
//   dn_hgpsl_dinv_f32         dinv[v] = deg[v]^-1/2 (0 where deg == 0), deg[v] = sum of w over the out-edges of v in CSR order.
//   dn_hgpsl_score_f32        score[i] = sum_f | x[i, f] - sum_{e: col = i} (dinv[row_e] w_e) dinv[i] x[row_e, f] |: a wavefront per node,
//                             the gather over the CSR by destination fused with the row sum of magnitudes; [N, H] is never written.
//   dn_hgpsl_topk_f32         per listed graph the k_g highest scores, descending, ties to the lower node: the u64 keys
//                             (~bits << 32) | local index sorted ascending (scores are >= 0: their bits order as unsigned integers).  A
//                             wavefront per graph of up to 64 nodes, a workgroup with the keys in LDS up to dn_hgpsl_topk_max_nodes().
//   dn_hgpsl_pq_f32           p[i] = <xp[i], att[:H]>, q[i] = <xp[i], att[H:]>: a wavefront per pooled row.
//   dn_hgpsl_structure_fwd_f32   per listed pooled row i of graph g: z_j = leaky_relu(p_i + q_j) + lamb A_ij over the k_g columns, A_ij
//                             gathered from the row's out-edges through the inverse map; then softmax (max subtracted, + 1e-16 in the
//                             denominator) or sparsemax.  Rows of up to 64 keys: a wavefront (shuffle sort + ballot); up to 1024 keys:
//                             a workgroup with the logits and a sorted copy in LDS.
//   dn_hgpsl_structure_bwd_*  rows: dz from the saved blocks and their gradient (softmax: o (g - <o, g>); sparsemax: g - mean over
//                             the support), dl = dz leaky', dp_i = sum_j dl_ij, the row term kept for the edge pass; cols: dq_j =
//                             sum_i dl_ij, one thread per column walking the graph's rows in order; edges: dw_e = lamb dz at the pair.
//   dn_hgpsl_att_grad_f32     datt = [sum_i dp_i xp_i, sum_j dq_j xp_j] by a fixed-order reduction in two stages (ws [dn_hgpsl_att_slabs(), 2 H]).
#include <hip/hip_runtime.h>
#include <math.h>

#include "dn_common.h"
#include "dn_hip.h"
#include "dn_rows.h"
#include "dn_wl_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxH = 512;
constexpr int kWaveKeys = 64;
constexpr int kBlockKeys = 1024;
constexpr int kTopkMaxNodes = 4096;          // 32 KB of u64 keys in LDS

__device__ __forceinline__ float leaky(float v, float slope) { return v > 0.f ? v : v * slope; }

// ---------------------------------------------------------------------------------------------- dinv and the score
__global__ __launch_bounds__(kBlock) void dinv_kernel(int64_t N, int64_t E, const int32_t* __restrict__ out_ptr,
                                                      const int32_t* __restrict__ out_perm, const float* __restrict__ w,
                                                      float* __restrict__ dinv) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= N) return;
    int64_t e0, e1;
    dn_csr_range(out_ptr, v, E, e0, e1);
    float deg = 0.f;
    for (int64_t e = e0; e < e1; ++e) deg += dn_edge_weight(w, out_perm, e, E);
    dinv[v] = deg > 0.f ? 1.f / sqrtf(deg) : 0.f;
}

__global__ __launch_bounds__(kBlock) void score_kernel(int64_t N, int64_t E, int H, const int32_t* __restrict__ in_ptr,
                                                       const int32_t* __restrict__ in_perm, const int32_t* __restrict__ src_by_dst,
                                                       const float* __restrict__ w, const float* __restrict__ dinv,
                                                       const float* __restrict__ x, float* __restrict__ score) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (i >= N) return;
    int64_t e0, e1;
    dn_csr_range(in_ptr, i, E, e0, e1);
    const float di = dinv[i];
    float total = 0.f;
    for (int f0 = 0; f0 < H; f0 += 64) {
        const int f = f0 + lane;
        float agg = 0.f;
        for (int64_t e = e0; e < e1; ++e) {                                 // (wave-uniform)
            const int64_t s = src_by_dst[e];
            if (s < 0 || s >= N) continue;
            const float coef = dinv[s] * dn_edge_weight(w, in_perm, e, E) * di;
            if (f < H) agg += coef * x[s * H + f];
        }
        if (f < H) total += fabsf(x[i * H + f] - agg);
    }
    total = dn_wave_sum(total);
    if (lane == 0) score[i] = total;
}

// ---------------------------------------------------------------------------------------------- per-graph top-k
struct TopkRange { int64_t beg; int n, k; int64_t pbeg; bool ok; };

__device__ __forceinline__ TopkRange topk_range(int64_t B, int64_t N, int64_t Np, int64_t g, const int32_t* __restrict__ gptr,
                                                const int32_t* __restrict__ pptr, int cap) {
    TopkRange r{0, 0, 0, 0, false};
    if (g < 0 || g >= B) return r;
    const int64_t beg = gptr[g], end = gptr[g + 1], pb = pptr[g], pe = pptr[g + 1];
    if (beg < 0 || end < beg || end > N || pb < 0 || pe < pb || pe > Np || end - beg > cap || pe - pb > end - beg) return r;
    r.beg = beg; r.n = (int)(end - beg); r.k = (int)(pe - pb); r.pbeg = pb; r.ok = true;
    return r;
}

__device__ __forceinline__ u64 topk_key(float s, int idx) { return ((u64)(~__float_as_uint(s)) << 32) | (unsigned)idx; }

__device__ __forceinline__ void topk_emit(const TopkRange& r, int pos, u64 key, int64_t g, int32_t* __restrict__ perm,
                                          int32_t* __restrict__ pbatch, int32_t* __restrict__ inv) {
    const int idx = (int)(unsigned)(key & 0xffffffffu);
    if (idx >= r.n) return;
    if (pos < r.k) {
        perm[r.pbeg + pos] = (int32_t)(r.beg + idx);
        pbatch[r.pbeg + pos] = (int32_t)g;
        inv[r.beg + idx] = (int32_t)(r.pbeg + pos);
    } else {
        inv[r.beg + idx] = -1;
    }
}

__global__ __launch_bounds__(kBlock) void topk_wave_kernel(int64_t B, int64_t N, int64_t Np, int64_t num_list, const int32_t* __restrict__ graphs,
                                                           const int32_t* __restrict__ gptr, const int32_t* __restrict__ pptr,
                                                           const float* __restrict__ score, int32_t* __restrict__ perm,
                                                           int32_t* __restrict__ pbatch, int32_t* __restrict__ inv) {
    const int lane = threadIdx.x & 63;
    const int64_t it = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (it >= num_list) return;
    const int64_t g = graphs[it];
    const TopkRange r = topk_range(B, N, Np, g, gptr, pptr, kWaveKeys);
    if (!r.ok) return;
    u64 key = ~0ull;
    if (lane < r.n) key = topk_key(score[r.beg + lane], lane);
    key = wl_sort_group<64>(key, lane, lane);
    if (lane < r.n) topk_emit(r, lane, key, g, perm, pbatch, inv);
}

__global__ __launch_bounds__(kBlock) void topk_block_kernel(int64_t B, int64_t N, int64_t Np, int n2, const int32_t* __restrict__ graphs,
                                                            const int32_t* __restrict__ gptr, const int32_t* __restrict__ pptr,
                                                            const float* __restrict__ score, int32_t* __restrict__ perm,
                                                            int32_t* __restrict__ pbatch, int32_t* __restrict__ inv) {
    extern __shared__ __attribute__((aligned(16))) u64 hg_keys[];
    const int tid = threadIdx.x;
    const int64_t g = graphs[blockIdx.x];
    const TopkRange r = topk_range(B, N, Np, g, gptr, pptr, n2);
    if (!r.ok) return;                                                    // (uniform over the workgroup)
    for (int i = tid; i < n2; i += kBlock) hg_keys[i] = i < r.n ? topk_key(score[r.beg + i], i) : ~0ull;
    __syncthreads();
    wl_sort_block<kBlock>(hg_keys, n2, tid);
    for (int i = tid; i < r.n; i += kBlock) topk_emit(r, i, hg_keys[i], g, perm, pbatch, inv);
}

// ---------------------------------------------------------------------------------------------- p and q
__global__ __launch_bounds__(kBlock) void pq_kernel(int64_t Np, int H, const float* __restrict__ xp, const float* __restrict__ att,
                                                    float* __restrict__ p, float* __restrict__ q) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (i >= Np) return;
    float a = 0.f, b = 0.f;
    for (int f = lane; f < H; f += 64) {
        const float v = xp[i * H + f];
        a = fmaf(v, att[f], a);
        b = fmaf(v, att[H + f], b);
    }
    a = dn_wave_sum(a);
    b = dn_wave_sum(b);
    if (lane == 0) { p[i] = a; q[i] = b; }
}

// ---------------------------------------------------------------------------------------------- structure learning
struct RowAt { int64_t i; int64_t c0; int k; int64_t at; bool ok; };   // pooled row, its graph's first pooled row, its size, its block row

__device__ __forceinline__ RowAt row_at(int64_t B, int64_t Np, int64_t T, int64_t i, const int32_t* __restrict__ pptr,
                                        const int64_t* __restrict__ bptr, const int32_t* __restrict__ pbatch, int cap) {
    RowAt r{i, 0, 0, 0, false};
    if (i < 0 || i >= Np) return r;
    const int64_t g = pbatch[i];
    if (g < 0 || g >= B) return r;
    const int64_t c0 = pptr[g], c1 = pptr[g + 1], k = c1 - c0, b0 = bptr[g];
    if (c0 < 0 || c1 > Np || i < c0 || i >= c1 || k > cap || b0 < 0 || b0 + k * k > T) return r;
    r.c0 = c0; r.k = (int)k; r.at = b0 + (i - c0) * k; r.ok = true;
    return r;
}

template <bool kSoft>
__global__ __launch_bounds__(kBlock) void structure_fwd_wave_kernel(int64_t B, int64_t N, int64_t E, int64_t Np, int64_t T, int64_t num_rows,
                                                                    const int32_t* __restrict__ rows, const int32_t* __restrict__ pptr,
                                                                    const int64_t* __restrict__ bptr, const int32_t* __restrict__ pbatch,
                                                                    const int32_t* __restrict__ perm, const int32_t* __restrict__ inv,
                                                                    const int32_t* __restrict__ out_ptr, const int32_t* __restrict__ out_perm,
                                                                    const int32_t* __restrict__ dst_by_src, const float* __restrict__ w,
                                                                    const float* __restrict__ p, const float* __restrict__ q, float lamb,
                                                                    float slope, float* __restrict__ blocks) {
    const int lane = threadIdx.x & 63;
    const int64_t it = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (it >= num_rows) return;
    const RowAt r = row_at(B, Np, T, rows[it], pptr, bptr, pbatch, kWaveKeys);
    if (!r.ok) return;                                                    // (uniform over the wavefront)
    const bool live = lane < r.k;
    float z = live ? leaky(p[r.i] + q[r.c0 + lane], slope) : -INFINITY;
    const int64_t node = perm[r.i];
    if (node >= 0 && node < N) {
        int64_t e0, e1;
        dn_csr_range(out_ptr, node, E, e0, e1);
        for (int64_t e = e0; e < e1; ++e) {                                 // every lane reads the same edge; the pairs are unique
            const int64_t c = dst_by_src[e];
            if (c < 0 || c >= N) continue;
            if ((int64_t)inv[c] != r.c0 + lane || !live) continue;
            z += dn_edge_weight(w, out_perm, e, E) * lamb;
        }
    }
    const float mx = dn_wave_max(z);
    float o;
    if (kSoft) {
        const float ex = live ? expf(z - mx) : 0.f;
        const float s = dn_wave_sum(ex);
        o = ex / (s + 1e-16f);
    } else {
        const float zc = z - mx;                                           // (-inf on the lanes past the row)
        const float tau = dn_sparsemax_tau_wave(zc, lane, DnSupportOps());
        o = live ? fmaxf(zc - tau, 0.f) : 0.f;
    }
    if (live) blocks[r.at + lane] = o;
}

// LDS: zs [n2] the logits, srt [n2] their sorted copy (sparsemax), st [2] = {max, sum or tau}
template <bool kSoft>
__global__ __launch_bounds__(kBlock) void structure_fwd_block_kernel(int64_t B, int64_t N, int64_t E, int64_t Np, int64_t T, int n2,
                                                                     const int32_t* __restrict__ rows, const int32_t* __restrict__ pptr,
                                                                     const int64_t* __restrict__ bptr, const int32_t* __restrict__ pbatch,
                                                                     const int32_t* __restrict__ perm, const int32_t* __restrict__ inv,
                                                                     const int32_t* __restrict__ out_ptr, const int32_t* __restrict__ out_perm,
                                                                     const int32_t* __restrict__ dst_by_src, const float* __restrict__ w,
                                                                     const float* __restrict__ p, const float* __restrict__ q, float lamb,
                                                                     float slope, float* __restrict__ blocks) {
    extern __shared__ __attribute__((aligned(16))) float hg_smem[];
    float* zs = hg_smem;
    float* srt = zs + n2;
    float* st = srt + n2;
    const int tid = threadIdx.x, lane = tid & 63;
    const RowAt r = row_at(B, Np, T, rows[blockIdx.x], pptr, bptr, pbatch, n2 < kBlockKeys ? n2 : kBlockKeys);
    if (!r.ok) return;                                                    // (uniform over the workgroup)
    const float pi = p[r.i];
    for (int j = tid; j < n2; j += kBlock) zs[j] = j < r.k ? leaky(pi + q[r.c0 + j], slope) : -INFINITY;
    __syncthreads();
    const int64_t node = perm[r.i];
    if (node >= 0 && node < N) {
        int64_t e0, e1;
        dn_csr_range(out_ptr, node, E, e0, e1);
        for (int64_t e = e0 + tid; e < e1; e += kBlock) {                   // the pairs are unique: every slot has one writer
            const int64_t c = dst_by_src[e];
            if (c < 0 || c >= N) continue;
            const int64_t j = (int64_t)inv[c] - r.c0;
            if (j < 0 || j >= r.k) continue;
            zs[j] += dn_edge_weight(w, out_perm, e, E) * lamb;
        }
    }
    __syncthreads();
    if (!kSoft) {
        for (int j = tid; j < n2; j += kBlock) srt[j] = zs[j];
        __syncthreads();
        dn_sort_desc_lists<kBlock>(srt, 1, n2, tid);
    }
    if (tid < 64) {                                                       // the first wavefront: the maximum and the sum, or the threshold
        if (kSoft) {
            float m = -INFINITY;
            for (int j = lane; j < n2; j += 64) m = fmaxf(m, zs[j]);
            m = dn_wave_max(m);
            float s = 0.f;
            for (int j = lane; j < r.k; j += 64) s += expf(zs[j] - m);
            s = dn_wave_sum(s);
            if (lane == 0) { st[0] = m; st[1] = s; }
        } else {
            float m, tau;
            dn_sparsemax_tau_sorted(srt, n2, lane, DnSupportOps(), m, tau);
            if (lane == 0) { st[0] = m; st[1] = tau; }
        }
    }
    __syncthreads();
    const float m = st[0], t = st[1];
    for (int j = tid; j < r.k; j += kBlock)
        blocks[r.at + j] = kSoft ? expf(zs[j] - m) / (t + 1e-16f) : fmaxf(zs[j] - m - t, 0.f);
}

// A wavefront per listed row, the lanes striding over its columns (any k): the output row and its gradient decide dz; the sign of
// p_i + q_j decides the leaky slope.  No logit is recomputed.
template <bool kSoft>
__global__ __launch_bounds__(kBlock) void structure_bwd_rows_kernel(int64_t B, int64_t Np, int64_t T, int64_t num_rows,
                                                                    const int32_t* __restrict__ rows, const int32_t* __restrict__ pptr,
                                                                    const int64_t* __restrict__ bptr, const int32_t* __restrict__ pbatch,
                                                                    const float* __restrict__ p, const float* __restrict__ q, float slope,
                                                                    const float* __restrict__ blocks, const float* __restrict__ dblocks,
                                                                    float* __restrict__ dl, float* __restrict__ dp, float* __restrict__ rterm) {
    const int lane = threadIdx.x & 63;
    const int64_t it = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (it >= num_rows) return;
    const RowAt r = row_at(B, Np, T, rows[it], pptr, bptr, pbatch, kBlockKeys);
    if (!r.ok) return;
    float s1 = 0.f, cnt = 0.f;
    for (int j = lane; j < r.k; j += 64) {
        const float o = blocks[r.at + j], g = dblocks[r.at + j];
        if (kSoft) s1 = fmaf(o, g, s1);
        else if (o > 0.f) { s1 += g; cnt += 1.f; }
    }
    s1 = dn_wave_sum(s1);
    cnt = dn_wave_sum(cnt);
    const float term = kSoft ? s1 : (cnt > 0.f ? s1 / cnt : 0.f);
    const float pi = p[r.i];
    float acc = 0.f;
    for (int j = lane; j < r.k; j += 64) {
        const float o = blocks[r.at + j], g = dblocks[r.at + j];
        const float dz = dn_score_dz(kSoft, o, g - term);
        const float d = pi + q[r.c0 + j] > 0.f ? dz : dz * slope;
        dl[r.at + j] = d;
        acc += d;
    }
    acc = dn_wave_sum(acc);
    if (lane == 0) { dp[r.i] = acc; rterm[r.i] = term; }
}

__global__ __launch_bounds__(kBlock) void structure_bwd_cols_kernel(int64_t B, int64_t Np, int64_t T, int64_t num_rows,
                                                                    const int32_t* __restrict__ rows, const int32_t* __restrict__ pptr,
                                                                    const int64_t* __restrict__ bptr, const int32_t* __restrict__ pbatch,
                                                                    const float* __restrict__ dl, float* __restrict__ dq) {
    const int64_t it = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (it >= num_rows) return;
    const RowAt r = row_at(B, Np, T, rows[it], pptr, bptr, pbatch, kBlockKeys);
    if (!r.ok) return;
    const int64_t col = r.at - (r.i - r.c0) * r.k + (r.i - r.c0);         // block start + the column of this pooled node
    float acc = 0.f;
    for (int i = 0; i < r.k; ++i) acc += dl[col + (int64_t)i * r.k];      // the graph's rows in order
    dq[r.i] = acc;
}

template <bool kSoft>
__global__ __launch_bounds__(kBlock) void structure_bwd_edges_kernel(int64_t B, int64_t N, int64_t E, int64_t Np, int64_t T,
                                                                     const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                                                     const int32_t* __restrict__ inv, const int32_t* __restrict__ pptr,
                                                                     const int64_t* __restrict__ bptr, const int32_t* __restrict__ pbatch,
                                                                     const float* __restrict__ blocks, const float* __restrict__ dblocks,
                                                                     const float* __restrict__ rterm, float lamb, float* __restrict__ dw) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= E) return;
    float out = 0.f;
    const int64_t a = src[e], b = dst[e];
    if (a >= 0 && a < N && b >= 0 && b < N) {
        const int64_t i = inv[a], j = inv[b];
        if (i >= 0 && j >= 0 && j < Np) {
            const RowAt r = row_at(B, Np, T, i, pptr, bptr, pbatch, kBlockKeys);
            if (r.ok && j >= r.c0 && j < r.c0 + r.k) {
                const float o = blocks[r.at + (j - r.c0)], g = dblocks[r.at + (j - r.c0)];
                out = lamb * dn_score_dz(kSoft, o, g - rterm[i]);
            }
        }
    }
    dw[e] = out;
}

// datt[c] = sum_i dp_i xp[i, c], datt[H + c] = sum_j dq_j xp[j, c] in two fixed-order stages: workgroup (x, y) owns 64 columns and the
// y-th of kAttSlabs equal row slabs, wave w its rows w, w + 4, ... in order, the four partial sums added in wave order into
// ws [kAttSlabs, 2 H]; the fold adds the slabs in order.
constexpr int kAttSlabs = 64;

__global__ __launch_bounds__(kBlock) void att_grad_kernel(int64_t Np, int H, const float* __restrict__ xp, const float* __restrict__ dp,
                                                          const float* __restrict__ dq, float* __restrict__ ws) {
    __shared__ float part[2][kWaves][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const int64_t chunk = (Np + kAttSlabs - 1) / kAttSlabs, r0 = (int64_t)blockIdx.y * chunk, r1 = r0 + chunk < Np ? r0 + chunk : Np;
    float a = 0.f, b = 0.f;
    if (c < H)
        for (int64_t i = r0 + wave; i < r1; i += kWaves) {
            const float v = xp[i * H + c];
            a = fmaf(dp[i], v, a);
            b = fmaf(dq[i], v, b);
        }
    part[0][wave][lane] = a;
    part[1][wave][lane] = b;
    __syncthreads();
    if (wave == 0 && c < H) {
        float sa = 0.f, sb = 0.f;
        for (int wv = 0; wv < kWaves; ++wv) { sa += part[0][wv][lane]; sb += part[1][wv][lane]; }
        ws[(size_t)blockIdx.y * 2 * H + c] = sa;
        ws[(size_t)blockIdx.y * 2 * H + H + c] = sb;
    }
}

__global__ __launch_bounds__(kBlock) void att_fold_kernel(int H, const float* __restrict__ ws, float* __restrict__ datt) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= 2 * H) return;
    float s = 0.f;
    for (int y = 0; y < kAttSlabs; ++y) s += ws[(size_t)y * 2 * H + c];
    datt[c] = s;
}

// ---------------------------------------------------------------------------------------------- host checks
int check_batch(const char* what, int64_t N, int64_t E) {
    DN_REQUIRE(N >= 1 && N < 0x7fffffffLL / kMaxH && E >= 0 && E < 0x7fffffffLL, "%s: bad sizes (N = %lld, E = %lld)", what, (long long)N,
               (long long)E);
    return DN_OK;
}

int check_pooled(const char* what, int64_t B, int64_t Np, int64_t T) {
    DN_REQUIRE(B >= 1 && B < 0x7fffffffLL && Np >= 1 && Np < 0x7fffffffLL / kMaxH && T >= Np && T < (1LL << 40),
               "%s: bad sizes (B = %lld, pooled rows = %lld, block floats = %lld)", what, (long long)B, (long long)Np, (long long)T);
    return DN_OK;
}

int check_h(const char* what, int32_t H) {
    DN_REQUIRE(H >= 1 && H <= kMaxH, "%s: 1 <= H <= %d feature columns (got %d)", what, kMaxH, H);
    return DN_OK;
}

}  // namespace

extern "C" {

int32_t dn_hgpsl_topk_max_nodes(void) { return kTopkMaxNodes; }
int32_t dn_hgpsl_wave_keys(void) { return kWaveKeys; }
int32_t dn_hgpsl_max_keys(void) { return kBlockKeys; }
int32_t dn_hgpsl_max_features(void) { return kMaxH; }

int dn_hgpsl_dinv_f32(int64_t N, int64_t E, const int32_t* out_ptr, const int32_t* out_perm, const float* w, float* dinv,
                      dn_stream_t stream) {
    if (int rc = check_batch("dn_hgpsl_dinv", N, E)) return rc;
    DN_REQUIRE(out_ptr && dinv && (!w || out_perm || E == 0), "dn_hgpsl_dinv: NULL pointer");
    hipLaunchKernelGGL(dinv_kernel, dim3((unsigned)dn_cdiv(N, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, N, E, out_ptr, out_perm, w, dinv);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_hgpsl_score_f32(int64_t N, int64_t E, int32_t H, const int32_t* in_ptr, const int32_t* in_perm, const int32_t* src_by_dst,
                       const float* w, const float* dinv, const float* x, float* score, dn_stream_t stream) {
    if (int rc = check_batch("dn_hgpsl_score", N, E)) return rc;
    if (int rc = check_h("dn_hgpsl_score", H)) return rc;
    DN_REQUIRE(in_ptr && dinv && x && score && (src_by_dst || E == 0) && (!w || in_perm || E == 0), "dn_hgpsl_score: NULL pointer");
    hipLaunchKernelGGL(score_kernel, dim3((unsigned)dn_cdiv(N, kWaves)), dim3(kBlock), 0, (hipStream_t)stream, N, E, H, in_ptr, in_perm,
                       src_by_dst, w, dinv, x, score);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_hgpsl_topk_f32(int64_t B, int64_t N, int64_t Np, int64_t num_list, int32_t max_nodes, const int32_t* graphs,
                      const int32_t* graph_ptr, const int32_t* pooled_ptr, const float* score, int32_t* perm, int32_t* pooled_batch,
                      int32_t* inv, dn_stream_t stream) {
    DN_REQUIRE(B >= 1 && B < 0x7fffffffLL && N >= 1 && N < 0x7fffffffLL && Np >= 1 && Np <= N && num_list >= 1 && num_list <= B,
               "dn_hgpsl_topk: bad sizes (B = %lld, N = %lld, pooled rows = %lld, listed = %lld)", (long long)B, (long long)N, (long long)Np,
               (long long)num_list);
    DN_REQUIRE(max_nodes >= 1 && max_nodes <= kTopkMaxNodes, "dn_hgpsl_topk: graph over the class limit: 1 <= max_nodes <= %d (got %d)",
               kTopkMaxNodes, max_nodes);
    DN_REQUIRE(graphs && graph_ptr && pooled_ptr && score && perm && pooled_batch && inv, "dn_hgpsl_topk: NULL pointer");
    if (max_nodes <= kWaveKeys) {
        hipLaunchKernelGGL(topk_wave_kernel, dim3((unsigned)dn_cdiv(num_list, kWaves)), dim3(kBlock), 0, (hipStream_t)stream, B, N, Np, num_list,
                           graphs, graph_ptr, pooled_ptr, score, perm, pooled_batch, inv);
    } else {
        const int n2 = dn_pow2_at_least(128, max_nodes);
        hipLaunchKernelGGL(topk_block_kernel, dim3((unsigned)num_list), dim3(kBlock), (size_t)n2 * sizeof(u64), (hipStream_t)stream, B, N, Np, n2,
                           graphs, graph_ptr, pooled_ptr, score, perm, pooled_batch, inv);
    }
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_hgpsl_pq_f32(int64_t Np, int32_t H, const float* xp, const float* att, float* p, float* q, dn_stream_t stream) {
    DN_REQUIRE(Np >= 1 && Np < 0x7fffffffLL / kMaxH, "dn_hgpsl_pq: bad sizes (pooled rows = %lld)", (long long)Np);
    if (int rc = check_h("dn_hgpsl_pq", H)) return rc;
    DN_REQUIRE(xp && att && p && q, "dn_hgpsl_pq: NULL pointer");
    hipLaunchKernelGGL(pq_kernel, dim3((unsigned)dn_cdiv(Np, kWaves)), dim3(kBlock), 0, (hipStream_t)stream, Np, H, xp, att, p, q);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_hgpsl_structure_fwd_f32(int64_t B, int64_t N, int64_t E, int64_t Np, int64_t T, int64_t num_rows, int32_t max_keys, int32_t score,
                               const int32_t* rows, const int32_t* pooled_ptr, const int64_t* blk_ptr, const int32_t* pooled_batch,
                               const int32_t* perm, const int32_t* inv, const int32_t* out_ptr, const int32_t* out_perm,
                               const int32_t* dst_by_src, const float* w, const float* p, const float* q, float lamb, float slope,
                               float* blocks, dn_stream_t stream) {
    if (int rc = check_batch("dn_hgpsl_structure_fwd", N, E)) return rc;
    if (int rc = check_pooled("dn_hgpsl_structure_fwd", B, Np, T)) return rc;
    DN_REQUIRE(num_rows >= 1 && num_rows <= Np, "dn_hgpsl_structure_fwd: bad list (%lld rows listed of %lld)", (long long)num_rows,
               (long long)Np);
    DN_REQUIRE(max_keys >= 1 && max_keys <= kBlockKeys, "dn_hgpsl_structure_fwd: key count over the class limit: 1 <= max_keys <= %d (got %d)",
               kBlockKeys, max_keys);
    if (int rc = dn_check_score("dn_hgpsl_structure_fwd", score)) return rc;
    DN_REQUIRE(rows && pooled_ptr && blk_ptr && pooled_batch && perm && inv && out_ptr && p && q && blocks && (dst_by_src || E == 0) &&
                   (!w || out_perm || E == 0),
               "dn_hgpsl_structure_fwd: NULL pointer");
    const bool soft = score == DN_SCORE_SOFTMAX;
    hipStream_t st = (hipStream_t)stream;
    if (max_keys <= kWaveKeys) {
        auto kern = soft ? structure_fwd_wave_kernel<true> : structure_fwd_wave_kernel<false>;
        hipLaunchKernelGGL(kern, dim3((unsigned)dn_cdiv(num_rows, kWaves)), dim3(kBlock), 0, st, B, N, E, Np, T, num_rows, rows, pooled_ptr,
                           blk_ptr, pooled_batch, perm, inv, out_ptr, out_perm, dst_by_src, w, p, q, lamb, slope, blocks);
    } else {
        const int n2 = dn_pow2_at_least(128, max_keys);
        auto kern = soft ? structure_fwd_block_kernel<true> : structure_fwd_block_kernel<false>;
        hipLaunchKernelGGL(kern, dim3((unsigned)num_rows), dim3(kBlock), ((size_t)2 * n2 + 2) * sizeof(float), st, B, N, E, Np, T, n2, rows,
                           pooled_ptr, blk_ptr, pooled_batch, perm, inv, out_ptr, out_perm, dst_by_src, w, p, q, lamb, slope, blocks);
    }
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_hgpsl_structure_bwd_rows_f32(int64_t B, int64_t Np, int64_t T, int64_t num_rows, int32_t score, const int32_t* rows,
                                    const int32_t* pooled_ptr, const int64_t* blk_ptr, const int32_t* pooled_batch, const float* p,
                                    const float* q, float slope, const float* blocks, const float* dblocks, float* dl, float* dp,
                                    float* rterm, dn_stream_t stream) {
    if (int rc = check_pooled("dn_hgpsl_structure_bwd_rows", B, Np, T)) return rc;
    DN_REQUIRE(num_rows >= 1 && num_rows <= Np, "dn_hgpsl_structure_bwd_rows: bad list (%lld rows listed of %lld)", (long long)num_rows,
               (long long)Np);
    if (int rc = dn_check_score("dn_hgpsl_structure_bwd_rows", score)) return rc;
    DN_REQUIRE(rows && pooled_ptr && blk_ptr && pooled_batch && p && q && blocks && dblocks && dl && dp && rterm,
               "dn_hgpsl_structure_bwd_rows: NULL pointer");
    auto kern = score == DN_SCORE_SOFTMAX ? structure_bwd_rows_kernel<true> : structure_bwd_rows_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)dn_cdiv(num_rows, kWaves)), dim3(kBlock), 0, (hipStream_t)stream, B, Np, T, num_rows, rows, pooled_ptr,
                       blk_ptr, pooled_batch, p, q, slope, blocks, dblocks, dl, dp, rterm);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_hgpsl_structure_bwd_cols_f32(int64_t B, int64_t Np, int64_t T, int64_t num_rows, const int32_t* rows, const int32_t* pooled_ptr,
                                    const int64_t* blk_ptr, const int32_t* pooled_batch, const float* dl, float* dq, dn_stream_t stream) {
    if (int rc = check_pooled("dn_hgpsl_structure_bwd_cols", B, Np, T)) return rc;
    DN_REQUIRE(num_rows >= 1 && num_rows <= Np, "dn_hgpsl_structure_bwd_cols: bad list (%lld rows listed of %lld)", (long long)num_rows,
               (long long)Np);
    DN_REQUIRE(rows && pooled_ptr && blk_ptr && pooled_batch && dl && dq, "dn_hgpsl_structure_bwd_cols: NULL pointer");
    hipLaunchKernelGGL(structure_bwd_cols_kernel, dim3((unsigned)dn_cdiv(num_rows, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, B, Np, T,
                       num_rows, rows, pooled_ptr, blk_ptr, pooled_batch, dl, dq);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_hgpsl_structure_bwd_edges_f32(int64_t B, int64_t N, int64_t E, int64_t Np, int64_t T, int32_t score, const int32_t* src,
                                     const int32_t* dst, const int32_t* inv, const int32_t* pooled_ptr, const int64_t* blk_ptr,
                                     const int32_t* pooled_batch, const float* blocks, const float* dblocks, const float* rterm, float lamb,
                                     float* dw, dn_stream_t stream) {
    if (int rc = check_batch("dn_hgpsl_structure_bwd_edges", N, E)) return rc;
    DN_REQUIRE(E >= 1, "dn_hgpsl_structure_bwd_edges: bad sizes (E = %lld; must be positive)", (long long)E);
    if (int rc = check_pooled("dn_hgpsl_structure_bwd_edges", B, Np, T)) return rc;
    if (int rc = dn_check_score("dn_hgpsl_structure_bwd_edges", score)) return rc;
    DN_REQUIRE(src && dst && inv && pooled_ptr && blk_ptr && pooled_batch && blocks && dblocks && rterm && dw,
               "dn_hgpsl_structure_bwd_edges: NULL pointer");
    auto kern = score == DN_SCORE_SOFTMAX ? structure_bwd_edges_kernel<true> : structure_bwd_edges_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)dn_cdiv(E, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, B, N, E, Np, T, src, dst, inv, pooled_ptr,
                       blk_ptr, pooled_batch, blocks, dblocks, rterm, lamb, dw);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int32_t dn_hgpsl_att_slabs(void) { return kAttSlabs; }

int dn_hgpsl_att_grad_f32(int64_t Np, int32_t H, const float* xp, const float* dp, const float* dq, float* ws, float* datt,
                          dn_stream_t stream) {
    DN_REQUIRE(Np >= 1 && Np < 0x7fffffffLL / kMaxH, "dn_hgpsl_att_grad: bad sizes (pooled rows = %lld)", (long long)Np);
    if (int rc = check_h("dn_hgpsl_att_grad", H)) return rc;
    DN_REQUIRE(xp && dp && dq && ws && datt, "dn_hgpsl_att_grad: NULL pointer");
    hipLaunchKernelGGL(att_grad_kernel, dim3((unsigned)dn_cdiv(H, 64), kAttSlabs), dim3(kBlock), 0, (hipStream_t)stream, Np, H, xp, dp, dq, ws);
    DN_CHECK_LAUNCH();
    hipLaunchKernelGGL(att_fold_kernel, dim3((unsigned)dn_cdiv(2 * H, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, H, ws, datt);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

}  // extern "C"
