// The glue of the SI count models around the representation nets (GraphAdjModel.forward, subgraph_isomorphism/models/
// basemodel.py:887-982): label filter, code embedding, ragged head pooling and the padded node masks.  All of it is
// per-graph or per-row work on a ragged batch (node_ptr), so every kernel walks the rows of a graph in order: no float
// atomics, fixed-order fp32 sums, results bit-identical from run to run.  Ids / labels are checked ONCE, by
// dn_si_filter_meta_*, which also writes the two padded lengths; the caller reads those four ints back in one copy.  The
// later kernels still clamp every table read (an out-of-range key reads zeros), so a bad batch never reads out of bounds.
#include "dn_common.h"
#include "../../include/dn_hip.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWgradChunk = 32;                   // rows a workgroup of the embedding weight gradient sums
constexpr int kWgradMaxH = 256;                   // (its LDS stage: kWgradChunk x H gradient rows, kWgradChunk x K encoder rows)
constexpr int kWgradMaxK = 64;
constexpr int kEmbedMaxLds = 16384;               // fp32 words of the two staged embedding weights (64 KB)

// meta = {Lp, Lg, flags, 0}: Lp / Lg = longest pattern / graph of the batch.  Every block reduces the pattern lengths itself
// (B int loads, L2-resident) so that the label-0 rule below needs no second launch.
template <typename T>
__global__ __launch_bounds__(kBlock) void filter_meta_kernel(
    int64_t B, const int32_t* __restrict__ p_ptr, const int32_t* __restrict__ p_label, const int32_t* __restrict__ p_id, int64_t Np,
    const int32_t* __restrict__ g_ptr, const int32_t* __restrict__ g_label, const int32_t* __restrict__ g_id, int64_t Ng,
    int32_t p_nlab, int32_t p_nid, int32_t g_nlab, int32_t g_nid, T* __restrict__ gate, int32_t* __restrict__ meta) {
    __shared__ int s_max[2][kBlock / 64];
    __shared__ int s_flag;
    const int tid = threadIdx.x;
    if (tid == 0) s_flag = 0;
    int mp = 0, mg = 0, flag = 0;
    for (int64_t i = tid; i < B; i += kBlock) {
        const int lp = p_ptr[i + 1] - p_ptr[i], lg = g_ptr[i + 1] - g_ptr[i];
        mp = max(mp, lp);
        mg = max(mg, lg);
        if (lp <= 0) flag |= DN_SI_ZERO_PATTERN;
        if (lg <= 0) flag |= DN_SI_ZERO_GRAPH;
    }
    for (int o = 32; o > 0; o >>= 1) {
        mp = max(mp, __shfl_xor(mp, o));
        mg = max(mg, __shfl_xor(mg, o));
    }
    if ((tid & 63) == 0) { s_max[0][tid >> 6] = mp; s_max[1][tid >> 6] = mg; }
    __syncthreads();
    mp = max(max(s_max[0][0], s_max[0][1]), max(s_max[0][2], s_max[0][3]));
    mg = max(max(s_max[1][0], s_max[1][1]), max(s_max[1][2], s_max[1][3]));
    const int64_t b = blockIdx.x;
    if (b == 0 && tid == 0) {
        meta[0] = mp;
        meta[1] = mg;
        if (p_ptr[0] != 0 || p_ptr[B] != Np) flag |= DN_SI_BAD_PTR;
        if (g_ptr[0] != 0 || g_ptr[B] != Ng) flag |= DN_SI_BAD_PTR;
    }
    int p0 = p_ptr[b], p1 = p_ptr[b + 1];
    int g0 = g_ptr[b], g1 = g_ptr[b + 1];
    if (p0 < 0 || p1 < p0 || p1 > Np || g0 < 0 || g1 < g0 || g1 > Ng) {   // a broken ptr reads nothing
        flag |= DN_SI_BAD_PTR;
        p0 = p1 = g0 = g1 = 0;
    }
    const bool short_pattern = p1 - p0 < mp;     // front-padded with label 0 by the reference (basemodel.py:838)
    for (int j = p0 + tid; j < p1; j += kBlock) {
        const int l = p_label[j], id = p_id[j];
        if (l < 0 || l >= p_nlab) flag |= DN_SI_BAD_LABEL;
        if (id < 0 || id >= p_nid) flag |= DN_SI_BAD_ID;
    }
    for (int v = g0 + tid; v < g1; v += kBlock) {
        const int l = g_label[v], id = g_id[v];
        if (l < 0 || l >= g_nlab) flag |= DN_SI_BAD_LABEL;
        if (id < 0 || id >= g_nid) flag |= DN_SI_BAD_ID;
        if (gate != nullptr) {
            bool hit = short_pattern && l == 0;
            for (int j = p0; j < p1 && !hit; ++j) hit = p_label[j] == l;   // same address across the wave: one broadcast load
            gate[v] = st<T>(hit ? 1.f : 0.f);
        }
    }
    if (flag) atomicOr(&s_flag, flag);
    __syncthreads();
    if (tid == 0 && s_flag) atomicOr(&meta[2], s_flag);                    // (integer flag bits: order does not matter)
}

// out[v, h] = sum_k enc1[key1[v], k] W1[k, h] (+ the same over table 2).  Both W staged in LDS as fp32.
template <typename T>
__global__ __launch_bounds__(kBlock) void embed_fwd_kernel(
    int64_t N, int32_t H, const int32_t* __restrict__ key1, const T* __restrict__ enc1, int32_t rows1, int32_t K1,
    const T* __restrict__ W1, const int32_t* __restrict__ key2, const T* __restrict__ enc2, int32_t rows2, int32_t K2,
    const T* __restrict__ W2, T* __restrict__ out) {
    extern __shared__ float s_w[];
    const int n1 = K1 * H, n2 = key2 ? K2 * H : 0;
    for (int i = threadIdx.x; i < n1; i += kBlock) s_w[i] = ld(W1, i);
    for (int i = threadIdx.x; i < n2; i += kBlock) s_w[n1 + i] = ld(W2, i);
    __syncthreads();
    const int64_t total = N * H;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int64_t v = i / H;
        const int h = (int)(i - v * H);
        float acc = 0.f;
        const int k1 = key1[v];
        if (k1 >= 0 && k1 < rows1)
            for (int k = 0; k < K1; ++k) acc = fmaf(ld(enc1, (int64_t)k1 * K1 + k), s_w[k * H + h], acc);
        if (key2 != nullptr) {
            float acc2 = 0.f;
            const int k2 = key2[v];
            if (k2 >= 0 && k2 < rows2)
                for (int k = 0; k < K2; ++k) acc2 = fmaf(ld(enc2, (int64_t)k2 * K2 + k), s_w[n1 + k * H + h], acc2);
            acc += acc2;                                                   // emb_vl + emb_v (basemodel.py:864-866)
        }
        out[i] = st<T>(acc);
    }
}

// part[c, k, h] = sum over the rows of chunk c (in order) of enc[key[v], k] G[v, h].  The chunk's gradient rows and encoder rows
// are staged in LDS first (coalesced loads), so the products run from LDS; small chunks keep enough workgroups in flight.
template <typename T>
__global__ __launch_bounds__(kBlock) void embed_wgrad_part_kernel(
    int64_t N, int32_t H, const int32_t* __restrict__ key, const T* __restrict__ enc, int32_t rows, int32_t K,
    const T* __restrict__ G, float* __restrict__ part) {
    __shared__ float s_g[kWgradChunk * kWgradMaxH];
    __shared__ float s_e[kWgradChunk * kWgradMaxK];
    const int64_t r0 = (int64_t)blockIdx.x * kWgradChunk;
    const int n = (int)min((int64_t)kWgradChunk, N - r0);
    for (int i = threadIdx.x; i < n * H; i += kBlock) s_g[i] = ld(G, r0 * H + i);
    for (int i = threadIdx.x; i < n * K; i += kBlock) {
        const int r = i / K;
        const int kk = key[r0 + r];
        s_e[i] = (kk >= 0 && kk < rows) ? ld(enc, (int64_t)kk * K + (i - r * K)) : 0.f;
    }
    __syncthreads();
    const int KH = K * H;
    for (int e = threadIdx.x; e < KH; e += kBlock) {
        const int k = e / H, h = e - k * H;
        float acc = 0.f;
        for (int i = 0; i < n; ++i) acc = fmaf(s_e[i * K + k], s_g[i * H + h], acc);
        part[(int64_t)blockIdx.x * KH + e] = acc;
    }
}

// dW[e] = sum over the chunks of part[c, e]: 16 slices of a workgroup take every 16th chunk (in order), then slice 0 adds the
// 16 slice sums in order -- the same fixed order on every run.
constexpr int kRedCols = 16;
constexpr int kRedSlices = kBlock / kRedCols;

template <typename T>
__global__ __launch_bounds__(kBlock) void embed_wgrad_reduce_kernel(int64_t nchunks, int32_t KH, const float* __restrict__ part,
                                                                    T* __restrict__ dW) {
    __shared__ float s_part[kRedSlices][kRedCols];
    const int col = threadIdx.x % kRedCols, slice = threadIdx.x / kRedCols;
    const int e = blockIdx.x * kRedCols + col;
    float acc = 0.f;
    if (e < KH) {
#pragma unroll 4
        for (int64_t c = slice; c < nchunks; c += kRedSlices) acc += part[c * KH + e];
    }
    s_part[slice][col] = acc;
    __syncthreads();
    if (slice == 0 && e < KH) {
        float t = 0.f;
        for (int j = 0; j < kRedSlices; ++j) t += s_part[j][col];
        dW[e] = st<T>(t);
    }
}

// pooled[b, :] = sum over the non-dummy rows v of graph b of [enc_v(id) | enc_vl(label) | out_deg | in_deg | rep].  A workgroup
// owns graph b; when a row is narrower than the workgroup, P = 256 / D slices of threads take every P-th row (in order) and slice 0
// adds the P slice sums in order.
template <typename T>
__global__ __launch_bounds__(kBlock) void pool_sum_kernel(
    const int32_t* __restrict__ node_ptr, const uint8_t* __restrict__ dummy, const int32_t* __restrict__ id, const T* __restrict__ enc_v,
    int32_t rows_v, int32_t Kv, const int32_t* __restrict__ label, const T* __restrict__ enc_vl, int32_t rows_vl, int32_t Kvl,
    const int32_t* __restrict__ out_deg, const int32_t* __restrict__ in_deg, const T* __restrict__ rep, int32_t H, int32_t D,
    float* __restrict__ pooled, int32_t* __restrict__ count) {
    __shared__ float s_acc[kBlock];
    const int64_t b = blockIdx.x;
    const int r0 = node_ptr[b], r1 = node_ptr[b + 1];
    const int c_vl = id ? Kv : 0;
    const int c_deg = c_vl + (label ? Kvl : 0);
    const int c_rep = c_deg + (out_deg ? 2 : 0);
    const int P = D >= kBlock ? 1 : kBlock / D;
    const int cols = kBlock / P;
    const int slice = threadIdx.x / cols, cl = threadIdx.x - slice * cols;
    for (int c0 = 0; c0 < D; c0 += cols) {
        const int c = c0 + cl;
        float acc = 0.f;
        if (slice < P && c < D) {
            for (int v = r0 + slice; v < r1; v += P) {
                if (dummy != nullptr && dummy[v]) continue;
                float x;
                if (c >= c_rep) {
                    x = ld(rep, (int64_t)v * H + (c - c_rep));
                } else if (c >= c_deg) {
                    x = (float)(c == c_deg ? out_deg[v] : in_deg[v]);
                } else if (c >= c_vl) {
                    const int l = label[v];
                    x = (l >= 0 && l < rows_vl) ? ld(enc_vl, (int64_t)l * Kvl + (c - c_vl)) : 0.f;
                } else {
                    const int i = id[v];
                    x = (i >= 0 && i < rows_v) ? ld(enc_v, (int64_t)i * Kv + c) : 0.f;
                }
                acc += x;
            }
        }
        s_acc[threadIdx.x] = acc;
        __syncthreads();
        if (slice == 0 && c < D) {
            float t = 0.f;
            for (int j = 0; j < P; ++j) t += s_acc[j * cols + cl];
            pooled[b * D + c] = t;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int n = 0;
        for (int v = r0; v < r1; ++v) n += (dummy != nullptr && dummy[v]) ? 0 : 1;
        count[b] = n;
    }
}

// drep[v, h] = dpooled[graph(v), col0 + h], 0 at dummy rows
template <typename T>
__global__ __launch_bounds__(kBlock) void pool_sum_bwd_kernel(const int32_t* __restrict__ node_ptr, const uint8_t* __restrict__ dummy,
                                                              const float* __restrict__ dpooled, int32_t D, int32_t col0, int32_t H,
                                                              T* __restrict__ drep) {
    const int64_t b = blockIdx.x;
    const int r0 = node_ptr[b], r1 = node_ptr[b + 1];
    const int64_t n = (int64_t)(r1 - r0) * H;
    for (int64_t i = threadIdx.x; i < n; i += kBlock) {
        const int64_t v = r0 + i / H;
        const int h = (int)(i % H);
        drep[v * H + h] = st<T>((dummy != nullptr && dummy[v]) ? 0.f : dpooled[b * D + col0 + h]);
    }
}

// out[b, c] = max(Y[v, c] over the non-dummy rows of graph b, bias[c] when graph b has fewer of them than L); argmax = the row,
// or -1 where the bias won.  First maximum in row order wins (strict >).
template <typename T>
__global__ __launch_bounds__(kBlock) void pool_max_kernel(const int32_t* __restrict__ node_ptr, const uint8_t* __restrict__ dummy,
                                                          const T* __restrict__ Y, int32_t C, const T* __restrict__ bias, int32_t L,
                                                          T* __restrict__ out, int32_t* __restrict__ argmax) {
    const int64_t b = blockIdx.x;
    const int r0 = node_ptr[b], r1 = node_ptr[b + 1];
    for (int c = threadIdx.x; c < C; c += kBlock) {
        float best = -INFINITY;
        int arg = -1, n = 0;
        for (int v = r0; v < r1; ++v) {
            if (dummy != nullptr && dummy[v]) continue;
            ++n;
            const float y = ld(Y, (int64_t)v * C + c);
            if (arg < 0 || y > best) { best = y; arg = v; }
        }
        if (n < L) {
            const float bb = ld(bias, c);
            if (arg < 0 || bb > best) { best = bb; arg = -1; }
        }
        out[b * C + c] = st<T>(best);
        argmax[b * C + c] = arg;
    }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void pool_max_bwd_kernel(int64_t total, int32_t C, const int32_t* __restrict__ argmax,
                                                              const T* __restrict__ dout, T* __restrict__ dY) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const int a = argmax[i];
    if (a >= 0) dY[(int64_t)a * C + (i % C)] = dout[i];                     // the rows of graph b are only b's argmaxes
}

__global__ __launch_bounds__(kBlock) void len_mask_kernel(int64_t B, int32_t L, const int32_t* __restrict__ node_ptr,
                                                          const uint8_t* __restrict__ dummy, uint8_t* __restrict__ mask) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= B * L) return;
    const int64_t b = i / L;
    const int pos = (int)(i - b * L);
    const int r0 = node_ptr[b], len = node_ptr[b + 1] - r0;
    const int start = L - len;                                              // pre-padded (utils/dl.py:113-127)
    uint8_t m = 0;
    if (pos >= start && len > 0) m = (dummy != nullptr && dummy[r0 + pos - start]) ? 0 : 1;
    mask[i] = m;
}

unsigned grid_for(int64_t n) {
    const int64_t g = dn_cdiv(n, kBlock);
    return (unsigned)(g < 1 ? 1 : (g > 65535 * 16 ? 65535 * 16 : g));
}

template <typename T>
int filter_meta(int64_t B, const int32_t* p_ptr, const int32_t* p_label, const int32_t* p_id, int64_t Np, const int32_t* g_ptr,
                const int32_t* g_label, const int32_t* g_id, int64_t Ng, int32_t p_nlab, int32_t p_nid, int32_t g_nlab, int32_t g_nid,
                void* gate, int32_t* meta, dn_stream_t stream) {
    DN_REQUIRE(B >= 1 && B < 0x7fffffffLL, "dn_si_filter_meta: 1 <= B < 2^31");
    DN_REQUIRE(Np >= 0 && Ng >= 0 && Np < 0x7fffffffLL && Ng < 0x7fffffffLL, "dn_si_filter_meta: node counts must fit int32");
    DN_REQUIRE(p_ptr && g_ptr && meta, "dn_si_filter_meta: NULL pointer");
    DN_REQUIRE((Np == 0 || (p_label && p_id)) && (Ng == 0 || (g_label && g_id)), "dn_si_filter_meta: NULL label / id");
    DN_REQUIRE(p_nlab >= 1 && p_nid >= 1 && g_nlab >= 1 && g_nid >= 1, "dn_si_filter_meta: table sizes must be >= 1");
    hipStream_t st = (hipStream_t)stream;
    DN_CHECK_HIP(hipMemsetAsync(meta, 0, 4 * sizeof(int32_t), st));
    hipLaunchKernelGGL(filter_meta_kernel<T>, dim3((unsigned)B), dim3(kBlock), 0, st, B, p_ptr, p_label, p_id, Np, g_ptr, g_label, g_id,
                       Ng, p_nlab, p_nid, g_nlab, g_nid, (T*)gate, meta);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

template <typename T>
int embed_fwd(int64_t N, int32_t H, const int32_t* key1, const void* enc1, int32_t rows1, int32_t K1, const void* W1,
              const int32_t* key2, const void* enc2, int32_t rows2, int32_t K2, const void* W2, void* out, dn_stream_t stream) {
    DN_REQUIRE(N >= 0 && H >= 1 && K1 >= 1 && rows1 >= 1, "dn_si_embed_fwd: bad sizes");
    DN_REQUIRE(H <= kWgradMaxH && K1 <= kWgradMaxK && (key2 == nullptr || K2 <= kWgradMaxK),
               "dn_si_embed_fwd: H <= %d and K <= %d (the limits of its weight gradient)", kWgradMaxH, kWgradMaxK);
    DN_REQUIRE(key1 && enc1 && W1 && out, "dn_si_embed_fwd: NULL pointer");
    DN_REQUIRE(key2 == nullptr || (enc2 && W2 && K2 >= 1 && rows2 >= 1), "dn_si_embed_fwd: second table incomplete");
    const int64_t words = (int64_t)K1 * H + (key2 ? (int64_t)K2 * H : 0);
    DN_REQUIRE(words <= kEmbedMaxLds, "dn_si_embed_fwd: (K1 + K2) * H must be <= %d", kEmbedMaxLds);
    if (N == 0) return DN_OK;
    hipLaunchKernelGGL(embed_fwd_kernel<T>, dim3(grid_for(N * H) > 2048 ? 2048 : grid_for(N * H)), dim3(kBlock),
                       (size_t)words * sizeof(float), (hipStream_t)stream, N, H, key1, (const T*)enc1, rows1, K1, (const T*)W1, key2,
                       (const T*)enc2, rows2, K2, (const T*)W2, (T*)out);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

size_t wgrad_ws_bytes(int64_t N, int32_t K, int32_t H) {
    return (size_t)dn_cdiv(N < 1 ? 1 : N, kWgradChunk) * (size_t)K * (size_t)H * sizeof(float);
}

template <typename T>
int embed_wgrad(int64_t N, int32_t H, const int32_t* key, const void* enc, int32_t rows, int32_t K, const void* G, void* dW, void* ws,
                size_t ws_bytes, dn_stream_t stream) {
    DN_REQUIRE(N >= 0 && H >= 1 && K >= 1 && rows >= 1, "dn_si_embed_wgrad: bad sizes");
    DN_REQUIRE(H <= kWgradMaxH && K <= kWgradMaxK, "dn_si_embed_wgrad: H <= %d and K <= %d", kWgradMaxH, kWgradMaxK);
    DN_REQUIRE(dW && (N == 0 || (key && enc && G && ws)), "dn_si_embed_wgrad: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {
        DN_CHECK_HIP(hipMemsetAsync(dW, 0, (size_t)K * H * sizeof(T), st));
        return DN_OK;
    }
    DN_REQUIRE(ws_bytes >= wgrad_ws_bytes(N, K, H), "dn_si_embed_wgrad: workspace too small");
    const int64_t nchunks = dn_cdiv(N, kWgradChunk);
    DN_REQUIRE(nchunks < 0x7fffffffLL, "dn_si_embed_wgrad: too many rows");
    hipLaunchKernelGGL(embed_wgrad_part_kernel<T>, dim3((unsigned)nchunks), dim3(kBlock), 0, st, N, H, key, (const T*)enc, rows, K,
                       (const T*)G, (float*)ws);
    hipLaunchKernelGGL(embed_wgrad_reduce_kernel<T>, dim3((unsigned)dn_cdiv((int64_t)K * H, kRedCols)), dim3(kBlock), 0, st, nchunks,
                       K * H, (const float*)ws, (T*)dW);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

template <typename T>
int pool_sum(int64_t B, const int32_t* node_ptr, const uint8_t* dummy, const int32_t* id, const void* enc_v, int32_t rows_v, int32_t Kv,
             const int32_t* label, const void* enc_vl, int32_t rows_vl, int32_t Kvl, const int32_t* out_deg, const int32_t* in_deg,
             const void* rep, int32_t H, float* pooled, int32_t* count, dn_stream_t stream) {
    DN_REQUIRE(B >= 1 && B < 0x7fffffffLL && H >= 1, "dn_si_pool_sum: bad sizes");
    DN_REQUIRE(node_ptr && rep && pooled && count, "dn_si_pool_sum: NULL pointer");
    DN_REQUIRE(id == nullptr || (enc_v && Kv >= 1 && rows_v >= 1), "dn_si_pool_sum: enc_v incomplete");
    DN_REQUIRE(label == nullptr || (enc_vl && Kvl >= 1 && rows_vl >= 1), "dn_si_pool_sum: enc_vl incomplete");
    DN_REQUIRE((out_deg == nullptr) == (in_deg == nullptr), "dn_si_pool_sum: give both degrees or neither");
    const int D = (id ? Kv : 0) + (label ? Kvl : 0) + (out_deg ? 2 : 0) + H;
    hipLaunchKernelGGL(pool_sum_kernel<T>, dim3((unsigned)B), dim3(kBlock), 0, (hipStream_t)stream, node_ptr, dummy, id, (const T*)enc_v,
                       rows_v, Kv, label, (const T*)enc_vl, rows_vl, Kvl, out_deg, in_deg, (const T*)rep, H, D, pooled, count);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

template <typename T>
int pool_sum_bwd(int64_t B, const int32_t* node_ptr, const uint8_t* dummy, const float* dpooled, int32_t D, int32_t col0, int32_t H,
                 void* drep, dn_stream_t stream) {
    DN_REQUIRE(B >= 1 && B < 0x7fffffffLL && H >= 1 && col0 >= 0 && col0 + H <= D, "dn_si_pool_sum_bwd: bad sizes");
    DN_REQUIRE(node_ptr && dpooled && drep, "dn_si_pool_sum_bwd: NULL pointer");
    hipLaunchKernelGGL(pool_sum_bwd_kernel<T>, dim3((unsigned)B), dim3(kBlock), 0, (hipStream_t)stream, node_ptr, dummy, dpooled, D, col0,
                       H, (T*)drep);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

template <typename T>
int pool_max(int64_t B, const int32_t* node_ptr, const uint8_t* dummy, const void* Y, int32_t C, const void* bias, int32_t L, void* out,
             int32_t* argmax, dn_stream_t stream) {
    DN_REQUIRE(B >= 1 && B < 0x7fffffffLL && C >= 1 && L >= 1, "dn_si_pool_max: bad sizes");
    DN_REQUIRE(node_ptr && Y && bias && out && argmax, "dn_si_pool_max: NULL pointer");
    hipLaunchKernelGGL(pool_max_kernel<T>, dim3((unsigned)B), dim3(kBlock), 0, (hipStream_t)stream, node_ptr, dummy, (const T*)Y, C,
                       (const T*)bias, L, (T*)out, argmax);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

template <typename T>
int pool_max_bwd(int64_t B, int32_t C, const int32_t* argmax, const void* dout, void* dY, dn_stream_t stream) {
    DN_REQUIRE(B >= 1 && C >= 1 && B * C < 0x7fffffffLL, "dn_si_pool_max_bwd: bad sizes");
    DN_REQUIRE(argmax && dout && dY, "dn_si_pool_max_bwd: NULL pointer");
    hipLaunchKernelGGL(pool_max_bwd_kernel<T>, dim3((unsigned)dn_cdiv(B * C, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, B * C, C,
                       argmax, (const T*)dout, (T*)dY);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

}  // namespace

extern "C" {

int dn_si_filter_meta_f32(int64_t B, const int32_t* p_ptr, const int32_t* p_label, const int32_t* p_id, int64_t Np, const int32_t* g_ptr,
                          const int32_t* g_label, const int32_t* g_id, int64_t Ng, int32_t p_nlab, int32_t p_nid, int32_t g_nlab,
                          int32_t g_nid, float* gate, int32_t* meta, dn_stream_t stream) {
    return filter_meta<float>(B, p_ptr, p_label, p_id, Np, g_ptr, g_label, g_id, Ng, p_nlab, p_nid, g_nlab, g_nid, gate, meta, stream);
}
int dn_si_filter_meta_bf16(int64_t B, const int32_t* p_ptr, const int32_t* p_label, const int32_t* p_id, int64_t Np, const int32_t* g_ptr,
                           const int32_t* g_label, const int32_t* g_id, int64_t Ng, int32_t p_nlab, int32_t p_nid, int32_t g_nlab,
                           int32_t g_nid, void* gate, int32_t* meta, dn_stream_t stream) {
    return filter_meta<bf16_t>(B, p_ptr, p_label, p_id, Np, g_ptr, g_label, g_id, Ng, p_nlab, p_nid, g_nlab, g_nid, gate, meta, stream);
}

int dn_si_embed_fwd_f32(int64_t N, int32_t H, const int32_t* key1, const float* enc1, int32_t rows1, int32_t K1, const float* W1,
                        const int32_t* key2, const float* enc2, int32_t rows2, int32_t K2, const float* W2, float* out, dn_stream_t stream) {
    return embed_fwd<float>(N, H, key1, enc1, rows1, K1, W1, key2, enc2, rows2, K2, W2, out, stream);
}
int dn_si_embed_fwd_bf16(int64_t N, int32_t H, const int32_t* key1, const void* enc1, int32_t rows1, int32_t K1, const void* W1,
                         const int32_t* key2, const void* enc2, int32_t rows2, int32_t K2, const void* W2, void* out, dn_stream_t stream) {
    return embed_fwd<bf16_t>(N, H, key1, enc1, rows1, K1, W1, key2, enc2, rows2, K2, W2, out, stream);
}

size_t dn_si_embed_wgrad_workspace_bytes(int64_t N, int32_t K, int32_t H) {
    if (N < 0 || K < 1 || H < 1) { dn_set_error("dn_si_embed_wgrad_workspace_bytes: bad sizes"); return 0; }
    return wgrad_ws_bytes(N, K, H);
}
int dn_si_embed_wgrad_f32(int64_t N, int32_t H, const int32_t* key, const float* enc, int32_t rows, int32_t K, const float* G, float* dW,
                          void* workspace, size_t workspace_bytes, dn_stream_t stream) {
    return embed_wgrad<float>(N, H, key, enc, rows, K, G, dW, workspace, workspace_bytes, stream);
}
int dn_si_embed_wgrad_bf16(int64_t N, int32_t H, const int32_t* key, const void* enc, int32_t rows, int32_t K, const void* G, void* dW,
                           void* workspace, size_t workspace_bytes, dn_stream_t stream) {
    return embed_wgrad<bf16_t>(N, H, key, enc, rows, K, G, dW, workspace, workspace_bytes, stream);
}

int dn_si_pool_sum_f32(int64_t B, const int32_t* node_ptr, const uint8_t* dummy, const int32_t* id, const float* enc_v, int32_t rows_v,
                       int32_t Kv, const int32_t* label, const float* enc_vl, int32_t rows_vl, int32_t Kvl, const int32_t* out_deg,
                       const int32_t* in_deg, const float* rep, int32_t H, float* pooled, int32_t* count, dn_stream_t stream) {
    return pool_sum<float>(B, node_ptr, dummy, id, enc_v, rows_v, Kv, label, enc_vl, rows_vl, Kvl, out_deg, in_deg, rep, H, pooled, count,
                           stream);
}
int dn_si_pool_sum_bf16(int64_t B, const int32_t* node_ptr, const uint8_t* dummy, const int32_t* id, const void* enc_v, int32_t rows_v,
                        int32_t Kv, const int32_t* label, const void* enc_vl, int32_t rows_vl, int32_t Kvl, const int32_t* out_deg,
                        const int32_t* in_deg, const void* rep, int32_t H, float* pooled, int32_t* count, dn_stream_t stream) {
    return pool_sum<bf16_t>(B, node_ptr, dummy, id, enc_v, rows_v, Kv, label, enc_vl, rows_vl, Kvl, out_deg, in_deg, rep, H, pooled, count,
                            stream);
}
int dn_si_pool_sum_bwd_f32(int64_t B, const int32_t* node_ptr, const uint8_t* dummy, const float* dpooled, int32_t D, int32_t col0,
                           int32_t H, float* drep, dn_stream_t stream) {
    return pool_sum_bwd<float>(B, node_ptr, dummy, dpooled, D, col0, H, drep, stream);
}
int dn_si_pool_sum_bwd_bf16(int64_t B, const int32_t* node_ptr, const uint8_t* dummy, const float* dpooled, int32_t D, int32_t col0,
                            int32_t H, void* drep, dn_stream_t stream) {
    return pool_sum_bwd<bf16_t>(B, node_ptr, dummy, dpooled, D, col0, H, drep, stream);
}

int dn_si_pool_max_f32(int64_t B, const int32_t* node_ptr, const uint8_t* dummy, const float* Y, int32_t C, const float* bias, int32_t L,
                       float* out, int32_t* argmax, dn_stream_t stream) {
    return pool_max<float>(B, node_ptr, dummy, Y, C, bias, L, out, argmax, stream);
}
int dn_si_pool_max_bf16(int64_t B, const int32_t* node_ptr, const uint8_t* dummy, const void* Y, int32_t C, const void* bias, int32_t L,
                        void* out, int32_t* argmax, dn_stream_t stream) {
    return pool_max<bf16_t>(B, node_ptr, dummy, Y, C, bias, L, out, argmax, stream);
}
int dn_si_pool_max_bwd_f32(int64_t B, int32_t C, const int32_t* argmax, const float* dout, float* dY, dn_stream_t stream) {
    return pool_max_bwd<float>(B, C, argmax, dout, dY, stream);
}
int dn_si_pool_max_bwd_bf16(int64_t B, int32_t C, const int32_t* argmax, const void* dout, void* dY, dn_stream_t stream) {
    return pool_max_bwd<bf16_t>(B, C, argmax, dout, dY, stream);
}

int dn_si_len_mask_u8(int64_t B, int32_t L, const int32_t* node_ptr, const uint8_t* dummy, uint8_t* mask, dn_stream_t stream) {
    DN_REQUIRE(B >= 1 && L >= 1 && B * L < 0x7fffffffLL, "dn_si_len_mask: bad sizes");
    DN_REQUIRE(node_ptr && mask, "dn_si_len_mask: NULL pointer");
    hipLaunchKernelGGL(len_mask_kernel, dim3((unsigned)dn_cdiv(B * L, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, B, L, node_ptr, dummy,
                       mask);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

}  // extern "C"
