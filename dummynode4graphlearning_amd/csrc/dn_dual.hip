// Dual (node + edge) message passing of the SI models CompGCN / DMPNN (subgraph_isomorphism/models/compgcn.py:104-283,
// dmpnn.py:16-187) and the ragged edge head of GraphAdjModelV2 (basemodel.py:1622-1667).
//
// Dual aggregation: ONE pass over a grouped edge list (the CSR by destination, or the CSC by source) sums the rows of the
// forward edges and of the reversed edges into two outputs,
//     out[d][v] = sum over e in list(v) with rev_e == d of scale_e * m_e,     m_e = ef_e | x[src_e] - ef_e | x[src_e] * ef_e
// so neither the composed [E, H] rows nor per-direction [E] float masks are ever written.  The list is walked through a unit
// table {segment, first entry, end entry, partial slot}: a segment of at most HUB_SPLIT entries is one unit and writes its two
// sums; a longer one (the dummy node of a large graph) is cut into units that write fp32 partials, folded afterwards in unit
// order.  Every sum runs in list order in fp32: no float atomics, bit-identical from run to run.
#include "dn_common.h"
#include "../../include/dn_hip.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxH = 256;
constexpr int kMaxGrid = 4096;

enum { kModeEdge = DN_DUAL_EDGE, kModeSub = DN_DUAL_SUB, kModeMult = DN_DUAL_MULT };

// scale_e * m_e of edge e at column col (0 for an edge id or a source outside the tables: never read out of bounds)
template <typename T, int MODE>
__device__ __forceinline__ float message(int32_t e, int col, int64_t N, int64_t E, int32_t H, const int32_t* __restrict__ src,
                                         const float* __restrict__ scale, const T* __restrict__ ef, const T* __restrict__ x) {
    if ((uint32_t)e >= (uint64_t)E) return 0.f;
    float m = ld(ef, (int64_t)e * H + col);
    if (MODE != kModeEdge) {
        const int32_t s = src[e];
        const float xs = (uint32_t)s < (uint64_t)N ? ld(x, (int64_t)s * H + col) : 0.f;
        m = MODE == kModeSub ? xs - m : xs * m;
    }
    return scale != nullptr ? scale[e] * m : m;
}

// a group of gsz lanes (gsz = the power of two >= H) owns a unit; lane = column
template <typename T, int MODE>
__global__ __launch_bounds__(kBlock) void dual_agg_kernel(
    int64_t N, int64_t E, int32_t H, int32_t gsz, int64_t U, const int4* __restrict__ units, const int32_t* __restrict__ perm,
    const int32_t* __restrict__ src, const uint8_t* __restrict__ rev, const float* __restrict__ scale, const T* __restrict__ ef,
    const T* __restrict__ x, void* __restrict__ out, int32_t out_f32, float* __restrict__ part, int64_t P) {
    const int upb = kBlock / gsz;
    const int64_t u = (int64_t)blockIdx.x * upb + threadIdx.x / gsz;
    const int col = threadIdx.x & (gsz - 1);
    if (u >= U || col >= H) return;
    const int4 un = units[u];
    if ((uint32_t)un.x >= (uint64_t)N || un.w >= P) return;            // (a broken table writes nothing out of bounds)
    const int end = un.z < E ? un.z : (int)E;
    float a0 = 0.f, a1 = 0.f;
    int i = un.y < 0 ? 0 : un.y;
    for (; i + 4 <= end; i += 4) {                       // four rows in flight; added in list order
        int32_t e[4];
        float m[4];
        bool r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = perm[i + k];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            m[k] = message<T, MODE>(e[k], col, N, E, H, src, scale, ef, x);
            r[k] = rev != nullptr && (uint32_t)e[k] < (uint64_t)E && rev[e[k]] != 0;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (r[k]) a1 += m[k];
            else a0 += m[k];
        }
    }
    for (; i < end; ++i) {
        const int32_t e = perm[i];
        const float m = message<T, MODE>(e, col, N, E, H, src, scale, ef, x);
        if (rev != nullptr && (uint32_t)e < (uint64_t)E && rev[e] != 0) a1 += m;
        else a0 += m;
    }
    if (un.w < 0) {
        const int64_t i0 = (int64_t)un.x * H + col, i1 = (N + un.x) * H + col;
        if (out_f32) {                                    // fp32 sums for a caller that adds two passes before it rounds
            ((float*)out)[i0] = a0;
            ((float*)out)[i1] = a1;
        } else {
            ((T*)out)[i0] = st<T>(a0);
            ((T*)out)[i1] = st<T>(a1);
        }
    } else {
        part[((int64_t)un.w * 2) * H + col] = a0;
        part[((int64_t)un.w * 2 + 1) * H + col] = a1;
    }
}

// G_e = scale_e * g[rev_e][dst_e] at column col
template <typename T>
__device__ __forceinline__ float upstream(int32_t e, int col, int64_t N, int32_t H, const int32_t* __restrict__ dst,
                                          const uint8_t* __restrict__ rev, const float* __restrict__ scale, const T* __restrict__ g) {
    const int32_t d = dst[e];
    if ((uint32_t)d >= (uint64_t)N) return 0.f;
    const int64_t row = (rev != nullptr && rev[e] != 0) ? N + d : (int64_t)d;
    const float v = ld(g, row * H + col);
    return scale != nullptr ? scale[e] * v : v;
}

// d ef[e] = G_e | -G_e | G_e * x[src_e]
template <typename T, int MODE>
__global__ __launch_bounds__(kBlock) void dual_agg_bwd_edge_kernel(
    int64_t N, int64_t E, int32_t H, const int32_t* __restrict__ src, const int32_t* __restrict__ dst, const uint8_t* __restrict__ rev,
    const float* __restrict__ scale, const T* __restrict__ g, const T* __restrict__ x, T* __restrict__ d_ef) {
    const int64_t total = E * H;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int32_t e = (int32_t)(i / H);
        const int col = (int)(i - (int64_t)e * H);
        float G = upstream<T>(e, col, N, H, dst, rev, scale, g);
        if (MODE == kModeSub) G = -G;
        if (MODE == kModeMult) {
            const int32_t s = src[e];
            G = (uint32_t)s < (uint64_t)N ? G * ld(x, (int64_t)s * H + col) : 0.f;
        }
        d_ef[i] = st<T>(G);
    }
}

// d x[u] = sum over the out-list of u of G_e (sub) | G_e * ef_e (mult); units over the CSC by source
template <typename T, int MODE>
__global__ __launch_bounds__(kBlock) void dual_agg_bwd_node_kernel(
    int64_t N, int64_t E, int32_t H, int32_t gsz, int64_t U, const int4* __restrict__ units, const int32_t* __restrict__ perm,
    const int32_t* __restrict__ dst, const uint8_t* __restrict__ rev, const float* __restrict__ scale, const T* __restrict__ g,
    const T* __restrict__ ef, T* __restrict__ dx, float* __restrict__ part, int64_t P) {
    const int upb = kBlock / gsz;
    const int64_t u = (int64_t)blockIdx.x * upb + threadIdx.x / gsz;
    const int col = threadIdx.x & (gsz - 1);
    if (u >= U || col >= H) return;
    const int4 un = units[u];
    if ((uint32_t)un.x >= (uint64_t)N || un.w >= P) return;
    const int end = un.z < E ? un.z : (int)E;
    float acc = 0.f;
    int i = un.y < 0 ? 0 : un.y;
    for (; i + 4 <= end; i += 4) {
        int32_t e[4];
        float m[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = perm[i + k];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            m[k] = 0.f;
            if ((uint32_t)e[k] < (uint64_t)E) {
                m[k] = upstream<T>(e[k], col, N, H, dst, rev, scale, g);
                if (MODE == kModeMult) m[k] *= ld(ef, (int64_t)e[k] * H + col);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) acc += m[k];
    }
    for (; i < end; ++i) {
        const int32_t e = perm[i];
        if ((uint32_t)e >= (uint64_t)E) continue;
        float m = upstream<T>(e, col, N, H, dst, rev, scale, g);
        if (MODE == kModeMult) m *= ld(ef, (int64_t)e * H + col);
        acc += m;
    }
    if (un.w < 0) dx[(int64_t)un.x * H + col] = st<T>(acc);
    else part[(int64_t)un.w * H + col] = acc;
}

// DMP edge update: out[e] = (p_loop[e] + coef[dst_e] p_diff[e]) + (xd[a_e] - xs[b_e]) + ebias,
// (a, b) = (dst, src) on forward edges, (src, dst) on reversed ones
template <typename T>
__global__ __launch_bounds__(kBlock) void edge_update_kernel(
    int64_t N, int64_t E, int32_t H, const int32_t* __restrict__ src, const int32_t* __restrict__ dst, const uint8_t* __restrict__ rev,
    const float* __restrict__ coef, const T* __restrict__ p_loop, const T* __restrict__ p_diff, const T* __restrict__ xd,
    const T* __restrict__ xs, const T* __restrict__ ebias, T* __restrict__ out) {
    const int64_t total = E * H;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int32_t e = (int32_t)(i / H);
        const int col = (int)(i - (int64_t)e * H);
        const int32_t s = src[e], d = dst[e];
        float v = 0.f;
        if ((uint32_t)s < (uint64_t)N && (uint32_t)d < (uint64_t)N) {
            const bool r = rev != nullptr && rev[e] != 0;
            const int32_t a = r ? s : d, b = r ? d : s;
            v = (ld(p_loop, i) + coef[d] * ld(p_diff, i)) + (ld(xd, (int64_t)a * H + col) - ld(xs, (int64_t)b * H + col));
        }
        if (ebias != nullptr) v += ld(ebias, col);
        out[i] = st<T>(v);
    }
}

// d p_diff[e] = coef[dst_e] * g[e]   (d p_loop = g itself; the row sums into xd / xs are two dual aggregations of g)
template <typename T>
__global__ __launch_bounds__(kBlock) void edge_update_bwd_kernel(int64_t N, int64_t E, int32_t H, const int32_t* __restrict__ dst,
                                                                 const float* __restrict__ coef, const T* __restrict__ g,
                                                                 T* __restrict__ d_diff) {
    const int64_t total = E * H;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int32_t d = dst[i / H];
        d_diff[i] = st<T>((uint32_t)d < (uint64_t)N ? coef[d] * ld(g, i) : 0.f);
    }
}

// pooled[b, :] = sum over the kept edges e = (u, v) of graph b of
// [enc_v(id[u]) | enc_v(id[v]) | enc_vl(vl[u]) | enc_el(el[e]) | enc_vl(vl[v]) | out_deg[u] | in_deg[v] | rep[e]].
// Thread layout as dn_si_pool_sum: a workgroup per graph, P = 256 / D slices take every P-th edge and are added in slice order.
template <typename T>
__global__ __launch_bounds__(kBlock) void edge_pool_sum_kernel(
    const int32_t* __restrict__ edge_ptr, const uint8_t* __restrict__ skip, const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
    int64_t N, const int32_t* __restrict__ id, const T* __restrict__ enc_v, int32_t rows_v, int32_t Kv, const int32_t* __restrict__ vlabel,
    const T* __restrict__ enc_vl, int32_t rows_vl, int32_t Kvl, const int32_t* __restrict__ elabel, const T* __restrict__ enc_el,
    int32_t rows_el, int32_t Kel, const int32_t* __restrict__ out_deg, const int32_t* __restrict__ in_deg, const T* __restrict__ rep,
    int32_t H, int32_t D, float* __restrict__ pooled, int32_t* __restrict__ count) {
    __shared__ float s_acc[kBlock];
    const int64_t b = blockIdx.x;
    const int r0 = edge_ptr[b], r1 = edge_ptr[b + 1];
    const bool has_enc = id != nullptr;
    const int c1 = has_enc ? Kv : 0;                    // enc_v(id[v])
    const int c2 = has_enc ? 2 * Kv : 0;                // enc_vl(vl[u])
    const int c3 = c2 + (has_enc ? Kvl : 0);            // enc_el(el[e])
    const int c4 = c3 + (has_enc ? Kel : 0);            // enc_vl(vl[v])
    const int c_deg = c4 + (has_enc ? Kvl : 0);
    const int c_rep = c_deg + (out_deg ? 2 : 0);
    const int P = D >= kBlock ? 1 : kBlock / D;
    const int cols = kBlock / P;
    const int slice = threadIdx.x / cols, cl = threadIdx.x - slice * cols;
    for (int c0 = 0; c0 < D; c0 += cols) {
        const int c = c0 + cl;
        float acc = 0.f;
        if (slice < P && c < D) {
            for (int e = r0 + slice; e < r1; e += P) {
                if (skip != nullptr && skip[e]) continue;
                float v = 0.f;
                if (c >= c_rep) {
                    v = ld(rep, (int64_t)e * H + (c - c_rep));
                } else {
                    const bool from_src = c < c1 || (c >= c2 && c < c3) || c == c_deg;
                    const int32_t n = from_src ? src[e] : dst[e];
                    if (c >= c3 && c < c4) {
                        const int l = elabel[e];
                        if (l >= 0 && l < rows_el) v = ld(enc_el, (int64_t)l * Kel + (c - c3));
                    } else if ((uint32_t)n < (uint64_t)N) {
                        if (c >= c_deg) {
                            v = (float)(c == c_deg ? out_deg[n] : in_deg[n]);
                        } else if (c < c2) {
                            const int k = id[n];
                            if (k >= 0 && k < rows_v) v = ld(enc_v, (int64_t)k * Kv + (c < c1 ? c : c - c1));
                        } else {
                            const int l = vlabel[n];
                            if (l >= 0 && l < rows_vl) v = ld(enc_vl, (int64_t)l * Kvl + (c < c3 ? c - c2 : c - c4));
                        }
                    }
                }
                acc += v;
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
    // the kept edges of the graph: a strided share per thread, wave sums, four partials (integers: any order)
    __shared__ int s_cnt[kBlock / 64];
    int n = 0;
    for (int e = r0 + (int)threadIdx.x; e < r1; e += kBlock) n += (skip != nullptr && skip[e]) ? 0 : 1;
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) count[b] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

int group_size(int32_t H) {
    int g = 16;
    while (g < H) g <<= 1;
    return g;
}

unsigned stride_grid(int64_t total) {
    const int64_t b = dn_cdiv(total, kBlock);
    return (unsigned)(b > kMaxGrid ? kMaxGrid : b);
}

int check_units(const char* what, int64_t N, int64_t E, int32_t H, int64_t U, const void* units, const void* perm, const void* part,
                int64_t P) {
    DN_REQUIRE(N >= 0 && E >= 0 && N < 0x3fffffffLL && E < 0x7fffffffLL, "%s: N < 2^30 and E < 2^31", what);
    DN_REQUIRE(H >= 1 && H <= kMaxH, "%s: 1 <= H <= %d", what, kMaxH);
    DN_REQUIRE(U >= 0 && U < 0x7fffffffLL && P >= 0 && P <= U, "%s: bad unit counts", what);
    DN_REQUIRE(U == 0 || units, "%s: NULL unit table", what);
    DN_REQUIRE(E == 0 || perm, "%s: NULL pointer", what);
    DN_REQUIRE(P == 0 || part, "%s: partial slots without a partial buffer", what);
    return DN_OK;
}

template <typename T>
int dual_agg(int32_t mode, int64_t N, int64_t E, int32_t H, int64_t U, const int32_t* units, const int32_t* perm, const int32_t* src,
             const uint8_t* rev, const float* scale, const void* ef, const void* x, void* out, int32_t out_f32, float* part,
             int64_t P, dn_stream_t stream) {
    DN_REQUIRE(mode == kModeEdge || mode == kModeSub || mode == kModeMult, "dn_dual_agg: bad mode %d", mode);
    if (int rc = check_units("dn_dual_agg", N, E, H, U, units, perm, part, P)) return rc;
    DN_REQUIRE(N == 0 || out, "dn_dual_agg: NULL pointer");
    DN_REQUIRE(E == 0 || ef, "dn_dual_agg: NULL pointer");
    DN_REQUIRE(mode == kModeEdge || E == 0 || (src && x), "dn_dual_agg: sub / mult need src and x");
    if (U == 0) return DN_OK;
    const int gsz = group_size(H);
    const dim3 grid((unsigned)dn_cdiv(U, kBlock / gsz)), block(kBlock);
    hipStream_t st = (hipStream_t)stream;
#define DN_DUAL_LAUNCH(M)                                                                                                        \
    hipLaunchKernelGGL((dual_agg_kernel<T, M>), grid, block, 0, st, N, E, H, gsz, U, (const int4*)units, perm, src, rev, scale, \
                       (const T*)ef, (const T*)x, out, out_f32, part, P)
    if (mode == kModeEdge) DN_DUAL_LAUNCH(kModeEdge);
    else if (mode == kModeSub) DN_DUAL_LAUNCH(kModeSub);
    else DN_DUAL_LAUNCH(kModeMult);
#undef DN_DUAL_LAUNCH
    DN_CHECK_LAUNCH();
    return DN_OK;
}

template <typename T>
int dual_agg_bwd_edge(int32_t mode, int64_t N, int64_t E, int32_t H, const int32_t* src, const int32_t* dst, const uint8_t* rev,
                      const float* scale, const void* g, const void* x, void* d_ef, dn_stream_t stream) {
    DN_REQUIRE(mode == kModeEdge || mode == kModeSub || mode == kModeMult, "dn_dual_agg_bwd_edge: bad mode %d", mode);
    DN_REQUIRE(N >= 0 && E >= 0 && N < 0x3fffffffLL && E < 0x7fffffffLL, "dn_dual_agg_bwd_edge: N < 2^30 and E < 2^31");
    DN_REQUIRE(H >= 1 && H <= kMaxH, "dn_dual_agg_bwd_edge: 1 <= H <= %d", kMaxH);
    if (E == 0) return DN_OK;
    DN_REQUIRE(dst && g && d_ef, "dn_dual_agg_bwd_edge: NULL pointer");
    DN_REQUIRE(mode != kModeMult || (src && x), "dn_dual_agg_bwd_edge: mult needs src and x");
    const dim3 grid(stride_grid(E * H)), block(kBlock);
    hipStream_t st = (hipStream_t)stream;
#define DN_DUAL_LAUNCH(M)                                                                                                   \
    hipLaunchKernelGGL((dual_agg_bwd_edge_kernel<T, M>), grid, block, 0, st, N, E, H, src, dst, rev, scale, (const T*)g, \
                       (const T*)x, (T*)d_ef)
    if (mode == kModeEdge) DN_DUAL_LAUNCH(kModeEdge);
    else if (mode == kModeSub) DN_DUAL_LAUNCH(kModeSub);
    else DN_DUAL_LAUNCH(kModeMult);
#undef DN_DUAL_LAUNCH
    DN_CHECK_LAUNCH();
    return DN_OK;
}

template <typename T>
int dual_agg_bwd_node(int32_t mode, int64_t N, int64_t E, int32_t H, int64_t U, const int32_t* units, const int32_t* perm,
                      const int32_t* dst, const uint8_t* rev, const float* scale, const void* g, const void* ef, void* dx, float* part,
                      int64_t P, dn_stream_t stream) {
    DN_REQUIRE(mode == kModeSub || mode == kModeMult, "dn_dual_agg_bwd_node: bad mode %d (sub or mult)", mode);
    if (int rc = check_units("dn_dual_agg_bwd_node", N, E, H, U, units, perm, part, P)) return rc;
    DN_REQUIRE(N == 0 || dx, "dn_dual_agg_bwd_node: NULL pointer");
    DN_REQUIRE(E == 0 || (dst && g), "dn_dual_agg_bwd_node: NULL pointer");
    DN_REQUIRE(mode != kModeMult || E == 0 || ef, "dn_dual_agg_bwd_node: mult needs ef");
    if (U == 0) return DN_OK;
    const int gsz = group_size(H);
    const dim3 grid((unsigned)dn_cdiv(U, kBlock / gsz)), block(kBlock);
    hipStream_t st = (hipStream_t)stream;
    if (mode == kModeSub)
        hipLaunchKernelGGL((dual_agg_bwd_node_kernel<T, kModeSub>), grid, block, 0, st, N, E, H, gsz, U, (const int4*)units, perm, dst, rev,
                           scale, (const T*)g, (const T*)ef, (T*)dx, part, P);
    else
        hipLaunchKernelGGL((dual_agg_bwd_node_kernel<T, kModeMult>), grid, block, 0, st, N, E, H, gsz, U, (const int4*)units, perm, dst, rev,
                           scale, (const T*)g, (const T*)ef, (T*)dx, part, P);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

template <typename T>
int edge_update(int64_t N, int64_t E, int32_t H, const int32_t* src, const int32_t* dst, const uint8_t* rev, const float* coef,
                const void* p_loop, const void* p_diff, const void* xd, const void* xs, const void* ebias, void* out,
                dn_stream_t stream) {
    DN_REQUIRE(N >= 0 && E >= 0 && N < 0x3fffffffLL && E < 0x7fffffffLL, "dn_dual_edge_update: N < 2^30 and E < 2^31");
    DN_REQUIRE(H >= 1 && H <= kMaxH, "dn_dual_edge_update: 1 <= H <= %d", kMaxH);
    if (E == 0) return DN_OK;
    DN_REQUIRE(src && dst && coef && p_loop && p_diff && xd && xs && out, "dn_dual_edge_update: NULL pointer");
    hipLaunchKernelGGL(edge_update_kernel<T>, dim3(stride_grid(E * H)), dim3(kBlock), 0, (hipStream_t)stream, N, E, H, src, dst, rev, coef,
                       (const T*)p_loop, (const T*)p_diff, (const T*)xd, (const T*)xs, (const T*)ebias, (T*)out);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

template <typename T>
int edge_update_bwd(int64_t N, int64_t E, int32_t H, const int32_t* dst, const float* coef, const void* g, void* d_diff,
                    dn_stream_t stream) {
    DN_REQUIRE(N >= 0 && E >= 0 && N < 0x3fffffffLL && E < 0x7fffffffLL, "dn_dual_edge_update_bwd: N < 2^30 and E < 2^31");
    DN_REQUIRE(H >= 1 && H <= kMaxH, "dn_dual_edge_update_bwd: 1 <= H <= %d", kMaxH);
    if (E == 0) return DN_OK;
    DN_REQUIRE(dst && coef && g && d_diff, "dn_dual_edge_update_bwd: NULL pointer");
    hipLaunchKernelGGL(edge_update_bwd_kernel<T>, dim3(stride_grid(E * H)), dim3(kBlock), 0, (hipStream_t)stream, N, E, H, dst, coef,
                       (const T*)g, (T*)d_diff);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

template <typename T>
int edge_pool_sum(int64_t B, const int32_t* edge_ptr, const uint8_t* skip, const int32_t* src, const int32_t* dst, int64_t N,
                  const int32_t* id, const void* enc_v, int32_t rows_v, int32_t Kv, const int32_t* vlabel, const void* enc_vl,
                  int32_t rows_vl, int32_t Kvl, const int32_t* elabel, const void* enc_el, int32_t rows_el, int32_t Kel,
                  const int32_t* out_deg, const int32_t* in_deg, const void* rep, int32_t H, float* pooled, int32_t* count,
                  dn_stream_t stream) {
    DN_REQUIRE(B >= 1 && B < 0x7fffffffLL && H >= 1 && N >= 0 && N < 0x7fffffffLL, "dn_sie_pool_sum: bad sizes");
    DN_REQUIRE(edge_ptr && rep && pooled && count, "dn_sie_pool_sum: NULL pointer");
    const bool any_enc = id || vlabel || elabel;
    DN_REQUIRE(!any_enc || (id && vlabel && elabel && enc_v && enc_vl && enc_el), "dn_sie_pool_sum: give all three encoders or none");
    DN_REQUIRE(!any_enc || (Kv >= 1 && Kvl >= 1 && Kel >= 1 && rows_v >= 1 && rows_vl >= 1 && rows_el >= 1),
               "dn_sie_pool_sum: encoder sizes must be >= 1");
    DN_REQUIRE((out_deg == nullptr) == (in_deg == nullptr), "dn_sie_pool_sum: give both degrees or neither");
    DN_REQUIRE(!(any_enc || out_deg) || (src && dst), "dn_sie_pool_sum: encoder / degree columns need src and dst");
    const int D = (any_enc ? 2 * Kv + 2 * Kvl + Kel : 0) + (out_deg ? 2 : 0) + H;
    hipLaunchKernelGGL(edge_pool_sum_kernel<T>, dim3((unsigned)B), dim3(kBlock), 0, (hipStream_t)stream, edge_ptr, skip, src, dst, N, id,
                       (const T*)enc_v, rows_v, Kv, vlabel, (const T*)enc_vl, rows_vl, Kvl, elabel, (const T*)enc_el, rows_el, Kel,
                       out_deg, in_deg, (const T*)rep, H, D, pooled, count);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

}  // namespace

extern "C" {

int dn_dual_agg_f32(int32_t mode, int64_t N, int64_t E, int32_t H, int64_t U, const int32_t* units, const int32_t* perm,
                    const int32_t* src, const uint8_t* rev, const float* scale, const float* ef, const float* x, float* out,
                    int32_t out_f32, float* part, int64_t P, dn_stream_t stream) {
    return dual_agg<float>(mode, N, E, H, U, units, perm, src, rev, scale, ef, x, out, out_f32, part, P, stream);
}
int dn_dual_agg_bf16(int32_t mode, int64_t N, int64_t E, int32_t H, int64_t U, const int32_t* units, const int32_t* perm,
                     const int32_t* src, const uint8_t* rev, const float* scale, const void* ef, const void* x, void* out,
                     int32_t out_f32, float* part, int64_t P, dn_stream_t stream) {
    return dual_agg<bf16_t>(mode, N, E, H, U, units, perm, src, rev, scale, ef, x, out, out_f32, part, P, stream);
}
int dn_dual_agg_bwd_edge_f32(int32_t mode, int64_t N, int64_t E, int32_t H, const int32_t* src, const int32_t* dst, const uint8_t* rev,
                             const float* scale, const float* g, const float* x, float* d_ef, dn_stream_t stream) {
    return dual_agg_bwd_edge<float>(mode, N, E, H, src, dst, rev, scale, g, x, d_ef, stream);
}
int dn_dual_agg_bwd_edge_bf16(int32_t mode, int64_t N, int64_t E, int32_t H, const int32_t* src, const int32_t* dst, const uint8_t* rev,
                              const float* scale, const void* g, const void* x, void* d_ef, dn_stream_t stream) {
    return dual_agg_bwd_edge<bf16_t>(mode, N, E, H, src, dst, rev, scale, g, x, d_ef, stream);
}
int dn_dual_agg_bwd_node_f32(int32_t mode, int64_t N, int64_t E, int32_t H, int64_t U, const int32_t* units, const int32_t* perm,
                             const int32_t* dst, const uint8_t* rev, const float* scale, const float* g, const float* ef, float* dx,
                             float* part, int64_t P, dn_stream_t stream) {
    return dual_agg_bwd_node<float>(mode, N, E, H, U, units, perm, dst, rev, scale, g, ef, dx, part, P, stream);
}
int dn_dual_agg_bwd_node_bf16(int32_t mode, int64_t N, int64_t E, int32_t H, int64_t U, const int32_t* units, const int32_t* perm,
                              const int32_t* dst, const uint8_t* rev, const float* scale, const void* g, const void* ef, void* dx,
                              float* part, int64_t P, dn_stream_t stream) {
    return dual_agg_bwd_node<bf16_t>(mode, N, E, H, U, units, perm, dst, rev, scale, g, ef, dx, part, P, stream);
}

int dn_dual_edge_update_f32(int64_t N, int64_t E, int32_t H, const int32_t* src, const int32_t* dst, const uint8_t* rev,
                            const float* coef, const float* p_loop, const float* p_diff, const float* xd, const float* xs,
                            const float* ebias, float* out, dn_stream_t stream) {
    return edge_update<float>(N, E, H, src, dst, rev, coef, p_loop, p_diff, xd, xs, ebias, out, stream);
}
int dn_dual_edge_update_bf16(int64_t N, int64_t E, int32_t H, const int32_t* src, const int32_t* dst, const uint8_t* rev,
                             const float* coef, const void* p_loop, const void* p_diff, const void* xd, const void* xs,
                             const void* ebias, void* out, dn_stream_t stream) {
    return edge_update<bf16_t>(N, E, H, src, dst, rev, coef, p_loop, p_diff, xd, xs, ebias, out, stream);
}
int dn_dual_edge_update_bwd_f32(int64_t N, int64_t E, int32_t H, const int32_t* dst, const float* coef, const float* g, float* d_diff,
                                dn_stream_t stream) {
    return edge_update_bwd<float>(N, E, H, dst, coef, g, d_diff, stream);
}
int dn_dual_edge_update_bwd_bf16(int64_t N, int64_t E, int32_t H, const int32_t* dst, const float* coef, const void* g, void* d_diff,
                                 dn_stream_t stream) {
    return edge_update_bwd<bf16_t>(N, E, H, dst, coef, g, d_diff, stream);
}

int dn_sie_pool_sum_f32(int64_t B, const int32_t* edge_ptr, const uint8_t* skip, const int32_t* src, const int32_t* dst, int64_t N,
                        const int32_t* id, const float* enc_v, int32_t rows_v, int32_t Kv, const int32_t* vlabel, const float* enc_vl,
                        int32_t rows_vl, int32_t Kvl, const int32_t* elabel, const float* enc_el, int32_t rows_el, int32_t Kel,
                        const int32_t* out_deg, const int32_t* in_deg, const float* rep, int32_t H, float* pooled, int32_t* count,
                        dn_stream_t stream) {
    return edge_pool_sum<float>(B, edge_ptr, skip, src, dst, N, id, enc_v, rows_v, Kv, vlabel, enc_vl, rows_vl, Kvl, elabel, enc_el,
                                rows_el, Kel, out_deg, in_deg, rep, H, pooled, count, stream);
}
int dn_sie_pool_sum_bf16(int64_t B, const int32_t* edge_ptr, const uint8_t* skip, const int32_t* src, const int32_t* dst, int64_t N,
                         const int32_t* id, const void* enc_v, int32_t rows_v, int32_t Kv, const int32_t* vlabel, const void* enc_vl,
                         int32_t rows_vl, int32_t Kvl, const int32_t* elabel, const void* enc_el, int32_t rows_el, int32_t Kel,
                         const int32_t* out_deg, const int32_t* in_deg, const void* rep, int32_t H, float* pooled, int32_t* count,
                         dn_stream_t stream) {
    return edge_pool_sum<bf16_t>(B, edge_ptr, skip, src, dst, N, id, enc_v, rows_v, Kv, vlabel, enc_vl, rows_vl, Kvl, elabel, enc_el,
                                 rows_el, Kel, out_deg, in_deg, rep, H, pooled, count, stream);
}

}  // extern "C"
