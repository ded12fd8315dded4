// HGT (heterogeneous graph transformer) edge-softmax attention of the SI count model HGT (subgraph_isomorphism/models/hgt.py).
//
// The per-edge-type d_k x d_k matrices stay OUTSIDE these kernels, on the destination side (docs/LAB_NOTES.md "SI count models:
// HGT").  A "pair" is a (destination, edge type) that has at least one edge; the caller hands in Qp [P, H] = q_dst @ blockdiag(att[r])^T
// for every pair and receives U [P, H] = the attention-weighted sums of the plain value rows of the pair's edges, which the relation-
// grouped product with blockdiag(msg[r]) and a sum over the pairs of a destination turn into the layer's aggregate.  The rows of
// Qp / U (and of their gradients) are stored grouped by edge type, the order the grouped products want: pair_row [P] is a pair's row,
// row_s [E] the row of an edge's pair.  What is left here are dot products and weighted sums of H-wide rows:
//
//     logit[e, h] = <Qp[pair_e, h], k[src_e, h]> * pri[et_e, h] * scale        softmax over ALL in-edges of dst, per head
//     U[p]        = sum over the edges of pair p of a[e, head(c)] * v[src_e, c]
//
// The edges come sorted by (destination, edge type) (ops.HgtIndex): dst_ptr [N + 1] bounds the pairs of every destination (they are
// consecutive), pair_ptr [P + 1] the edges of every pair, so the in-edges of d are pair_ptr[dst_ptr[d]] .. pair_ptr[dst_ptr[d + 1]].
// Mapping: ONE WORKGROUP of 256 threads per destination.  The (edge, head) logits of the segment are spread over all 256 threads (a
// thread's head is fixed: 256 % heads == 0), the max and the sum are reduced per head by xor shuffles inside a wave and a fixed-order
// sum of the four wave results.  For the weighted sums a row is H / 4 float4 lanes wide, so 256 / (H / 4) edge slots run side by side
// (4 at H = 256, 16 at H = 64) and their partial rows are folded through LDS in slot order: a hub segment (the dummy node) is
// walked by the whole workgroup, never by one lane group.  Nothing of size E x H is stored; the only per-edge outputs are
// [E, heads].  No atomics: two runs give the same bits.
#include <hip/hip_runtime.h>
#include <math.h>

#include "dn_common.h"
#include "dn_hip.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxH = 256;
constexpr int kMaxHeads = 8;

__device__ __forceinline__ float4 f4_fma(float w, const float4 a, float4 acc) {
    acc.x = fmaf(w, a.x, acc.x);
    acc.y = fmaf(w, a.y, acc.y);
    acc.z = fmaf(w, a.z, acc.z);
    acc.w = fmaf(w, a.w, acc.w);
    return acc;
}

__device__ __forceinline__ float4 f4_add(float4 a, const float4 b) {
    a.x += b.x;
    a.y += b.y;
    a.z += b.z;
    a.w += b.w;
    return a;
}

__device__ __forceinline__ float dot_rows(const float* a, const float* b, int n4) {
    const float4* a4 = reinterpret_cast<const float4*>(a);
    const float4* b4 = reinterpret_cast<const float4*>(b);
    float s = 0.f;
    for (int j = 0; j < n4; ++j) {
        const float4 x = a4[j], y = b4[j];
        s = fmaf(x.x, y.x, s);
        s = fmaf(x.y, y.y, s);
        s = fmaf(x.z, y.z, s);
        s = fmaf(x.w, y.w, s);
    }
    return s;
}

// The reduction over all threads of the workgroup that share threadIdx.x % heads; every thread calls it and gets the result of its
// head.  Butterfly inside a wave (every lane ends with the same bits), then the four wave results in wave order.
template <bool kMax>
__device__ __forceinline__ float block_head_reduce(float v, int heads, float* red) {
    for (int o = 32; o >= heads; o >>= 1) {
        const float u = __shfl_xor(v, o, 64);
        v = kMax ? fmaxf(v, u) : v + u;
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();                                       // (the previous call's readers are done with red)
    if (lane < heads) red[w * kMaxHeads + lane] = v;
    __syncthreads();
    const int h = lane % heads;
    float r = red[h];
    for (int i = 1; i < kBlock / 64; ++i) r = kMax ? fmaxf(r, red[i * kMaxHeads + h]) : r + red[i * kMaxHeads + h];
    return r;
}

// acc of slot 0 <- the partial rows of the first nslots slots in slot order (all threads call it: nslots is workgroup-uniform)
__device__ __forceinline__ float4 fold_slots(float4 acc, int nslots, int CL, int cg, int es, bool live, float4* fold) {
    if (nslots > 1) {
        __syncthreads();                                   // (the previous fold's readers are done)
        if (live) fold[es * CL + cg] = acc;
        __syncthreads();
        if (es == 0)
            for (int s = 1; s < nslots; ++s) acc = f4_add(acc, fold[s * CL + cg]);
    }
    return acc;
}

__global__ __launch_bounds__(kBlock) void hgt_fwd_kernel(int32_t H, int32_t heads, const int32_t* __restrict__ dst_ptr,
                                                         const int32_t* __restrict__ pair_ptr, const int32_t* __restrict__ pair_row,
                                                         const int32_t* __restrict__ src_s, const int32_t* __restrict__ et_s,
                                                         const int32_t* __restrict__ row_s, const float* __restrict__ Qp,
                                                         const float* __restrict__ K,
                                                         const float* __restrict__ V, const float* __restrict__ pri, float scale,
                                                         float* __restrict__ att, float* __restrict__ U) {
    __shared__ float red[(kBlock / 64) * kMaxHeads];
    __shared__ float4 fold[kBlock];
    const int t = threadIdx.x;
    const size_t d = blockIdx.x;
    const int dk = H / heads, dk4 = dk >> 2;
    const int32_t p0 = dst_ptr[d], p1 = dst_ptr[d + 1];
    const int32_t beg = pair_ptr[p0], end = pair_ptr[p1];
    const int64_t items = (int64_t)(end - beg) * heads;
    const int h = t % heads;

    float mx = -INFINITY;
    for (int64_t i = t; i < items; i += kBlock) {
        const int32_t e = beg + (int32_t)(i / heads);
        const float dot = dot_rows(Qp + (size_t)row_s[e] * H + h * dk, K + (size_t)src_s[e] * H + h * dk, dk4);
        const float l = dot * pri[et_s[e] * heads + h] * scale;
        att[(size_t)e * heads + h] = l;
        mx = fmaxf(mx, l);
    }
    mx = block_head_reduce<true>(mx, heads, red);
    float sm = 0.f;
    for (int64_t i = t; i < items; i += kBlock) {           // (a thread reads back what it stored itself)
        const size_t a = (size_t)(beg + (int32_t)(i / heads)) * heads + h;
        const float w = expf(att[a] - mx);
        att[a] = w;
        sm += w;
    }
    sm = block_head_reduce<false>(sm, heads, red);
    const float inv = 1.f / sm;                             // (sm >= 1 wherever an item exists)
    for (int64_t i = t; i < items; i += kBlock) {
        const size_t a = (size_t)(beg + (int32_t)(i / heads)) * heads + h;
        att[a] *= inv;
    }
    __syncthreads();                                        // att of the segment is visible to the workgroup

    const int CL = H >> 2, S = kBlock / CL;
    const int cg = t % CL, es = t / CL;
    const bool live = es < S;
    const int hc = (cg << 2) / dk;
    for (int32_t p = p0; p < p1; ++p) {
        const int32_t sb = pair_ptr[p], se = pair_ptr[p + 1];
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live)
            for (int32_t e = sb + es; e < se; e += S)
                acc = f4_fma(att[(size_t)e * heads + hc], reinterpret_cast<const float4*>(V + (size_t)src_s[e] * H)[cg], acc);
        acc = fold_slots(acc, min(se - sb, S), CL, cg, es, live, fold);
        if (es == 0) reinterpret_cast<float4*>(U + (size_t)pair_row[p] * H)[cg] = acc;
    }
}

// Destination order: da = <dU[pair, h], v[src, h]>, dlogit = a (da - sum a da), dl = dlogit pri scale (the gradient of the raw dot
// product, [E, heads]), dQp[p] = sum dl k[src], and the pair's partial of d pri: dpri_part[p, h] = sum dlogit dot scale.
__global__ __launch_bounds__(kBlock) void hgt_bwd_dst_kernel(int32_t H, int32_t heads, const int32_t* __restrict__ dst_ptr,
                                                             const int32_t* __restrict__ pair_ptr, const int32_t* __restrict__ pair_rel,
                                                             const int32_t* __restrict__ pair_row, const int32_t* __restrict__ src_s,
                                                             const int32_t* __restrict__ row_s, const float* __restrict__ Qp,
                                                             const float* __restrict__ K, const float* __restrict__ V,
                                                             const float* __restrict__ pri, float scale,
                                                             const float* __restrict__ att, const float* __restrict__ dU,
                                                             float* __restrict__ dl, float* __restrict__ dQp,
                                                             float* __restrict__ dpri_part) {
    __shared__ float red[(kBlock / 64) * kMaxHeads];
    __shared__ float4 fold[kBlock];
    const int t = threadIdx.x;
    const size_t d = blockIdx.x;
    const int dk = H / heads, dk4 = dk >> 2;
    const int32_t p0 = dst_ptr[d], p1 = dst_ptr[d + 1];
    const int32_t beg = pair_ptr[p0], end = pair_ptr[p1];
    const int64_t items = (int64_t)(end - beg) * heads;
    const int h = t % heads;

    float sa = 0.f;
    for (int64_t i = t; i < items; i += kBlock) {
        const int32_t e = beg + (int32_t)(i / heads);
        const float da = dot_rows(dU + (size_t)row_s[e] * H + h * dk, V + (size_t)src_s[e] * H + h * dk, dk4);
        const size_t a = (size_t)e * heads + h;
        dl[a] = da;
        sa = fmaf(att[a], da, sa);
    }
    sa = block_head_reduce<false>(sa, heads, red);

    const int CL = H >> 2, S = kBlock / CL;
    const int cg = t % CL, es = t / CL;
    const bool live = es < S;
    const int hc = (cg << 2) / dk;
    for (int32_t p = p0; p < p1; ++p) {
        const int32_t sb = pair_ptr[p], se = pair_ptr[p + 1];
        const int64_t n = (int64_t)(se - sb) * heads;
        const size_t prow = (size_t)pair_row[p];
        const float ps = pri[pair_rel[p] * heads + h] * scale;
        float pp = 0.f;
        for (int64_t i = t; i < n; i += kBlock) {           // (da: stored in front of the barriers of the reduction above)
            const int32_t e = sb + (int32_t)(i / heads);
            const size_t a = (size_t)e * heads + h;
            const float dlog = att[a] * (dl[a] - sa);
            const float dot = dot_rows(Qp + prow * H + h * dk, K + (size_t)src_s[e] * H + h * dk, dk4);
            pp = fmaf(dlog, dot * scale, pp);
            dl[a] = dlog * ps;
        }
        pp = block_head_reduce<false>(pp, heads, red);
        __syncthreads();                                    // dl of the pair is visible to the workgroup
        if (t < heads) dpri_part[prow * heads + t] = pp;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live)
            for (int32_t e = sb + es; e < se; e += S)
                acc = f4_fma(dl[(size_t)e * heads + hc], reinterpret_cast<const float4*>(K + (size_t)src_s[e] * H)[cg], acc);
        acc = fold_slots(acc, min(se - sb, S), CL, cg, es, live, fold);
        if (es == 0) reinterpret_cast<float4*>(dQp + prow * H)[cg] = acc;
    }
}

// Source order (the reverse CSR: out_pos = the edge's place in the destination order, out_row = the row of its pair): dk[s] = sum dl Qp[row],
// dv[s] = sum a dU[row]
__global__ __launch_bounds__(kBlock) void hgt_bwd_src_kernel(int32_t H, int32_t heads, const int32_t* __restrict__ out_ptr,
                                                             const int32_t* __restrict__ out_pos, const int32_t* __restrict__ out_row,
                                                             const float* __restrict__ Qp, const float* __restrict__ dU,
                                                             const float* __restrict__ att, const float* __restrict__ dl,
                                                             float* __restrict__ dK, float* __restrict__ dV) {
    __shared__ float4 fold[kBlock];
    const int t = threadIdx.x;
    const size_t s = blockIdx.x;
    const int dk = H / heads;
    const int CL = H >> 2, S = kBlock / CL;
    const int cg = t % CL, es = t / CL;
    const bool live = es < S;
    const int hc = (cg << 2) / dk;
    const int32_t sb = out_ptr[s], se = out_ptr[s + 1];
    float4 ak = make_float4(0.f, 0.f, 0.f, 0.f), av = ak;
    if (live)
        for (int32_t j = sb + es; j < se; j += S) {
            const size_t a = (size_t)out_pos[j] * heads + hc;
            const size_t row = (size_t)out_row[j] * CL + cg;
            ak = f4_fma(dl[a], reinterpret_cast<const float4*>(Qp)[row], ak);
            av = f4_fma(att[a], reinterpret_cast<const float4*>(dU)[row], av);
        }
    const int nslots = min(se - sb, S);
    ak = fold_slots(ak, nslots, CL, cg, es, live, fold);
    av = fold_slots(av, nslots, CL, cg, es, live, fold);
    if (es == 0) {
        reinterpret_cast<float4*>(dK + s * H)[cg] = ak;
        reinterpret_cast<float4*>(dV + s * H)[cg] = av;
    }
}

int check_shape(const char* what, int64_t N, int64_t E, int64_t P, int32_t H, int32_t heads) {
    DN_REQUIRE(N >= 0 && E >= 0 && P >= 0 && N < 0x7fffffffLL && E < 0x7fffffffLL && P <= E, "%s: bad sizes", what);
    DN_REQUIRE(heads == 1 || heads == 2 || heads == 4 || heads == 8, "%s: heads must be 1, 2, 4 or 8 (got %d)", what, heads);
    DN_REQUIRE(H >= 4 && H <= kMaxH && H % heads == 0 && (H / heads) % 4 == 0,
               "%s: H <= %d with H / heads a multiple of 4 (got H = %d, heads = %d)", what, kMaxH, H, heads);
    return DN_OK;
}

}  // namespace

extern "C" {

int dn_hgt_attn_fwd_f32(int64_t N, int64_t E, int64_t P, int32_t H, int32_t heads, const int32_t* dst_ptr, const int32_t* pair_ptr,
                        const int32_t* pair_row, const int32_t* src_s, const int32_t* et_s, const int32_t* row_s, const float* Qp,
                        const float* K, const float* V, const float* pri, float scale, float* att, float* U, dn_stream_t stream) {
    if (int rc = check_shape("dn_hgt_attn_fwd", N, E, P, H, heads)) return rc;
    if (N == 0) return DN_OK;
    DN_REQUIRE(dst_ptr && pair_ptr && K && V && pri, "dn_hgt_attn_fwd: NULL pointer");
    DN_REQUIRE(E == 0 || (pair_row && src_s && et_s && row_s && Qp && att && U), "dn_hgt_attn_fwd: NULL pointer");
    hipLaunchKernelGGL(hgt_fwd_kernel, dim3((unsigned)N), dim3(kBlock), 0, (hipStream_t)stream, H, heads, dst_ptr, pair_ptr, pair_row,
                       src_s, et_s, row_s, Qp, K, V, pri, scale, att, U);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_hgt_attn_bwd_dst_f32(int64_t N, int64_t E, int64_t P, int32_t H, int32_t heads, const int32_t* dst_ptr, const int32_t* pair_ptr,
                            const int32_t* pair_rel, const int32_t* pair_row, const int32_t* src_s, const int32_t* row_s, const float* Qp,
                            const float* K, const float* V, const float* pri, float scale, const float* att, const float* dU, float* dl,
                            float* dQp, float* dpri_part, dn_stream_t stream) {
    if (int rc = check_shape("dn_hgt_attn_bwd_dst", N, E, P, H, heads)) return rc;
    if (N == 0 || E == 0) return DN_OK;
    DN_REQUIRE(dst_ptr && pair_ptr && pair_rel && pair_row && src_s && row_s && Qp && K && V && pri && att && dU && dl && dQp && dpri_part,
               "dn_hgt_attn_bwd_dst: NULL pointer");
    hipLaunchKernelGGL(hgt_bwd_dst_kernel, dim3((unsigned)N), dim3(kBlock), 0, (hipStream_t)stream, H, heads, dst_ptr, pair_ptr, pair_rel,
                       pair_row, src_s, row_s, Qp, K, V, pri, scale, att, dU, dl, dQp, dpri_part);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_hgt_attn_bwd_src_f32(int64_t N, int64_t E, int64_t P, int32_t H, int32_t heads, const int32_t* out_ptr, const int32_t* out_pos,
                            const int32_t* out_row, const float* Qp, const float* dU, const float* att, const float* dl, float* dK,
                            float* dV, dn_stream_t stream) {
    if (int rc = check_shape("dn_hgt_attn_bwd_src", N, E, P, H, heads)) return rc;
    if (N == 0) return DN_OK;
    DN_REQUIRE(out_ptr && dK && dV, "dn_hgt_attn_bwd_src: NULL pointer");
    DN_REQUIRE(E == 0 || (out_pos && out_row && Qp && dU && att && dl), "dn_hgt_attn_bwd_src: NULL pointer");
    hipLaunchKernelGGL(hgt_bwd_src_kernel, dim3((unsigned)N), dim3(kBlock), 0, (hipStream_t)stream, H, heads, out_ptr, out_pos, out_row,
                       Qp, dU, att, dl, dK, dV);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

}  // extern "C"
