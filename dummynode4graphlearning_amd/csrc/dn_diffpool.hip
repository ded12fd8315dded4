// DiffPool on ragged rows (graph_classification/diffpool.py; reference: models/diffpool.py + torch_geometric's dense_diff_pool, which
// pad the batch to [B, Nmax, .] and multiply through a dense [B, Nmax, Nmax] adjacency).
//
//   dn_segment_gram_f32            out[g] = L[rows_g]^T R[rows_g]  ([CL, CR] per graph): a product whose K dimension is the ragged row
//                                  range of a graph, on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32: bit for bit a k-ordered fmaf chain).
//   dn_diffpool_softmax_fwd / bwd  S = softmax(logits) over the C cluster columns; dlogits = S (dS - rowsum(dS S)), dS = d0 + d1 + d2.
//   dn_diffpool_assign_graphs_f32  the graphs whose S fits in LDS, each taken WHOLE by one workgroup: row softmax into LDS (S stored
//                                  once for the backward), A S gathered from LDS through the graph's slice of the CSR by source
//                                  (row i receives the S rows of its out-edges' destinations, duplicates counted), then X' = S^T z with z
//                                  streamed in 16-row tiles and A' = S^T (A S) entirely from LDS.
//
// One product scheme for all three: a 256-thread workgroup owns 64 output columns and ALL CL <= 256 output rows; wave w owns the 16
// columns 16 w .. 16 w + 15 and up to 16 accumulators (one per 16 output rows).  A step of 4 k takes one LDS read of the B operand and
// one per accumulator of the A operand.  The rows of a graph are walked in order by one workgroup: no split K, no atomics, the same
// bits on every run.  fp32 only.
#include "dn_common.h"
#include "dn_hip.h"
#include "dn_rows.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxC = 256;               // cluster columns (the A operand's width: 16 accumulators of 16 rows)
constexpr int kMaxF = 512;               // feature columns
constexpr int kMaxTiles = kMaxC / 16;
constexpr int kKT = 16;                  // rows of a graph per staged tile
constexpr int kCT = 64;                  // output columns per workgroup
constexpr int kRS = kCT + 16;            // row stride of the staged B tile: the 4 k-rows of a step land on 4 different bank groups
constexpr int kLdsFloats = 16384;        // S (and A S) of a whole-graph workgroup: rows rounded up to 16 times the padded stride

// Stride of an operand with C columns held [row][column] in LDS: C rounded up to 16 (the padding is zero), and == 16 (mod 32) so that
// the rows k .. k + 3 a step reads start 16 banks apart.
__host__ __device__ constexpr int dp_stride(int C) {
    const int p = (C + 15) / 16 * 16;
    return p % 32 == 16 ? p : p + 16;
}

// acc[m] += A[k + q][16 m + j]^T-fragment times b, for the nclt row tiles of the output (wave-uniform nclt): a_row = &A[k + q][j]
__device__ __forceinline__ void dp_mma(f32x4 (&acc)[kMaxTiles], int nclt, const float* a_row, float b) {
#pragma unroll
    for (int m = 0; m < kMaxTiles; ++m)
        if (m < nclt) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a_row[16 * m], b, acc[m], 0, 0, 0);
}

__device__ __forceinline__ void dp_clear(f32x4 (&acc)[kMaxTiles]) {
#pragma unroll
    for (int m = 0; m < kMaxTiles; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// lane (j = lane & 15, q = lane >> 4) holds out[16 m + 4 q + reg][col] of its wave's column col
__device__ __forceinline__ void dp_store(const f32x4 (&acc)[kMaxTiles], int nclt, int CL, int CR, int col, int q, float* __restrict__ out) {
    if (col >= CR) return;
#pragma unroll
    for (int m = 0; m < kMaxTiles; ++m)
        if (m < nclt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * m + 4 * q + r;
                if (row < CL) out[(size_t)row * CR + col] = acc[m][r];
            }
        }
}

__device__ __forceinline__ void dp_row_range(const int32_t* __restrict__ gptr, int64_t g, int64_t N, int64_t& beg, int64_t& end) {
    beg = gptr[g];
    end = gptr[g + 1];
    beg = beg < 0 ? 0 : (beg > N ? N : beg);
    end = end < beg ? beg : (end > N ? N : end);
}

// ---------------------------------------------------------------------------------------------- out[g] = L[rows_g]^T R[rows_g]
__global__ __launch_bounds__(kBlock) void segment_gram_kernel(int64_t B, int64_t N, int CL, int CR, const int32_t* __restrict__ graphs,
                                                              const int32_t* __restrict__ gptr, const float* __restrict__ L, const float* __restrict__ R,
                                                              float* __restrict__ out) {
    __shared__ float Ls[kKT * dp_stride(kMaxC)];
    __shared__ float Rs[kKT * kRS];
    const int64_t g = graphs ? (int64_t)graphs[blockIdx.x] : (int64_t)blockIdx.x;       // (a list: only those graphs are written)
    if (g < 0 || g >= B) return;
    const int c0 = blockIdx.y * kCT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, q = lane >> 4;
    const int nclt = (CL + 15) >> 4, SS = dp_stride(CL);
    const bool active = c0 + 16 * wave < CR;
    int64_t beg, end;
    dp_row_range(gptr, g, N, beg, end);
    f32x4 acc[kMaxTiles];
    dp_clear(acc);
    for (int64_t k0 = beg; k0 < end; k0 += kKT) {
        __syncthreads();                                                  // the previous tile has been read
        for (int idx = tid; idx < kKT * SS; idx += kBlock) {
            const int r = idx / SS, c = idx - r * SS;
            const int64_t row = k0 + r;
            Ls[idx] = (row < end && c < CL) ? L[row * CL + c] : 0.f;
        }
        for (int idx = tid; idx < kKT * kCT; idx += kBlock) {
            const int r = idx >> 6, c = idx & 63;
            const int64_t row = k0 + r;
            Rs[r * kRS + c] = (row < end && c0 + c < CR) ? R[row * CR + c0 + c] : 0.f;
        }
        __syncthreads();
        if (active) {
#pragma unroll
            for (int kk = 0; kk < kKT; kk += 4) dp_mma(acc, nclt, Ls + (kk + q) * SS + j, Rs[(kk + q) * kRS + 16 * wave + j]);
        }
    }
    if (active) dp_store(acc, nclt, CL, CR, c0 + 16 * wave + j, q, out + (size_t)g * CL * CR);
}

// ---------------------------------------------------------------------------------------------- row softmax: one wavefront per row
constexpr int kPerLane = kMaxC / 64;     // columns lane, lane + 64, ... of a row

// s[i] = softmax(x)[lane + 64 i]  (0 past C)
__device__ __forceinline__ void dp_softmax_row(const float* __restrict__ x, int C, int lane, float (&s)[kPerLane]) {
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < kPerLane; ++i) {
        const int c = lane + 64 * i;
        s[i] = c < C ? x[c] : -INFINITY;
        mx = fmaxf(mx, s[i]);
    }
    mx = dn_wave_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < kPerLane; ++i) {
        s[i] = lane + 64 * i < C ? expf(s[i] - mx) : 0.f;
        sum += s[i];
    }
    sum = dn_wave_sum(sum);
    const float inv = 1.f / sum;
#pragma unroll
    for (int i = 0; i < kPerLane; ++i) s[i] *= inv;
}

__global__ __launch_bounds__(kBlock) void softmax_fwd_kernel(int64_t N, int C, const float* __restrict__ x, float* __restrict__ S) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (row >= N) return;
    float s[kPerLane];
    dp_softmax_row(x + row * C, C, lane, s);
#pragma unroll
    for (int i = 0; i < kPerLane; ++i)
        if (lane + 64 * i < C) S[row * C + lane + 64 * i] = s[i];
}

__global__ __launch_bounds__(kBlock) void softmax_bwd_kernel(int64_t N, int C, const float* __restrict__ S, const float* __restrict__ d0,
                                                             const float* __restrict__ d1, const float* __restrict__ d2,
                                                             float* __restrict__ dx) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (row >= N) return;
    float s[kPerLane], d[kPerLane], dot = 0.f;
#pragma unroll
    for (int i = 0; i < kPerLane; ++i) {
        const int c = lane + 64 * i;
        s[i] = d[i] = 0.f;
        if (c < C) {
            const int64_t at = row * C + c;
            s[i] = S[at];
            d[i] = d0[at];
            if (d1) d[i] += d1[at];
            if (d2) d[i] += d2[at];
        }
        dot += s[i] * d[i];
    }
    dot = dn_wave_sum(dot);
#pragma unroll
    for (int i = 0; i < kPerLane; ++i)
        if (lane + 64 * i < C) dx[row * C + lane + 64 * i] = s[i] * (d[i] - dot);
}

// ---------------------------------------------------------------------------------------------- a whole graph per workgroup
constexpr int kPadLane = (dp_stride(kMaxC) + 63) / 64;    // columns of a padded LDS row per lane

__global__ __launch_bounds__(kBlock) void assign_graphs_kernel(int64_t B, int64_t N, int64_t E, int C, int F, int np_max,
                                                               const int32_t* __restrict__ graphs, const int32_t* __restrict__ gptr,
                                                               const int32_t* __restrict__ optr, const int32_t* __restrict__ onbr,
                                                               const float* __restrict__ logits, const float* __restrict__ z,
                                                               float* __restrict__ S, float* __restrict__ AS, float* __restrict__ X,
                                                               float* __restrict__ A) {
    extern __shared__ __attribute__((aligned(16))) float dp_smem[];
    const int64_t g = graphs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, q = lane >> 4;
    const int nclt = (C + 15) >> 4, SS = dp_stride(C);
    if (g < 0 || g >= B) return;
    int64_t beg, end;
    dp_row_range(gptr, g, N, beg, end);
    const int64_t n64 = end - beg;
    if ((n64 + 15) / 16 * 16 > np_max) return;                            // (not of this class: the host lists none; LDS stays in bounds)
    const int n = (int)n64, NP = (n + 15) / 16 * 16;
    float* Ss = dp_smem;                                                  // [np_max][SS]  softmax rows, zero padded
    float* As = Ss + (size_t)np_max * SS;                                 // [np_max][SS]  A S
    float* Zs = As + (size_t)np_max * SS;                                 // [kKT][kRS]    a tile of z

    for (int r = wave; r < NP; r += kWaves) {
        float s[kPerLane];
        if (r < n) dp_softmax_row(logits + (beg + r) * C, C, lane, s);
#pragma unroll
        for (int i = 0; i < kPadLane; ++i) {
            const int c = lane + 64 * i;
            if (c < SS) {
                const bool live = r < n && c < C;
                const float v = live ? s[i < kPerLane ? i : 0] : 0.f;
                Ss[r * SS + c] = v;
                if (live) S[(beg + r) * C + c] = v;
            }
        }
    }
    __syncthreads();
    for (int r = wave; r < NP; r += kWaves) {
        float a[kPadLane];
#pragma unroll
        for (int i = 0; i < kPadLane; ++i) a[i] = 0.f;
        if (r < n) {
            int64_t e0, e1;
            dn_csr_range(optr, beg + r, E, e0, e1);
            for (int64_t e = e0; e < e1; ++e) {
                const int64_t d = (int64_t)onbr[e] - beg;
                if (d < 0 || d >= n) continue;                            // (an edge that leaves its graph: the host refuses such a batch)
#pragma unroll
                for (int i = 0; i < kPadLane; ++i)
                    if (lane + 64 * i < SS) a[i] += Ss[(int)d * SS + lane + 64 * i];
            }
        }
#pragma unroll
        for (int i = 0; i < kPadLane; ++i) {
            const int c = lane + 64 * i;
            if (c < SS) {
                As[r * SS + c] = a[i];
                if (r < n && c < C) AS[(beg + r) * C + c] = a[i];
            }
        }
    }
    __syncthreads();

    f32x4 acc[kMaxTiles];
    for (int c0 = 0; c0 < F; c0 += kCT) {                                 // X' = S^T z
        const bool active = c0 + 16 * wave < F;
        dp_clear(acc);
        for (int k0 = 0; k0 < n; k0 += kKT) {
            __syncthreads();
            for (int idx = tid; idx < kKT * kCT; idx += kBlock) {
                const int r = idx >> 6, c = idx & 63;
                Zs[r * kRS + c] = (k0 + r < n && c0 + c < F) ? z[(beg + k0 + r) * F + c0 + c] : 0.f;
            }
            __syncthreads();
            if (active) {
#pragma unroll
                for (int kk = 0; kk < kKT; kk += 4) dp_mma(acc, nclt, Ss + (k0 + kk + q) * SS + j, Zs[(kk + q) * kRS + 16 * wave + j]);
            }
        }
        if (active) dp_store(acc, nclt, C, F, c0 + 16 * wave + j, q, X + (size_t)g * C * F);
    }
    for (int c0 = 0; c0 < C; c0 += kCT) {                                 // A' = S^T (A S)
        if (c0 + 16 * wave >= C) continue;                                // (no barrier below)
        dp_clear(acc);
        for (int k = 0; k < NP; k += 4) dp_mma(acc, nclt, Ss + (k + q) * SS + j, As[(k + q) * SS + c0 + 16 * wave + j]);
        dp_store(acc, nclt, C, C, c0 + 16 * wave + j, q, A + (size_t)g * C * C);
    }
}

// ---------------------------------------------------------------------------------------------- host checks
int check_rows(const char* what, int64_t N, int32_t C) {
    DN_REQUIRE(N >= 1 && N < 0x7fffffffLL / kMaxF, "%s: bad sizes (N = %lld; must be positive)", what, (long long)N);
    DN_REQUIRE(C >= 1 && C <= kMaxC, "%s: 1 <= C <= %d cluster columns (got %d)", what, kMaxC, C);
    return DN_OK;
}

int graph_rows(int32_t C) { return kLdsFloats / dp_stride(C) / 16 * 16; }

}  // namespace

extern "C" {

int32_t dn_diffpool_max_clusters(void) { return kMaxC; }
int32_t dn_diffpool_max_features(void) { return kMaxF; }
int32_t dn_diffpool_graph_rows(int32_t C) { return C >= 1 && C <= kMaxC ? graph_rows(C) : 0; }

int dn_segment_gram_f32(int64_t B, int64_t N, int32_t CL, int32_t CR, const int32_t* graphs, int64_t num_list, const int32_t* graph_ptr,
                        const float* L, const float* R, float* out, dn_stream_t stream) {
    DN_REQUIRE(B >= 1 && B < 0x7fffffffLL, "dn_segment_gram: bad sizes (B = %lld; must be positive)", (long long)B);
    DN_REQUIRE(graphs ? (num_list >= 1 && num_list <= B) : num_list == 0,
               "dn_segment_gram: bad list (%lld graphs listed of %lld; 0 without a list)", (long long)num_list, (long long)B);
    if (int rc = check_rows("dn_segment_gram", N, CL)) return rc;
    DN_REQUIRE(CR >= 1 && CR <= kMaxF, "dn_segment_gram: 1 <= CR <= %d columns (got %d)", kMaxF, CR);
    DN_REQUIRE(graph_ptr && L && R && out, "dn_segment_gram: NULL pointer");
    hipLaunchKernelGGL(segment_gram_kernel, dim3((unsigned)(graphs ? num_list : B), (unsigned)dn_cdiv(CR, kCT)), dim3(kBlock), 0,
                       (hipStream_t)stream, B, N, CL, CR, graphs, graph_ptr, L, R, out);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_diffpool_softmax_fwd_f32(int64_t N, int32_t C, const float* logits, float* S, dn_stream_t stream) {
    if (int rc = check_rows("dn_diffpool_softmax_fwd", N, C)) return rc;
    DN_REQUIRE(logits && S, "dn_diffpool_softmax_fwd: NULL pointer");
    hipLaunchKernelGGL(softmax_fwd_kernel, dim3((unsigned)dn_cdiv(N, kWaves)), dim3(kBlock), 0, (hipStream_t)stream, N, C, logits, S);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_diffpool_softmax_bwd_f32(int64_t N, int32_t C, const float* S, const float* d0, const float* d1, const float* d2, float* dlogits,
                                dn_stream_t stream) {
    if (int rc = check_rows("dn_diffpool_softmax_bwd", N, C)) return rc;
    DN_REQUIRE(S && d0 && dlogits, "dn_diffpool_softmax_bwd: NULL pointer");
    hipLaunchKernelGGL(softmax_bwd_kernel, dim3((unsigned)dn_cdiv(N, kWaves)), dim3(kBlock), 0, (hipStream_t)stream, N, C, S, d0, d1, d2,
                       dlogits);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_diffpool_assign_graphs_f32(int64_t B, int64_t N, int64_t E, int64_t num_list, int32_t max_rows, int32_t C, int32_t F,
                                  const int32_t* graphs, const int32_t* graph_ptr, const int32_t* out_ptr, const int32_t* dst_by_src,
                                  const float* logits, const float* z, float* S, float* AS, float* X, float* A, dn_stream_t stream) {
    DN_REQUIRE(B >= 1 && B < 0x7fffffffLL && num_list >= 1 && num_list <= B && E >= 0 && E < 0x7fffffffLL,
               "dn_diffpool_assign_graphs: bad sizes (B = %lld, listed = %lld, E = %lld)", (long long)B, (long long)num_list, (long long)E);
    if (int rc = check_rows("dn_diffpool_assign_graphs", N, C)) return rc;
    DN_REQUIRE(F >= 1 && F <= kMaxF, "dn_diffpool_assign_graphs: 1 <= F <= %d feature columns (got %d)", kMaxF, F);
    DN_REQUIRE(max_rows >= 0 && max_rows <= graph_rows(C),
               "dn_diffpool_assign_graphs: graph over the class limit: at most %d rows at C = %d (got %d)", graph_rows(C), C, max_rows);
    DN_REQUIRE(graphs && graph_ptr && out_ptr && logits && z && S && AS && X && A && (dst_by_src || E == 0),
               "dn_diffpool_assign_graphs: NULL pointer");
    const int np_max = (max_rows + 15) / 16 * 16;
    const size_t lds = ((size_t)2 * np_max * dp_stride(C) + kKT * kRS) * sizeof(float);
    if (int rc = dn_allow_lds(assign_graphs_kernel, lds)) return rc;
    hipLaunchKernelGGL(assign_graphs_kernel, dim3((unsigned)num_list), dim3(kBlock), lds, (hipStream_t)stream, B, N, E, C, F, np_max, graphs,
                       graph_ptr, out_ptr, dst_by_src, logits, z, S, AS, X, A);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

}  // extern "C"
