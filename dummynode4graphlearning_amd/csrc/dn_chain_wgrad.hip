// An RGIN layer's backward (bf16, H = 256) with Linear 1's weight gradient derived from the conv's.
//
// Nothing lies between the conv's output h = sum_r A_r Wc_r + 1 b^T and the MLP's first Linear z1 = h W1^T + b1, so with g1 = dL/dz1,
// g0 = g1 W1 = dL/dh, M_r = A_r^T g1 (fp32 [R + 1, H, H], the self loop last) and c = colsum(g1):
//
//     dWc_r = A_r^T g0 = M_r W1          db  = colsum(g0) = c W1
//     dW1   = g1^T h   = sum_r M_r^T Wc_r + c b^T          db1 = c
//
// -- 2 (R + 1) products of 256^3 (1.2 GFLOP at R = 16) on matrices that stay in the L2s, instead of the pass over every row of h that
// g1^T h costs (0.5 GB and a million rows of weight-gradient MFMAs on BASELINE config 5).  The conv's weight-gradient launch runs
// unchanged, with g1 as its gradient operand and fp32 output.
//
//   dn_layer_chain_dgrad_bf16      g0 = g1 W1 on the dense ring transform (dn_rel_ring.hip) + the per-graph sums of g1 that the
//                                  collapsed relation of that weight-gradient launch reads, from the same pass
//   dn_layer_chain_wgrad_combine   the products above.  A product of an fp32 and a bf16 value has 32 significant bits: it is exact in
//                                  fp64 and rounds in fp32, and a sum of signed terms may cancel to an output far below its terms,
//                                  whose bf16 ulp an fp32 accumulation cannot meet.  So the sums are kept in fp64 (v_fma_f64 tiles:
//                                  1.2 GFLOP is ~15 us of the vector unit) and every output is rounded ONCE, fp64 -> bf16.
//                                  Launch 1: workgroup (tile, r, kind) = one 64 x 64 tile of dWc_r (kind 0, stored as bf16) or of
//                                  P_r = M_r^T Wc_r (kind 1, fp64 into the workspace), K = 256 in chunks of 32 through LDS, a thread
//                                  owns 4 x 4 outputs; launch 2: dW1 = P_0 + ... + P_R + c b^T in that order, db, db1.  No atomics.
#include "dn_common.h"
#include "dn_internal.h"
#include "../../include/dn_hip.h"

namespace {

constexpr int kH = 256;
constexpr int kTile = 64;                      // output tile of a workgroup (256 threads: 4 x 4 outputs each)
constexpr int kKC = 32;                        // K chunk
constexpr int kThreads = 256;
constexpr int kAld = kTile + 2;                // A tile kept [k][m]: 528-byte rows (16-byte aligned; the transposing stores spread over the banks)

__device__ __forceinline__ double bf16_to_f64(bf16_t v) { return (double)(float)v; }

// fp64 -> bf16 with ONE rounding: to fp32 by round-to-odd (the sticky bit survives), then to nearest even
__device__ __forceinline__ bf16_t f64_to_bf16(double d) {
    float f = (float)d;
    if ((double)f != d && f == f && fabsf(f) < __builtin_huge_valf()) {
        uint32_t u = __float_as_uint(f);
        if (fabs((double)f) > fabs(d)) u -= 1u;                            // towards zero: the truncated value
        f = __uint_as_float(u | 1u);
    }
    return (bf16_t)f;
}

__global__ __launch_bounds__(kThreads) void chain_combine_products_kernel(const float* __restrict__ M, const bf16_t* __restrict__ W1,
                                                                          const bf16_t* __restrict__ Wc,
                                                                          const bf16_t* __restrict__ Wc_loop, int32_t R,
                                                                          bf16_t* __restrict__ dWc, double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) double As[kKC * kAld];         // [k][m]
    __shared__ __attribute__((aligned(16))) double Bs[kKC * kTile];        // [k][n]
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int m0 = (int)(blockIdx.x >> 2) * kTile, n0 = (int)(blockIdx.x & 3) * kTile;
    const int r = (int)blockIdx.y, kind = (int)blockIdx.z;
    const float* Mr = M + (size_t)r * kH * kH;
    const bf16_t* B = kind == 0 ? W1 : (r < R ? Wc + (size_t)r * kH * kH : Wc_loop);
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    // the next chunk's operands travel global -> registers under the current chunk's FMAs (their latency was what the launch waited for)
    float ra[8];
    bf16_t rb[8];
    auto fetch = [&](int kc) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            if (kind == 0) ra[s] = Mr[(size_t)(m0 + (tid >> 5) + 8 * s) * kH + kc + (tid & 31)];    // A[m][k] = M_r[m0 + m][kc + k]
            else ra[s] = Mr[(size_t)(kc + (tid >> 6) + 4 * s) * kH + m0 + (tid & 63)];              // A[m][k] = M_r[kc + k][m0 + m]
            rb[s] = B[(size_t)(kc + (tid >> 6) + 4 * s) * kH + n0 + (tid & 63)];
        }
    };
    fetch(0);
    for (int kc = 0; kc < kH; kc += kKC) {
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            if (kind == 0) As[(tid & 31) * kAld + (tid >> 5) + 8 * s] = (double)ra[s];
            else As[((tid >> 6) + 4 * s) * kAld + (tid & 63)] = (double)ra[s];
            Bs[((tid >> 6) + 4 * s) * kTile + (tid & 63)] = bf16_to_f64(rb[s]);
        }
        if (kc + kKC < kH) fetch(kc + kKC);
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < kKC; ++k) {
            const double2 a01 = *reinterpret_cast<const double2*>(&As[k * kAld + 4 * ty]);
            const double2 a23 = *reinterpret_cast<const double2*>(&As[k * kAld + 4 * ty + 2]);
            const double2 b01 = *reinterpret_cast<const double2*>(&Bs[k * kTile + 4 * tx]);
            const double2 b23 = *reinterpret_cast<const double2*>(&Bs[k * kTile + 4 * tx + 2]);
            const double a[4] = {a01.x, a01.y, a23.x, a23.y}, b[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fma(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t o = (size_t)r * kH * kH + (size_t)(m0 + 4 * ty + i) * kH + n0 + 4 * tx + j;
            if (kind == 0) dWc[o] = f64_to_bf16(acc[i][j]);
            else part[o] = acc[i][j];
        }
}

// blocks 0 .. 255: row j of dW1 = P_0[j] + ... + P_R[j] + c[j] b (relation order); block 256: db = c W1 (j in order), db1 = c
__global__ __launch_bounds__(kH) void chain_combine_finish_kernel(const double* __restrict__ part, const float* __restrict__ c,
                                                                  const bf16_t* __restrict__ W1, const bf16_t* __restrict__ bias,
                                                                  int32_t R, bf16_t* __restrict__ dW1, bf16_t* __restrict__ db,
                                                                  bf16_t* __restrict__ db1) {
    const int h = threadIdx.x, j = (int)blockIdx.x;
    if (j < kH) {
        double sum = 0.0;
        for (int r = 0; r <= R; ++r) sum += part[(size_t)r * kH * kH + (size_t)j * kH + h];
        if (bias) sum = fma((double)c[j], bf16_to_f64(bias[h]), sum);
        dW1[(size_t)j * kH + h] = f64_to_bf16(sum);
        return;
    }
    if (db) {
        double sum = 0.0;
        for (int jj = 0; jj < kH; ++jj) sum = fma((double)c[jj], bf16_to_f64(W1[(size_t)jj * kH + h]), sum);
        db[h] = f64_to_bf16(sum);
    }
    if (db1) db1[h] = (bf16_t)c[h];
}

}  // namespace

extern "C" int dn_layer_chain_dgrad_bf16(const void* G1, const void* W_kn, int64_t N, int32_t H, const int32_t* tiles, int64_t num_tiles,
                                         void* G0, void* seg_sums, dn_stream_t stream) {
    DN_REQUIRE(H == 256, "dn_layer_chain_dgrad: unsupported width %d (256 only)", H);
    DN_REQUIRE(N >= 0 && N < 0x7fffffffLL && num_tiles >= 0 && num_tiles < 0x7fffffffLL, "dn_layer_chain_dgrad: bad sizes");
    if (num_tiles == 0) return DN_OK;
    DN_REQUIRE(G1 && W_kn && tiles && G0 && seg_sums, "dn_layer_chain_dgrad: NULL pointer");
    DN_REQUIRE((reinterpret_cast<uintptr_t>(G1) | reinterpret_cast<uintptr_t>(W_kn) | reinterpret_cast<uintptr_t>(tiles) |
                reinterpret_cast<uintptr_t>(G0) | reinterpret_cast<uintptr_t>(seg_sums)) % 16 == 0, "dn_layer_chain_dgrad: unaligned pointer");
    return dn_internal::launch_transform_ring256_seg(G1, W_kn, tiles, num_tiles, G0, seg_sums, (hipStream_t)stream);
}

extern "C" size_t dn_layer_chain_wgrad_combine_workspace_bytes(int64_t R, int32_t H) {
    return R >= 0 && H > 0 ? (size_t)(R + 1) * (size_t)H * (size_t)H * sizeof(double) : 0;
}

extern "C" int dn_layer_chain_wgrad_combine(const float* M, const float* c, const void* W1, const void* Wc, const void* Wc_loop,
                                            const void* bias, int64_t R, int32_t H, void* dWc, void* db, void* dW1, void* db1,
                                            void* workspace, size_t workspace_bytes, dn_stream_t stream) {
    DN_REQUIRE(H == 256, "dn_layer_chain_wgrad_combine: unsupported width %d (256 only)", H);
    DN_REQUIRE(R >= 0 && R < 65535, "dn_layer_chain_wgrad_combine: bad relation count");
    DN_REQUIRE(M && c && W1 && Wc_loop && dWc && dW1 && workspace && (Wc || R == 0), "dn_layer_chain_wgrad_combine: NULL pointer");
    DN_REQUIRE(workspace_bytes >= dn_layer_chain_wgrad_combine_workspace_bytes(R, H), "dn_layer_chain_wgrad_combine: workspace too small");
    DN_REQUIRE((reinterpret_cast<uintptr_t>(M) | reinterpret_cast<uintptr_t>(workspace)) % 16 == 0,
               "dn_layer_chain_wgrad_combine: unaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)workspace;
    hipLaunchKernelGGL(chain_combine_products_kernel, dim3((kH / kTile) * (kH / kTile), (unsigned)(R + 1), 2), dim3(kThreads), 0, st, M,
                       (const bf16_t*)W1, (const bf16_t*)Wc, (const bf16_t*)Wc_loop, (int32_t)R, (bf16_t*)dWc, part);
    DN_CHECK_LAUNCH();
    hipLaunchKernelGGL(chain_combine_finish_kernel, dim3(kH + 1), dim3(kH), 0, st, (const double*)part, c, (const bf16_t*)W1,
                       (const bf16_t*)bias, (int32_t)R, (bf16_t*)dW1, (bf16_t*)db, (bf16_t*)db1);
    DN_CHECK_LAUNCH();
    return DN_OK;
}
