// Batched SMO for the C-SVC dual on precomputed kernels (graph_classification/graph_kernels/seed_svm.py: SVC(kernel="precomputed")):
// one workgroup owns one solve; docs/LAB_NOTES.md "Graph kernels: SVM evaluation", DESIGN.md "Graph kernels: SVM evaluation".
//
// The problem.  minimise 1/2 a^T Q a - sum(a) subject to 0 <= a <= C and y^T a = 0, Q_tu = y_t y_u K_tu.  With v_t = -y_t G_t (G the
// gradient), I_up = {y = +1, a < C} u {y = -1, a > 0} and I_low = {y = +1, a > 0} u {y = -1, a < C}: m = max of v over I_up,
// M = min of v over I_low, stop when m - M < eps.  The working set is libsvm's second-order rule (Fan, Chen, Lin 2005): i = the
// maximal violator of I_up, j = the t of I_low with b = m - v_t > 0 that minimises -b^2 / a_t, a_t = K_ii + K_tt - 2 K_it, replaced
// by TAU = 1e-12 when it is not positive; ties go to the lowest index.  The two-variable update, its clipping and rho (the mean of
// y G over the free vectors, else the midpoint of the bounds) are libsvm's.  No shrinking.  Everything is fp64.
//
// The launch.  A solve is a row of a table of doubles {matrix, offset, length, positives, C}: its training rows are
// rows[offset .. offset + length), the first `positives` of them the +1 class, and its kernel is K[matrix] ([n, n] of the full
// [num_matrices, n, n] array: the two kernel rows of an iteration are gathers K[matrix][rows[i]][rows[t]], nothing is copied per
// solve, and the solves of one matrix share it in L2).  The workgroup keeps a, G, the diagonal and the row list in LDS (28 bytes a
// row: kMaxRows rows).  A launch runs at most iters_per_launch iterations of every listed solve, then stores a, G, the iteration
// count, rho and a status; the host lists the solves still running and launches again.  Every loop has a trip count the host gave
// or the row count bounds; no workgroup waits for another; no atomics: the reductions run in one fixed order (shuffles inside a
// wavefront, then the four wavefronts' partial results in LDS, combined by every thread in the same order), so the result does not
// depend on how the iterations were sliced into launches and two runs give the same bits.
#include <hip/hip_runtime.h>

#include "dn_common.h"
#include "dn_hip.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxRows = 5120;           // 28 bytes a row: 140 KiB of the CU's 160 KiB of LDS
constexpr double kTau = 1e-12;
constexpr int kConverged = 0, kRunning = 1, kCapped = 2, kBadRow = 3;

struct Best {                            // the larger value wins, then the lower index
    double v;
    int32_t idx;
};

__device__ __forceinline__ Best better(Best a, Best b) { return (b.v > a.v || (b.v == a.v && b.idx < a.idx)) ? b : a; }

__device__ __forceinline__ Best wave_best(Best x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        Best o;
        o.v = __shfl_xor(x.v, d, 64);
        o.idx = __shfl_xor(x.idx, d, 64);
        x = better(x, o);
    }
    return x;
}

__device__ __forceinline__ double wave_max(double x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x = fmax(x, __shfl_xor(x, d, 64));
    return x;
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}

__device__ __forceinline__ bool as_index(double x, int64_t limit, int64_t* out) {      // an integer in [0, limit) held in a double
    if (!(x >= 0.0 && x < (double)limit)) return false;
    *out = (int64_t)x;
    return (double)*out == x;
}

__global__ __launch_bounds__(kBlock) void svm_smo_kernel(int32_t num_matrices, int32_t n, const double* __restrict__ K, int32_t num_solves,
                                                         const double* __restrict__ table, const int32_t* __restrict__ list,
                                                         int64_t num_rows, const int32_t* __restrict__ rows, int32_t max_len, double eps,
                                                         int32_t iters_per_launch, double* __restrict__ alpha_g, double* __restrict__ grad_g,
                                                         double* __restrict__ rho_g, int64_t* __restrict__ iterations,
                                                         int32_t* __restrict__ status) {
    extern __shared__ double svm_lds[];
    __shared__ Best s_i[kWaves], s_j[kWaves];
    __shared__ double s_m2[kWaves], s_sum[kWaves], s_ub[kWaves], s_lb[kWaves];
    __shared__ int32_t s_free[kWaves], s_bad[kWaves];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t s = list ? list[blockIdx.x] : (int32_t)blockIdx.x;
    if (s < 0 || s >= num_solves) return;                                    // (uniform)
    const double* row = table + (size_t)s * 5;
    int64_t mat = 0, off = 0, len = 0, npos = 0;
    const double C = row[4];
    bool ok = as_index(row[0], num_matrices, &mat) && as_index(row[1], num_rows, &off) && as_index(row[2], (int64_t)max_len + 1, &len) &&
              as_index(row[3], (int64_t)max_len + 1, &npos);
    ok = ok && len >= 1 && off + len <= num_rows && npos <= len && C > 0.0 && C < 1e300;
    if (!ok) {                                                               // (uniform: every thread read the same row)
        if (tid == 0) status[s] = kBadRow;
        return;
    }
    const int32_t l = (int32_t)len, np = (int32_t)npos;
    double* a_s = svm_lds;                                                   // [max_len] each; idx_s behind them
    double* g_s = a_s + max_len;
    double* d_s = g_s + max_len;
    int32_t* idx_s = reinterpret_cast<int32_t*>(d_s + max_len);
    const double* Km = K + (size_t)mat * n * n;
    int32_t bad = 0;
    for (int32_t t = tid; t < l; t += kBlock) {
        const int32_t r = rows[off + t];
        const bool in = r >= 0 && r < n;
        bad |= !in;
        idx_s[t] = in ? r : 0;
        a_s[t] = alpha_g[off + t];
        g_s[t] = grad_g[off + t];
        d_s[t] = in ? Km[(size_t)r * n + r] : 0.0;
    }
    bad = __any(bad) ? 1 : 0;
    if (lane == 0) s_bad[wave] = bad;
    __syncthreads();
    bad = 0;
    for (int w = 0; w < kWaves; ++w) bad |= s_bad[w];
    if (bad) {                                                               // (uniform) a row index outside the matrix: nothing is computed
        if (tid == 0) status[s] = kBadRow;
        return;
    }
    int64_t iter = iterations[s];
    const int64_t cap = l > 100000 ? (int64_t)100 * l : 10000000LL;          // libsvm: max(10^7, 100 l)
    int32_t todo = iters_per_launch;
    if ((int64_t)todo > cap - iter) todo = cap - iter > 0 ? (int32_t)(cap - iter) : 0;
    int32_t st = kRunning;
    const double ninf = -__builtin_huge_val();
    for (int32_t it = 0; it < todo; ++it) {
        // i and m over I_up, -M over I_low
        Best bi = {ninf, 0x7fffffff};
        double m2 = ninf;
        for (int32_t t = tid; t < l; t += kBlock) {
            const bool pos = t < np;
            const double a = a_s[t], v = pos ? -g_s[t] : g_s[t];
            const bool up = pos ? a < C : a > 0.0, low = pos ? a > 0.0 : a < C;
            if (up) bi = better(bi, Best{v, t});
            if (low) m2 = fmax(m2, -v);
        }
        bi = wave_best(bi);
        m2 = wave_max(m2);
        if (lane == 0) { s_i[wave] = bi; s_m2[wave] = m2; }
        __syncthreads();
        bi = s_i[0];
        m2 = s_m2[0];
        for (int w = 1; w < kWaves; ++w) { bi = better(bi, s_i[w]); m2 = fmax(m2, s_m2[w]); }
        if (bi.idx >= l || bi.v + m2 < eps) { st = kConverged; break; }       // (uniform)
        const int32_t i = bi.idx;
        const double gmax = bi.v, Kii = d_s[i];
        const double* Ki = Km + (size_t)idx_s[i] * n;
        // j: the second-order rule over the violating part of I_low
        Best bj = {ninf, 0x7fffffff};
        for (int32_t t = tid; t < l; t += kBlock) {
            const bool pos = t < np;
            const double a = a_s[t], v = pos ? -g_s[t] : g_s[t];
            const bool low = pos ? a > 0.0 : a < C;
            const double b = gmax - v;
            if (low && b > 0.0) {
                const double q = Kii + d_s[t] - 2.0 * Ki[idx_s[t]];
                bj = better(bj, Best{(b * b) / (q > 0.0 ? q : kTau), t});    // the largest b^2 / a = the smallest -b^2 / a
            }
        }
        bj = wave_best(bj);
        if (lane == 0) s_j[wave] = bj;
        __syncthreads();
        bj = s_j[0];
        for (int w = 1; w < kWaves; ++w) bj = better(bj, s_j[w]);
        if (bj.idx >= l) { st = kConverged; break; }                         // (uniform)
        const int32_t j = bj.idx;
        const double* Kj = Km + (size_t)idx_s[j] * n;
        // the two-variable update, computed by every thread alike
        const double yi = i < np ? 1.0 : -1.0, yj = j < np ? 1.0 : -1.0;
        const double Qij = yi * yj * Ki[idx_s[j]], Gi = g_s[i], Gj = g_s[j], oai = a_s[i], oaj = a_s[j];
        double ai = oai, aj = oaj;
        if (yi != yj) {
            double q = Kii + d_s[j] + 2.0 * Qij;
            if (q <= 0.0) q = kTau;
            const double delta = (-Gi - Gj) / q, diff = ai - aj;
            ai += delta;
            aj += delta;
            if (diff > 0.0) { if (aj < 0.0) { aj = 0.0; ai = diff; } }
            else { if (ai < 0.0) { ai = 0.0; aj = -diff; } }
            if (diff > 0.0) { if (ai > C) { ai = C; aj = C - diff; } }       // (C_i == C_j: libsvm's diff > C_i - C_j)
            else { if (aj > C) { aj = C; ai = C + diff; } }
        } else {
            double q = Kii + d_s[j] - 2.0 * Qij;
            if (q <= 0.0) q = kTau;
            const double delta = (Gi - Gj) / q, sum = ai + aj;
            ai -= delta;
            aj += delta;
            if (sum > C) { if (ai > C) { ai = C; aj = sum - C; } }
            else { if (aj < 0.0) { aj = 0.0; ai = sum; } }
            if (sum > C) { if (aj > C) { aj = C; ai = sum - C; } }
            else { if (ai < 0.0) { ai = 0.0; aj = sum; } }
        }
        const double dai = ai - oai, daj = aj - oaj;
        __syncthreads();                                                     // every thread has read a and G at i and j
        for (int32_t t = tid; t < l; t += kBlock) {
            const double yt = t < np ? 1.0 : -1.0;
            const int32_t c = idx_s[t];
            // libsvm's association, each product and the sum rounded on its own (no contraction: a symmetric problem stays symmetric)
            g_s[t] += __dadd_rn(__dmul_rn(yt * yi * Ki[c], dai), __dmul_rn(yt * yj * Kj[c], daj));
        }
        if (tid == 0) { a_s[i] = ai; a_s[j] = aj; }
        ++iter;
        __syncthreads();
    }
    if (st == kRunning && iter >= cap) st = kCapped;
    // rho as calculate_rho takes it, from the state as it stands (the last launch of a solve leaves the final one)
    double sum_free = 0.0, ub = __builtin_huge_val(), lb = ninf;
    int32_t nfree = 0;
    for (int32_t t = tid; t < l; t += kBlock) {
        const bool pos = t < np;
        const double a = a_s[t], yG = pos ? g_s[t] : -g_s[t];
        if (a >= C) { if (pos) lb = fmax(lb, yG); else ub = fmin(ub, yG); }
        else if (a <= 0.0) { if (pos) ub = fmin(ub, yG); else lb = fmax(lb, yG); }
        else { ++nfree; sum_free += yG; }
        alpha_g[off + t] = a;
        grad_g[off + t] = g_s[t];
    }
    sum_free = wave_sum(sum_free);
    ub = -wave_max(-ub);
    lb = wave_max(lb);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) nfree += __shfl_xor(nfree, d, 64);
    if (lane == 0) { s_sum[wave] = sum_free; s_ub[wave] = ub; s_lb[wave] = lb; s_free[wave] = nfree; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kWaves; ++w) {
            sum_free += s_sum[w];
            ub = fmin(ub, s_ub[w]);
            lb = fmax(lb, s_lb[w]);
            nfree += s_free[w];
        }
        rho_g[s] = nfree > 0 ? sum_free / nfree : (ub + lb) / 2.0;
        iterations[s] = iter;
        status[s] = st;
    }
}

}  // namespace

extern "C" {

int32_t dn_svm_max_rows(void) { return kMaxRows; }

int dn_svm_smo_f64(int64_t num_matrices, int64_t n, const double* K, int64_t num_solves, const double* table, int64_t num_list,
                   const int32_t* list, int64_t num_rows, const int32_t* rows, int32_t max_len, double eps, int32_t iters_per_launch,
                   double* alpha, double* grad, double* rho, int64_t* iterations, int32_t* status, dn_stream_t stream) {
    DN_REQUIRE(num_matrices >= 1 && n >= 1 && n <= 0x7fffffffLL && num_matrices <= 0x7fffffffLL && num_solves >= 1 &&
               num_solves <= 0x7fffffffLL && num_list >= 1 && num_list <= num_solves && num_rows >= 1,
               "dn_svm_smo: bad sizes");
    DN_REQUIRE(K && table && rows && alpha && grad && rho && iterations && status, "dn_svm_smo: NULL pointer");
    DN_REQUIRE(list || num_list == num_solves, "dn_svm_smo: NULL pointer (a solve list is needed unless it is every solve)");
    DN_REQUIRE(eps > 0.0, "dn_svm_smo: eps must be > 0 (got %g)", eps);
    DN_REQUIRE(iters_per_launch >= 1, "dn_svm_smo: iters_per_launch must be >= 1 (got %d)", iters_per_launch);
    DN_REQUIRE(max_len >= 1 && max_len <= kMaxRows && max_len <= num_rows,
               "dn_svm_smo: a row list of %d rows is outside 1 .. %d (the LDS limit) or longer than all the rows", max_len, kMaxRows);
    const size_t lds = (size_t)max_len * (3 * sizeof(double) + sizeof(int32_t));
    if (dn_allow_lds(svm_smo_kernel, lds) != DN_OK) return DN_ERR_HIP;
    hipLaunchKernelGGL(svm_smo_kernel, dim3((unsigned)num_list), dim3(kBlock), lds, (hipStream_t)stream, (int32_t)num_matrices, (int32_t)n, K,
                       (int32_t)num_solves, table, list, num_rows, rows, max_len, eps, iters_per_launch, alpha, grad, rho, iterations,
                       status);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

}  // extern "C"
