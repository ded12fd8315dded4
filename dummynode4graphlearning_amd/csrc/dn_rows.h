// What the ragged-row sources (dn_seg_attn.hip, dn_diffpool.hip, dn_hgpsl.hip) share.  Each normalises rows of ragged length with one
// wavefront per short row (<= 64 keys) and one workgroup per long row (<= 1024 keys):
//   * the 64-lane reductions, the inclusive scan and the descending bitonic network of xor shuffles;
//   * the sparsemax threshold (Martins & Astudillo 2016) of a sorted row -- scan, support count, tau -- once per class: a row held one
//     key per lane, and one wavefront over a descending-sorted LDS list.  The support test is a parameter: see DnSupportAct and
//     DnSupportOps below, which are NOT interchangeable;
//   * the descending bitonic sort of float lists in LDS (wl_sort_block of dn_wl_common.h is u64 ascending and stays apart);
//   * the Jacobian line of the two score functions, and the guards of a CSR walk (clamped row range, guarded weight lookup).
// Everything is force-inlined: a kernel that calls these compiles to what it did with the code written out in place.
//
// What stays in the three files differs on purpose and is not to be merged here: the softmax arithmetic (HGP-SL adds 1e-16 to the
// denominator, DiffPool multiplies by the inverse of the sum, seg_attn divides), seg_attn's fp64 dot product and fp64 row term, the
// handling of a row without a live key and the layout of the saved statistics, and DiffPool's dp_softmax_row (up to four columns per
// lane in registers).  Each restates its own reference program bit for bit where the tests hold it to that.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

// ---- one value per lane of a wavefront
__device__ __forceinline__ float dn_wave_max(float v) {
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

template <typename T>
__device__ __forceinline__ T dn_wave_sum(T v) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// inclusive scan: lane l comes out with v_0 + ... + v_l, added in the order of an up-shuffle tree
template <typename T>
__device__ __forceinline__ T dn_wave_scan(T v, int lane) {
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

// sorted descending over the lanes (bitonic network of xor shuffles; every lane takes part)
__device__ __forceinline__ float dn_wave_sort_desc(float v, int lane) {
    for (int k = 2; k <= 64; k <<= 1)
        for (int j = k >> 1; j >= 1; j >>= 1) {
            const float u = __shfl_xor(v, j, 64);
            const bool keep_max = ((lane & k) == 0) == ((lane & j) == 0);
            v = keep_max ? fmaxf(v, u) : fminf(v, u);
        }
    return v;
}

// ---- the sparsemax support test: is the k-th largest entry s (k counted from 1, cs = the sum of the k largest) in the support?
// Two forms, equal over the reals.  In floats they round differently at the edge of the support, and each caller's tests hold its zero
// pattern to its own reference program exactly: do not unify them, and do not add a third.
struct DnSupportAct {     // subgraph_isomorphism/act.py states it as 1 + k s > cs (dn_seg_attn.hip)
    __device__ __forceinline__ bool operator()(float k, float s, float cs) const { return 1.f + k * s > cs; }
};
struct DnSupportOps {     // _sparsemax_rows of ops.py states it as k s > cs - 1 (dn_hgpsl.hip)
    __device__ __forceinline__ bool operator()(float k, float s, float cs) const { return k * s > cs - 1.f; }
};

// tau of a row of up to 64 keys.  zc = z - max on the lanes that hold a key, -inf on the others; every lane takes part and returns tau.
// (A row with a key has a support of at least one: the first sorted lane holds 0, and both tests pass there.)
template <typename Support>
__device__ __forceinline__ float dn_sparsemax_tau_wave(float zc, int lane, Support in_support) {
    const float s = dn_wave_sort_desc(zc, lane);
    const bool has = s > -INFINITY;
    const float cs = dn_wave_scan(has ? s : 0.f, lane);
    const int kk = __popcll(__ballot(has && in_support((float)(lane + 1), s, cs)));
    return (__shfl(cs, kk > 0 ? kk - 1 : 0, 64) - 1.f) / (float)(kk > 0 ? kk : 1);
}

// The maximum and tau of a row of up to 1024 keys: one wavefront over the descending-sorted LDS list s[0 .. n2), n2 a power of two
// >= 128, padded with -inf.  Lane l owns the entries l n2 / 64 ..: chunk sums, their scan, then the test entry by entry.  Every lane
// returns both.  (max == -inf: a row without a key; the sums are skipped and tau is 0.)
template <typename Support>
__device__ __forceinline__ void dn_sparsemax_tau_sorted(const float* s, int n2, int lane, Support in_support, float& max_out, float& tau_out) {
    const float m = s[0];
    const int C = n2 >> 6;
    float ls = 0.f;
    if (m > -INFINITY)
        for (int c = 0; c < C; ++c) {
            const float x = s[lane * C + c];
            if (x > -INFINITY) ls += x - m;
        }
    float cs = dn_wave_scan(ls, lane) - ls;                            // the sum of the entries before this lane's chunk
    float cnt = 0.f, ssum = 0.f;
    if (m > -INFINITY)
        for (int c = 0; c < C; ++c) {
            const float x = s[lane * C + c];
            if (x > -INFINITY) {
                const float zc = x - m;
                cs += zc;
                if (in_support((float)(lane * C + c + 1), zc, cs)) { cnt += 1.f; ssum += zc; }
            }
        }
    cnt = dn_wave_sum(cnt);
    ssum = dn_wave_sum(ssum);
    max_out = m;
    tau_out = cnt > 0.f ? (ssum - 1.f) / cnt : 0.f;
}

// Bitonic sort, descending, of `lists` lists of n2 floats each (n2 a power of two, list l at s + l n2) by the BLOCK threads of a
// workgroup, all lists in the same barrier rounds.  Pair i of list l is pair l n2 / 2 + i of the whole array: the shift that spreads
// a pair's index moves the list's bits up with it, and only the direction bit has to be masked to the list.  The caller has filled s
// and synchronised; the sort ends synchronised.
template <int BLOCK>
__device__ __forceinline__ void dn_sort_desc_lists(float* s, int lists, int n2, int tid) {
    const int half = (lists * n2) >> 1;
    for (int k = 2; k <= n2; k <<= 1) {
        const int dir = k & (n2 - 1);                                  // (the last stage, k == n2: every pair descends)
        for (int j = k >> 1; j >= 1; j >>= 1) {
            for (int i = tid; i < half; i += BLOCK) {
                const int a = ((i & ~(j - 1)) << 1) | (i & (j - 1));
                const float x = s[a], y = s[a | j];
                const bool desc = (a & dir) == 0;
                if ((x < y) == desc) { s[a] = y; s[a | j] = x; }
            }
            __syncthreads();
        }
    }
}

// dz of one entry from its weight p and diff = (gradient of p) - (the row term): softmax p diff, sparsemax diff on the support.  The
// caller forms diff in its own precision.
__device__ __forceinline__ float dn_score_dz(bool soft, float p, float diff) { return soft ? p * diff : (p > 0.f ? diff : 0.f); }

// ---- a CSR walk that stays in bounds whatever the arrays hold
__device__ __forceinline__ void dn_csr_range(const int32_t* __restrict__ ptr, int64_t row, int64_t E, int64_t& e0, int64_t& e1) {
    e0 = ptr[row];
    e1 = ptr[row + 1];
    e0 = e0 < 0 ? 0 : e0;
    e1 = e1 > E ? E : e1;
}

// the weight of CSR slot e: w[perm[e]], 0 where perm points outside the E edges; w == nullptr: every edge weighs 1
__device__ __forceinline__ float dn_edge_weight(const float* __restrict__ w, const int32_t* __restrict__ perm, int64_t e, int64_t E) {
    if (w == nullptr) return 1.f;
    const int32_t id = perm[e];
    return (id >= 0 && id < E) ? w[id] : 0.f;
}
