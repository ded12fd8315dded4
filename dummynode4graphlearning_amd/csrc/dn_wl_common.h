// What the graph-kernel sources (dn_wl.hip, dn_gk.hip, dn_kwl.hip, dn_k3wl.hip) share: the pairing function, the 64-bit shuffle, a
// lower bound, and the sort-and-fold of one list of unsigned 64-bit colours -- a bitonic network over the G lanes of a group or over a
// workgroup's LDS, and the fold of a sorted list of doubled entries that starts from its maximum.  Everything is force-inlined: a
// kernel that calls these compiles to what it did with the code written out in place.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef unsigned long long u64;

// Szudzik's pairing function, wrapping mod 2^64 (neither associative nor commutative: every fold over it is sequential)
__device__ __forceinline__ u64 wl_pair(u64 a, u64 b) { return a >= b ? a * a + a + b : a + b * b; }

__device__ __forceinline__ u64 shfl64(u64 v, int src) {
    const unsigned lo = (unsigned)__shfl((int)(unsigned)v, src, 64), hi = (unsigned)__shfl((int)(unsigned)(v >> 32), src, 64);
    return ((u64)hi << 32) | lo;
}

// first slot of the ascending list a[beg .. end) that holds a value >= w
template <typename K>
__device__ __forceinline__ int32_t wl_lower_bound(const K* __restrict__ a, int32_t beg, int32_t end, K w) {
    int32_t lo = beg, hi = end;
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < w) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Bitonic network of xor shuffles over the G lanes of a group (G = 8 or 64; lane: the lane of the wavefront, l: the lane of the group),
// one value per lane: lane l comes out with the l-th smallest (unsigned).  Callers pad with 2^64 - 1: a real entry of that value is
// indistinguishable from the padding, so the first cnt sorted values are the list's sorted entries either way.
template <int G>
__device__ __forceinline__ u64 wl_sort_group(u64 val, int lane, int l) {
#pragma unroll
    for (int k = 2; k <= G; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const u64 o = shfl64(val, lane ^ j);
            const bool keep_min = ((l & k) == 0) == ((l & j) == 0);
            const u64 mn = val < o ? val : o, mx = val < o ? o : val;
            val = keep_min ? mn : mx;
        }
    }
    return val;
}

// Bitonic sort of the n2 (a power of two) keys s[0 .. n2) in LDS by the BLOCK threads of a workgroup, ascending (unsigned).  The caller
// has filled s and synchronised; the sort ends synchronised.
template <int BLOCK>
__device__ __forceinline__ void wl_sort_block(u64* s, int32_t n2, int tid) {
    for (int32_t k = 2; k <= n2; k <<= 1) {
        for (int32_t j = k >> 1; j > 0; j >>= 1) {
            for (int32_t p = tid; p < (n2 >> 1); p += BLOCK) {
                const int32_t lo = ((p & ~(j - 1)) << 1) | (p & (j - 1)), hi = lo + j;
                const u64 a = s[lo], b = s[hi];
                if ((a > b) == ((lo & k) == 0)) { s[lo] = b; s[hi] = a; }
            }
            __syncthreads();
        }
    }
}

// The fold of a multiset that holds every one of cnt sorted entries TWICE (k-WL: the doubles are not sorted, the distinct list is):
// it starts from the maximum, takes every smaller entry twice in ascending order, and the maximum's second copy comes last.
//
// The lane-walk form: the entries sit sorted in the lanes base .. base + cnt - 1 of a group of G; every lane of the group walks them
// in lock-step and returns the fold.  Means nothing where cnt == 0.
template <int G>
__device__ __forceinline__ u64 wl_fold_doubled_group(u64 val, int base, int cnt) {
    const u64 top = shfl64(val, base + (cnt > 0 ? cnt - 1 : 0));
    u64 acc = top;
    for (int i = 0; i < G - 1; ++i) {
        if (G == 64 && i >= cnt - 1) break;                      // (one list per wavefront: cnt is uniform)
        const u64 e = shfl64(val, base + i);
        if (i < cnt - 1) acc = wl_pair(wl_pair(acc, e), e);
    }
    return wl_pair(acc, top);
}

// The sequential form: one thread over the sorted LDS list s[0 .. cnt), cnt >= 1.
__device__ __forceinline__ u64 wl_fold_doubled_block(const u64* s, int cnt) {
    const u64 top = s[cnt - 1];
    u64 acc = top;
    for (int i = 0; i < cnt - 1; ++i) acc = wl_pair(wl_pair(acc, s[i]), s[i]);
    return wl_pair(acc, top);
}
