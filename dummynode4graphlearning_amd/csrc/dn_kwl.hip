// Weisfeiler-Lehman graph kernels at k = 2 (graph_classification/graph_kernels: `gram --k 2 --kernel WL | DWL | LWL | LWLC`): the
// initial colours of the node pairs ("tuples") of every graph and one refinement step per flavour, in exact 64-bit integer arithmetic
// (docs/LAB_NOTES.md "Graph kernels: 2-WL").  The tuple graph of the reference is never built: a tuple's neighbour multisets are
// gathers from its graph's own colour matrix C[a, b], selected by the dataset CSR.
//
// A tuple (v, w) has up to four multisets: type 1 exchanges the first component (colours C[x, w]), type 2 the second (C[v, x]), each
// local or global.  Every neighbour enters TWICE (the reference's undirected add_edge pushes both ends), and in WL / DWL the tuple's
// own colour enters type 1 FOUR times (DWL: the global one).  A multiset is sorted ascending (unsigned) and folded with Szudzik's
// pairing function starting from its maximum; the tuple's colour is then folded over the sorted local folds and the sorted global
// folds.  The folds are sequential (the pairing function is neither associative nor commutative): one lane walks a sorted list.
//
//   LWL / LWLC   x runs over N(v) (type 1) and N(w) (type 2); LWLC keeps only tuples (i, j) with i == j or j in N(i), found by a
//                binary search in the ascending neighbour list.  Tuples are classed by max(deg v, deg w) once per dataset:
//                <= 8: 8 lanes per tuple, <= 64: a wavefront, <= kMaxEntries: a workgroup with both lists in LDS (the dummy node's
//                pairs).  The doubles are not sorted: the distinct list is, and every element is applied twice.
//   WL / DWL     x runs over ALL nodes, so every tuple reads a whole row and a whole column of the colour matrix.  One workgroup per
//                graph: all rows are sorted ONCE in LDS with the source index next to the key, every tuple walks its sorted row
//                (skipping w; DWL routes an element to the local or global fold by an adjacency bit), then the same for the columns
//                (v itself four times).  The type-2 folds wait in a global scratch between the two phases.  9 bytes per matrix
//                element plus the bit rows: graphs of up to kMaxNodes = 128 nodes in 146 KiB + 2 KiB of the CU's 160 KiB of LDS.
//
// Integer work only, no atomics on results (one LDS counter of kept entries): two runs give the same bits.
#include <hip/hip_runtime.h>

#include "dn_common.h"
#include "dn_hip.h"
#include "dn_wl_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxNodes = 128;           // the largest graph of the WL / DWL kernel (its colour matrix and source indices in LDS)
constexpr int kMaxEntries = 1024;        // the longest list (a degree) of the LWL / LWLC workgroup kernel: 2 lists, 16 KiB of LDS

// index of tuple (a, b) in the colour array, -1 where it is no tuple (LWLC only).  row_ptr[a] is the first tuple of row a: all
// pairs: tuples of the earlier graphs + (a - first) n, connected: ptr[a] + a (a row holds a itself among its ascending neighbours)
__device__ __forceinline__ int32_t kwl_tuple(bool connected, int32_t a, int32_t b, const int32_t* __restrict__ row_ptr,
                                             const int32_t* __restrict__ node_first, const int32_t* __restrict__ ptr,
                                             const int32_t* __restrict__ nbr) {
    if (!connected) return row_ptr[a] + (b - node_first[a]);
    const int32_t beg = ptr[a], end = ptr[a + 1];
    const int32_t p = wl_lower_bound(nbr, beg, end, b);
    if (a == b) return row_ptr[a] + (p - beg);
    if (p < end && nbr[p] == b) return row_ptr[a] + (p - beg) + (b > a ? 1 : 0);
    return -1;
}

// the tuple's colour folded over its sorted local folds, then its sorted global folds
__device__ __forceinline__ u64 kwl_combine(u64 own, u64 l1, bool hl1, u64 l2, bool hl2, u64 g1, bool hg1, u64 g2, bool hg2) {
    if (hl1 && hl2 && l1 > l2) { const u64 t = l1; l1 = l2; l2 = t; }
    if (hg1 && hg2 && g1 > g2) { const u64 t = g1; g1 = g2; g2 = t; }
    u64 acc = own;
    if (hl1) acc = wl_pair(acc, l1);
    if (hl2) acc = wl_pair(acc, l2);
    if (hg1) acc = wl_pair(acc, g1);
    if (hg2) acc = wl_pair(acc, g2);
    return acc;
}

__global__ __launch_bounds__(kBlock) void kwl_init_kernel(int64_t T, const int32_t* __restrict__ tup_v, const int32_t* __restrict__ tup_w,
                                                          const int32_t* __restrict__ ptr, const int32_t* __restrict__ nbr,
                                                          const u64* __restrict__ nl, const u64* __restrict__ el, u64* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= T) return;
    const int32_t v = tup_v[t], w = tup_w[t];
    const u64 ci = nl ? wl_pair(nl[v] + 1ull, 1ull) : 1ull, cj = nl ? wl_pair(nl[w] + 1ull, 2ull) : 2ull;
    const int32_t end = ptr[v + 1];
    const int32_t p = wl_lower_bound(nbr, ptr[v], end, w);
    u64 c = v == w ? 1ull : 2ull;
    if (p < end && nbr[p] == w) c = el ? wl_pair(3ull, el[p]) : 3ull;
    out[t] = wl_pair(wl_pair(ci, cj), c);
}

// entry k of list L of tuple (v, w): L = 0: C[x, w] for x = the k-th neighbour of v; L = 1: C[v, x] for x = the k-th neighbour of w
__device__ __forceinline__ bool kwl_local_entry(int L, int32_t k, int32_t v, int32_t w, bool connected, const int32_t* __restrict__ row_ptr,
                                                const int32_t* __restrict__ node_first, const int32_t* __restrict__ ptr,
                                                const int32_t* __restrict__ nbr, const u64* __restrict__ cin, u64* val) {
    const int32_t x = nbr[ptr[L ? w : v] + k];
    const int32_t idx = L ? kwl_tuple(connected, v, x, row_ptr, node_first, ptr, nbr) : kwl_tuple(connected, x, w, row_ptr, node_first, ptr, nbr);
    if (idx < 0) return false;
    *val = cin[idx];
    return true;
}

// G lanes per tuple (G = 8 or 64), one entry per lane, the two lists one after the other through the same shuffle network
// (dn_wl_common.h: wl_sort_group and the padding, wl_fold_doubled_group).
template <int G>
__global__ __launch_bounds__(kBlock) void kwl_local_group_kernel(int64_t num, const int32_t* __restrict__ list, int connected,
                                                                 const int32_t* __restrict__ tup_v, const int32_t* __restrict__ tup_w,
                                                                 const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ node_first,
                                                                 const int32_t* __restrict__ ptr, const int32_t* __restrict__ nbr,
                                                                 const u64* __restrict__ cin, u64* __restrict__ cout) {
    const int64_t gi = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / G;
    const int lane = (int)(threadIdx.x & 63), l = lane & (G - 1), base = lane & ~(G - 1);
    bool active = gi < num;
    int32_t t = 0, v = 0, w = 0, deg[2] = {0, 0};
    if (active) {
        t = list ? list[gi] : (int32_t)gi;
        v = tup_v[t];
        w = tup_w[t];
        deg[0] = ptr[v + 1] - ptr[v];
        deg[1] = ptr[w + 1] - ptr[w];
        active = deg[0] >= 0 && deg[1] >= 0 && deg[0] <= G && deg[1] <= G;      // a tuple of another class is left alone
    }
    u64 fold[2] = {0ull, 0ull};
    bool has[2] = {false, false};
#pragma unroll
    for (int L = 0; L < 2; ++L) {
        u64 val = ~0ull;
        bool kept = false;
        if (active && l < deg[L]) kept = kwl_local_entry(L, l, v, w, connected != 0, row_ptr, node_first, ptr, nbr, cin, &val);
        if (!kept) val = ~0ull;
        const u64 ballot = __ballot(kept);
        const int cnt = G == 64 ? __popcll(ballot) : __popcll((ballot >> base) & ((1ull << (G & 63)) - 1ull));
        val = wl_sort_group<G>(val, lane, l);
        fold[L] = wl_fold_doubled_group<G>(val, base, cnt);
        has[L] = cnt > 0;
    }
    if (active && l == 0) cout[t] = kwl_combine(cin[t], fold[0], has[0], fold[1], has[1], 0ull, false, 0ull, false);
}

// one workgroup per tuple: both lists in LDS (cap entries each, a power of two), bitonic sort of the next power of two >= the degree
__global__ __launch_bounds__(kBlock) void kwl_local_block_kernel(const int32_t* __restrict__ list, int32_t cap, int connected,
                                                                 const int32_t* __restrict__ tup_v, const int32_t* __restrict__ tup_w,
                                                                 const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ node_first,
                                                                 const int32_t* __restrict__ ptr, const int32_t* __restrict__ nbr,
                                                                 const u64* __restrict__ cin, u64* __restrict__ cout) {
    extern __shared__ u64 kwl_s[];
    __shared__ int kept_s[2];
    __shared__ u64 fold_s[2];
    const int tid = (int)threadIdx.x;
    const int32_t t = list ? list[blockIdx.x] : (int32_t)blockIdx.x;
    const int32_t v = tup_v[t], w = tup_w[t];
    const int32_t deg[2] = {ptr[v + 1] - ptr[v], ptr[w + 1] - ptr[w]};
    if (deg[0] < 0 || deg[1] < 0 || deg[0] > cap || deg[1] > cap) return;       // (uniform) a list longer than the launch's LDS
    if (tid < 2) kept_s[tid] = 0;
    __syncthreads();
    for (int L = 0; L < 2; ++L) {
        u64* s = kwl_s + (size_t)L * cap;
        int32_t n2 = 1;
        while (n2 < deg[L]) n2 <<= 1;
        int mine = 0;
        for (int32_t k = tid; k < n2; k += kBlock) {
            u64 val = ~0ull;
            if (k < deg[L] && kwl_local_entry(L, k, v, w, connected != 0, row_ptr, node_first, ptr, nbr, cin, &val)) ++mine;
            else val = ~0ull;
            s[k] = val;
        }
        if (mine) atomicAdd(&kept_s[L], mine);                   // a count, whatever the order of the additions
        __syncthreads();
        wl_sort_block<kBlock>(s, n2, tid);
    }
    if (tid == 0 || tid == 64) {                                 // one lane of two wavefronts: a list each
        const int L = tid >> 6;
        if (kept_s[L] > 0) fold_s[L] = wl_fold_doubled_block(kwl_s + (size_t)L * cap, kept_s[L]);
    }
    __syncthreads();
    if (tid == 0) cout[t] = kwl_combine(cin[t], fold_s[0], kept_s[0] > 0, fold_s[1], kept_s[1] > 0, 0ull, false, 0ull, false);
}

// bitonic sort of L lists of n2 (a power of two) (key, source) pairs each, ascending by key, then by source (padding: key 2^64 - 1,
// source 255, so it ends behind a real entry of that value).  Element i of list l sits at l lstride + i estride.  BYLIST: consecutive
// threads take the same step of consecutive lists (the column phase: consecutive addresses).
template <bool BYLIST>
__device__ __forceinline__ void kwl_sort_lists(u64* __restrict__ K, uint8_t* __restrict__ S, int L, int n2, int lstride, int estride) {
    const int half = n2 >> 1, total = L * half;
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = (int)threadIdx.x; p < total; p += (int)blockDim.x) {
                const int l = BYLIST ? p % L : p / half, tt = BYLIST ? p / L : p % half;
                const int lo = ((tt & ~(j - 1)) << 1) | (tt & (j - 1)), hi = lo + j;
                const int ia = l * lstride + lo * estride, ib = l * lstride + hi * estride;
                const u64 a = K[ia], b = K[ib];
                const uint8_t sa = S[ia], sb = S[ib];
                const bool gt = a > b || (a == b && sa > sb);
                if (gt == ((lo & k) == 0)) { K[ia] = b; K[ib] = a; S[ia] = sb; S[ib] = sa; }
            }
            __syncthreads();
        }
    }
}

// The folds of one sorted list of n (key, source) pairs, element i at off + i es, for the tuple whose exchanged component is `self`.
// SKIP (type 2, the row walk): the element that came from `self` is left out.  !SKIP (type 1, the column walk): it counts four times
// and is global.  Every other element counts twice; malkin: it is local where bit (self, source) of the adjacency rows is set,
// global elsewhere; else everything is local.  A fold starts from the LAST element of its class, whose remaining copies come last.
template <bool SKIP>
__device__ __forceinline__ void kwl_walk(const u64* __restrict__ K, const uint8_t* __restrict__ S, const uint32_t* __restrict__ bits,
                                         bool malkin, int n, int off, int es, int self, u64& f_loc, bool& h_loc, u64& f_glo, bool& h_glo) {
    const uint32_t b0 = malkin ? bits[self * 4] : 0u, b1 = malkin ? bits[self * 4 + 1] : 0u, b2 = malkin ? bits[self * 4 + 2] : 0u,
                   b3 = malkin ? bits[self * 4 + 3] : 0u;
    auto global_of = [&](int s) -> bool {
        if (!malkin) return false;
        if (s == self) return true;
        const uint32_t wd = (s >> 5) == 0 ? b0 : (s >> 5) == 1 ? b1 : (s >> 5) == 2 ? b2 : b3;
        return ((wd >> (s & 31)) & 1u) == 0u;
    };
    int m_loc = -1, m_glo = -1;
    for (int i = n - 1; i >= 0; --i) {
        const int s = S[off + i * es];
        if (SKIP && s == self) continue;
        if (global_of(s)) { if (m_glo < 0) m_glo = i; }
        else if (m_loc < 0) m_loc = i;
        if (m_loc >= 0 && (m_glo >= 0 || !malkin)) break;
    }
    u64 a_loc = m_loc >= 0 ? K[off + m_loc * es] : 0ull, a_glo = m_glo >= 0 ? K[off + m_glo * es] : 0ull;
    for (int i = 0; i < n; ++i) {
        const int s = S[off + i * es];
        if (SKIP && s == self) continue;
        const u64 k = K[off + i * es];
        const bool g = global_of(s);
        int m = (!SKIP && s == self) ? 4 : 2;
        if (i == (g ? m_glo : m_loc)) --m;                       // one copy of the class's maximum started the fold
        u64 acc = g ? a_glo : a_loc;
        acc = wl_pair(acc, k);
        if (m > 1) acc = wl_pair(acc, k);
        if (m > 2) acc = wl_pair(acc, k);
        if (m > 3) acc = wl_pair(acc, k);
        if (g) a_glo = acc;
        else a_loc = acc;
    }
    f_loc = a_loc; h_loc = m_loc >= 0;
    f_glo = a_glo; h_glo = m_glo >= 0;
}

// WL / DWL: one workgroup per graph of at most lds_nodes nodes.  LDS: keys [n2 n2] u64, adjacency rows [n2][4] u32, sources [n2 n2]
// u8 (n2 = the launch's lds_nodes, a power of two <= 128; rows and columns are sorted at the graph's own power of two).
__global__ __launch_bounds__(1024) void kwl_global_kernel(const int32_t* __restrict__ graphs, int32_t lds_nodes, int malkin,
                                                          const int32_t* __restrict__ node_ptr, const int32_t* __restrict__ tuple_ptr,
                                                          const int32_t* __restrict__ ptr, const int32_t* __restrict__ nbr,
                                                          const u64* __restrict__ cin, u64* __restrict__ cout, u64* __restrict__ work,
                                                          int64_t T) {
    extern __shared__ u64 kwl_m[];
    const int32_t g = graphs[blockIdx.x];
    const int32_t base = node_ptr[g], n = node_ptr[g + 1] - base, t0 = tuple_ptr[g];
    if (n < 1 || n > lds_nodes || tuple_ptr[g + 1] - t0 != n * n) return;        // (uniform) a graph of another class is left alone
    int n2 = 1;
    while (n2 < n) n2 <<= 1;
    u64* K = kwl_m;
    uint32_t* bits = reinterpret_cast<uint32_t*>(kwl_m + (size_t)lds_nodes * lds_nodes);
    uint8_t* S = reinterpret_cast<uint8_t*>(bits + (size_t)lds_nodes * 4);
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x, nn = n * n;
    if (malkin) {
        for (int a = tid; a < n; a += nt) {                      // a thread writes the four words of its own node: no atomics
            u64 lo = 0ull, hi = 0ull;
            for (int32_t e = ptr[base + a]; e < ptr[base + a + 1]; ++e) {
                const int32_t b = nbr[e] - base;
                if (b >= 0 && b < 64) lo |= 1ull << b;
                else if (b >= 64 && b < n) hi |= 1ull << (b - 64);
            }
            bits[a * 4] = (uint32_t)lo; bits[a * 4 + 1] = (uint32_t)(lo >> 32);
            bits[a * 4 + 2] = (uint32_t)hi; bits[a * 4 + 3] = (uint32_t)(hi >> 32);
        }
    }
    // ---- rows: type 2, C[v, x] for x != w
    for (int p = tid; p < n * n2; p += nt) {
        const int a = p / n2, i = p % n2;
        K[p] = i < n ? cin[t0 + a * n + i] : ~0ull;
        S[p] = (uint8_t)(i < n ? i : 255);
    }
    __syncthreads();
    kwl_sort_lists<false>(K, S, n, n2, n2, 1);
    for (int t = tid; t < nn; t += nt) {
        const int v = t / n, w = t % n;
        u64 fl, fg;
        bool hl, hg;
        kwl_walk<true>(K, S, bits, malkin != 0, n, v * n2, 1, w, fl, hl, fg, hg);
        work[t0 + t] = fl;
        if (malkin) work[T + t0 + t] = fg;
    }
    __syncthreads();
    // ---- columns: type 1, C[x, w] for x != v and the tuple itself four times
    for (int p = tid; p < n2 * n; p += nt) {
        const int i = p / n;
        K[p] = i < n ? cin[t0 + p] : ~0ull;
        S[p] = (uint8_t)(i < n ? i : 255);
    }
    __syncthreads();
    kwl_sort_lists<true>(K, S, n, n2, 1, n);
    for (int t = tid; t < nn; t += nt) {                         // (the thread that wrote work[t0 + t] reads it back)
        const int v = t / n, w = t % n;
        u64 fl, fg;
        bool hl, hg;
        kwl_walk<false>(K, S, bits, malkin != 0, n, w, n, v, fl, hl, fg, hg);
        int degw = 0;
        if (malkin) degw = __popc(bits[w * 4]) + __popc(bits[w * 4 + 1]) + __popc(bits[w * 4 + 2]) + __popc(bits[w * 4 + 3]);
        const bool hl2 = malkin ? degw > 0 : n > 1, hg2 = malkin ? n - 1 - degw > 0 : false;
        const u64 l2 = work[t0 + t], g2 = malkin ? work[T + t0 + t] : 0ull;
        cout[t0 + t] = kwl_combine(cin[t0 + t], fl, hl, l2, hl2, fg, hg, g2, hg2);
    }
}

bool fits_i32(int64_t v) { return v > 0 && v <= 0x7fffffffLL; }

}  // namespace

extern "C" {

int32_t dn_kwl_max_nodes(void) { return kMaxNodes; }
int32_t dn_kwl_max_entries(void) { return kMaxEntries; }

int dn_kwl_init_u64(int64_t num_nodes, int64_t num_tuples, const int32_t* tup_v, const int32_t* tup_w, const int32_t* ptr, const int32_t* nbr,
                    const int64_t* node_label, const int64_t* edge_label, int64_t* colors_out, dn_stream_t stream) {
    DN_REQUIRE(fits_i32(num_nodes) && fits_i32(num_tuples), "dn_kwl_init: bad sizes");
    DN_REQUIRE(tup_v && tup_w && ptr && nbr && colors_out, "dn_kwl_init: NULL pointer");   // (labels may be NULL: not used)
    hipLaunchKernelGGL(kwl_init_kernel, dim3((unsigned)dn_cdiv(num_tuples, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, num_tuples, tup_v,
                       tup_w, ptr, nbr, reinterpret_cast<const u64*>(node_label), reinterpret_cast<const u64*>(edge_label),
                       reinterpret_cast<u64*>(colors_out));
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_kwl_local_u64(int64_t num_nodes, int64_t num_tuples, int64_t num_list, const int32_t* tuples, int32_t group, int32_t lds_entries,
                     int32_t connected, const int32_t* tup_v, const int32_t* tup_w, const int32_t* row_ptr, const int32_t* node_first,
                     const int32_t* ptr, const int32_t* nbr, const int64_t* colors_in, int64_t* colors_out, dn_stream_t stream) {
    DN_REQUIRE(fits_i32(num_nodes) && fits_i32(num_tuples) && fits_i32(num_list) && num_list <= num_tuples, "dn_kwl_local: bad sizes");
    DN_REQUIRE(group == 8 || group == 64 || group == 0, "dn_kwl_local: group must be 8, 64 or 0 (a workgroup per tuple), got %d", group);
    DN_REQUIRE(tup_v && tup_w && row_ptr && node_first && ptr && nbr && colors_in && colors_out, "dn_kwl_local: NULL pointer");
    DN_REQUIRE(tuples || num_list == num_tuples, "dn_kwl_local: NULL pointer (a tuple list is needed unless it is every tuple)");
    DN_REQUIRE(colors_in != colors_out, "dn_kwl_local: colors_out must not alias colors_in");
    const u64* cin = reinterpret_cast<const u64*>(colors_in);
    u64* cout = reinterpret_cast<u64*>(colors_out);
    hipStream_t st = (hipStream_t)stream;
    if (group == 0) {
        DN_REQUIRE(lds_entries >= 1 && lds_entries <= kMaxEntries && (lds_entries & (lds_entries - 1)) == 0,
                   "dn_kwl_local: lds_entries must be a power of two <= %d (got %d)", kMaxEntries, lds_entries);
        const size_t lds = (size_t)2 * lds_entries * sizeof(u64);
        hipLaunchKernelGGL(kwl_local_block_kernel, dim3((unsigned)num_list), dim3(kBlock), lds, st, tuples,
                           lds_entries, (int)connected, tup_v, tup_w, row_ptr, node_first, ptr, nbr, cin, cout);
    } else {
        const int64_t blocks = dn_cdiv(num_list * group, kBlock);
        DN_REQUIRE(blocks <= 0x7fffffffLL, "dn_kwl_local: bad sizes");
        if (group == 8)
            hipLaunchKernelGGL(kwl_local_group_kernel<8>, dim3((unsigned)blocks), dim3(kBlock), 0, st, num_list, tuples, (int)connected, tup_v,
                               tup_w, row_ptr, node_first, ptr, nbr, cin, cout);
        else
            hipLaunchKernelGGL(kwl_local_group_kernel<64>, dim3((unsigned)blocks), dim3(kBlock), 0, st, num_list, tuples, (int)connected, tup_v,
                               tup_w, row_ptr, node_first, ptr, nbr, cin, cout);
    }
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_kwl_global_u64(int64_t num_graphs, int64_t num_tuples, int64_t num_list, const int32_t* graphs, int32_t lds_nodes, int32_t malkin,
                      const int32_t* node_ptr, const int32_t* tuple_ptr, const int32_t* ptr, const int32_t* nbr, const int64_t* colors_in,
                      int64_t* colors_out, int64_t* work, dn_stream_t stream) {
    DN_REQUIRE(fits_i32(num_graphs) && fits_i32(num_tuples) && fits_i32(num_list) && num_list <= num_graphs, "dn_kwl_global: bad sizes");
    DN_REQUIRE(lds_nodes >= 1 && lds_nodes <= kMaxNodes && (lds_nodes & (lds_nodes - 1)) == 0,
               "dn_kwl_global: lds_nodes must be a power of two <= %d (got %d)", kMaxNodes, lds_nodes);
    DN_REQUIRE(graphs && node_ptr && tuple_ptr && ptr && nbr && colors_in && colors_out && work, "dn_kwl_global: NULL pointer");
    DN_REQUIRE(colors_in != colors_out && work != colors_in && work != colors_out, "dn_kwl_global: colors_out and work must not alias");
    const size_t cells = (size_t)lds_nodes * lds_nodes;
    const size_t lds = cells * (sizeof(u64) + 1) + (size_t)lds_nodes * 4 * sizeof(uint32_t);
    const int threads = lds_nodes <= 16 ? 64 : lds_nodes == 32 ? 256 : lds_nodes == 64 ? 512 : 1024;
    if (int rc = dn_allow_lds(kwl_global_kernel, lds)) return rc;
    hipLaunchKernelGGL(kwl_global_kernel, dim3((unsigned)num_list), dim3(threads), lds, (hipStream_t)stream, graphs, lds_nodes, (int)malkin,
                       node_ptr, tuple_ptr, ptr, nbr, reinterpret_cast<const u64*>(colors_in), reinterpret_cast<u64*>(colors_out),
                       reinterpret_cast<u64*>(work), num_tuples);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

}  // extern "C"
