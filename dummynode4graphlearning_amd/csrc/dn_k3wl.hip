// Weisfeiler-Lehman graph kernels at k = 3 (graph_classification/graph_kernels: `gram --k 3 --kernel WL | DWL | LWL | LWLC`): the
// initial colours of the node triples of every graph and one refinement step per flavour, in exact 64-bit integer arithmetic
// (docs/LAB_NOTES.md "Graph kernels: 3-WL").  The tuple graph of the reference is never built: a triple's neighbour multisets are
// gathers from its graph's own colour cube C[a, b, c], selected by the dataset CSR.
//
// A triple (v, w, u) has up to six multisets: exchange 1 replaces the first component (colours C[x, w, u]), exchange 2 the second
// (C[v, x, u]), exchange 3 the third (C[v, w, x]), each local or global.  Every neighbour enters TWICE (the reference's undirected
// add_edge pushes both ends), and in WL / DWL the triple's own colour enters multiset 1 SIX times (DWL: the global one).  A multiset is
// sorted ascending (unsigned) and folded with Szudzik's pairing function starting from its maximum; the triple's colour is then folded
// over the sorted local folds and the sorted global folds.  The folds are sequential: one lane walks a sorted list.
//
//   LWL / LWLC   x runs over the neighbours of the exchanged node.  LWLC keeps only the items (i, i, i), (i, i, j) with j in N(i) and
//                pairwise distinct (i, j, k) with two adjacent pairs, found by binary search in the graph's ascending item keys
//                ((i n + j) n + k); its exchanges 1 and 2 share ONE multiset.  Triples are classed by their longest list once per
//                dataset: <= 8: 8 lanes per triple, <= 64: a wavefront, else a workgroup with the lists in LDS.  The doubles are not
//                sorted: the distinct list is, and every element is applied twice.
//   WL / DWL     x runs over ALL nodes: a fibre of the cube (n colours along one axis) is the multiset source of all n triples on it.
//                A group of G = 8 .. 64 lanes per fibre (graphs of up to kMaxNodes = 64 nodes): one colour per lane, (key, source)
//                sorted once in the group, then all lanes walk the sorted fibre in lock-step -- the element at a sorted position is a
//                broadcast -- each skipping its own entry (axis 1: counting it six times) and DWL routing an element by one bit test
//                against the lane's own 64-bit adjacency row.  The per-axis folds wait in a work buffer for the closing launch.
//
// Integer work only, no atomics on results (one LDS counter of kept entries): two runs give the same bits.
#include <hip/hip_runtime.h>

#include "dn_common.h"
#include "dn_hip.h"
#include "dn_wl_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxNodes = 64;            // the largest graph of the WL / DWL kernel (a fibre in one wavefront, an adjacency row in 64 bits)
constexpr int kMaxEntries = 256;         // the largest degree of the LWL / LWLC workgroup kernel: lists of up to 2 kMaxEntries (LWLC's
                                         // merged one), three of them: 12 KiB of LDS

// is w in the ascending list nbr[ptr[v] .. ptr[v + 1])?
__device__ __forceinline__ bool k3_adjacent(const int32_t* __restrict__ ptr, const int32_t* __restrict__ nbr, int32_t v, int32_t w) {
    const int32_t end = ptr[v + 1];
    const int32_t lo = wl_lower_bound(nbr, ptr[v], end, w);
    return lo < end && nbr[lo] == w;
}

// slot of triple (a, b, c) (nodes of one graph) in the colour array, -1 where it is no item (LWLC only)
__device__ __forceinline__ int32_t k3_slot(bool connected, int32_t a, int32_t b, int32_t c, const int32_t* __restrict__ node_graph,
                                           const int32_t* __restrict__ node_ptr, const int32_t* __restrict__ tuple_ptr,
                                           const int64_t* __restrict__ item_key, const int32_t* __restrict__ item_slot) {
    const int32_t g = node_graph[a];
    const int32_t first = node_ptr[g];
    const int64_t n = node_ptr[g + 1] - first;
    const int64_t key = ((int64_t)(a - first) * n + (b - first)) * n + (c - first);
    const int32_t t0 = tuple_ptr[g];
    if (!connected) return (int32_t)(t0 + key);
    const int32_t end = tuple_ptr[g + 1];
    const int32_t lo = wl_lower_bound(item_key, t0, end, key);
    return lo < end && item_key[lo] == key ? item_slot[lo] : -1;
}

// three folds, present before absent and ascending among the present: three compare-exchanges
__device__ __forceinline__ void k3_sort3(u64* f, bool* h) {
    auto cx = [&](int a, int b) {
        const bool swap = (!h[a] && h[b]) || (h[a] && h[b] && f[a] > f[b]);
        if (swap) { const u64 t = f[a]; f[a] = f[b]; f[b] = t; const bool q = h[a]; h[a] = h[b]; h[b] = q; }
    };
    cx(0, 1); cx(1, 2); cx(0, 1);
}

// the triple's colour folded over its sorted local folds, then its sorted global folds (absent ones left out)
__device__ __forceinline__ u64 k3_combine(u64 own, u64* fl, bool* hl, u64* fg, bool* hg) {
    k3_sort3(fl, hl);
    k3_sort3(fg, hg);
    u64 acc = own;
#pragma unroll
    for (int i = 0; i < 3; ++i) if (hl[i]) acc = wl_pair(acc, fl[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) if (hg[i]) acc = wl_pair(acc, fg[i]);
    return acc;
}

__global__ __launch_bounds__(kBlock) void k3_init_kernel(int64_t T, int connected, const int32_t* __restrict__ tup_v,
                                                         const int32_t* __restrict__ tup_w, const int32_t* __restrict__ tup_u,
                                                         const int32_t* __restrict__ ptr, const int32_t* __restrict__ nbr,
                                                         const u64* __restrict__ nl, u64* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= T) return;
    const int32_t v = tup_v[t], w = tup_w[t], u = tup_u[t];
    const u64 ci = nl ? wl_pair(nl[v] + 1ull, 1ull) : 1ull, cj = nl ? wl_pair(nl[w] + 1ull, 2ull) : 2ull,
              ck = nl ? wl_pair(nl[u] + 1ull, 3ull) : 3ull;
    // all triples: 1 adjacent, 2 not (a repeated node is not adjacent); LWLC: 3 adjacent, 1 the same node, 2 neither -- which gives
    // (1, 1, 1) for (i, i, i) and (1, 3, 3) for (i, i, j)
    auto code = [&](int32_t a, int32_t b) -> u64 {
        const bool adj = a != b && k3_adjacent(ptr, nbr, a, b);
        if (!connected) return adj ? 1ull : 2ull;
        return adj ? 3ull : a == b ? 1ull : 2ull;
    };
    const u64 a = code(v, w), b = code(v, u), c = code(w, u);
    out[t] = wl_pair(wl_pair(wl_pair(a, b), c), wl_pair(wl_pair(ci, cj), ck));
}

struct K3Local {
    int connected;
    const int32_t *tup_v, *tup_w, *tup_u, *node_graph, *node_ptr, *tuple_ptr, *ptr, *nbr, *item_slot;
    const int64_t* item_key;
};

// the lengths of the three lists of triple (v, w, u): LWL: an exchange each; LWLC: exchanges 1 and 2 together, exchange 3, none
__device__ __forceinline__ void k3_lengths(const K3Local& a, int32_t v, int32_t w, int32_t u, int32_t* len) {
    const int32_t dv = a.ptr[v + 1] - a.ptr[v], dw = a.ptr[w + 1] - a.ptr[w], du = a.ptr[u + 1] - a.ptr[u];
    if (a.connected) { len[0] = dv + dw; len[1] = du; len[2] = 0; }
    else { len[0] = dv; len[1] = dw; len[2] = du; }
}

// entry k of list m of triple (v, w, u); false where the neighbour triple is no item
__device__ __forceinline__ bool k3_entry(const K3Local& a, int m, int32_t k, int32_t v, int32_t w, int32_t u, const u64* __restrict__ cin,
                                         u64* val) {
    int ex = m;                                                   // the exchanged component
    if (a.connected) {
        const int32_t dv = a.ptr[v + 1] - a.ptr[v];
        if (m == 0) { ex = k < dv ? 0 : 1; if (ex) k -= dv; }
        else ex = 2;
    }
    const int32_t x = a.nbr[a.ptr[ex == 0 ? v : ex == 1 ? w : u] + k];
    const int32_t idx = k3_slot(a.connected != 0, ex == 0 ? x : v, ex == 1 ? x : w, ex == 2 ? x : u, a.node_graph, a.node_ptr, a.tuple_ptr,
                                a.item_key, a.item_slot);
    if (idx < 0) return false;
    *val = cin[idx];
    return true;
}

// G lanes per triple (G = 8 or 64), one entry per lane, the three lists one after the other through the same shuffle network
// (dn_wl_common.h: wl_sort_group and the padding, wl_fold_doubled_group).
template <int G>
__global__ __launch_bounds__(kBlock) void k3_local_group_kernel(int64_t num, const int32_t* __restrict__ list, K3Local a,
                                                                const u64* __restrict__ cin, u64* __restrict__ cout) {
    const int64_t gi = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / G;
    const int lane = (int)(threadIdx.x & 63), l = lane & (G - 1), base = lane & ~(G - 1);
    bool active = gi < num;
    int32_t t = 0, v = 0, w = 0, u = 0, len[3] = {0, 0, 0};
    if (active) {
        t = list ? list[gi] : (int32_t)gi;
        v = a.tup_v[t];
        w = a.tup_w[t];
        u = a.tup_u[t];
        k3_lengths(a, v, w, u, len);
        active = len[0] >= 0 && len[1] >= 0 && len[2] >= 0 && len[0] <= G && len[1] <= G && len[2] <= G;   // another class: left alone
    }
    u64 fold[3] = {0ull, 0ull, 0ull}, none[3] = {0ull, 0ull, 0ull};
    bool has[3] = {false, false, false}, no[3] = {false, false, false};
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        u64 val = ~0ull;
        bool kept = false;
        if (active && l < len[m]) kept = k3_entry(a, m, l, v, w, u, cin, &val);
        if (!kept) val = ~0ull;
        const u64 ballot = __ballot(kept);
        const int cnt = G == 64 ? __popcll(ballot) : __popcll((ballot >> base) & ((1ull << (G & 63)) - 1ull));
        val = wl_sort_group<G>(val, lane, l);
        fold[m] = wl_fold_doubled_group<G>(val, base, cnt);
        has[m] = cnt > 0;
    }
    if (active && l == 0) cout[t] = k3_combine(cin[t], fold, has, none, no);
}

// one workgroup per triple: the three lists in LDS (cap entries each, a power of two), bitonic sort of the next power of two >= the
// list's length
__global__ __launch_bounds__(kBlock) void k3_local_block_kernel(const int32_t* __restrict__ list, int32_t cap, K3Local a,
                                                                const u64* __restrict__ cin, u64* __restrict__ cout) {
    extern __shared__ u64 k3_s[];
    __shared__ int kept_s[3];
    __shared__ u64 fold_s[3];
    const int tid = (int)threadIdx.x;
    const int32_t t = list ? list[blockIdx.x] : (int32_t)blockIdx.x;
    const int32_t v = a.tup_v[t], w = a.tup_w[t], u = a.tup_u[t];
    int32_t len[3];
    k3_lengths(a, v, w, u, len);
    if (len[0] < 0 || len[1] < 0 || len[2] < 0 || len[0] > cap || len[1] > cap || len[2] > cap) return;   // (uniform) longer than the LDS
    if (tid < 3) kept_s[tid] = 0;
    __syncthreads();
    for (int m = 0; m < 3; ++m) {
        u64* s = k3_s + (size_t)m * cap;
        int32_t n2 = 1;
        while (n2 < len[m]) n2 <<= 1;
        int mine = 0;
        for (int32_t k = tid; k < n2; k += kBlock) {
            u64 val = ~0ull;
            if (k < len[m] && k3_entry(a, m, k, v, w, u, cin, &val)) ++mine;
            else val = ~0ull;
            s[k] = val;
        }
        if (mine) atomicAdd(&kept_s[m], mine);                   // a count, whatever the order of the additions
        __syncthreads();
        wl_sort_block<kBlock>(s, n2, tid);
    }
    if (tid == 0 || tid == 64 || tid == 128) {                   // one lane of three wavefronts: a list each
        const int m = tid >> 6;
        if (kept_s[m] > 0) fold_s[m] = wl_fold_doubled_block(k3_s + (size_t)m * cap, kept_s[m]);
    }
    __syncthreads();
    if (tid == 0) {
        u64 fold[3] = {fold_s[0], fold_s[1], fold_s[2]}, none[3] = {0ull, 0ull, 0ull};
        bool has[3] = {kept_s[0] > 0, kept_s[1] > 0, kept_s[2] > 0}, no[3] = {false, false, false};
        cout[t] = k3_combine(cin[t], fold, has, none, no);
    }
}

// WL / DWL, the fibre pass: G lanes per fibre of a graph of at most G nodes.  fib_ptr[q] is the first fibre of graphs[q] (3 n^2 each:
// axis 0 exchanges the first component, stride n^2; axis 1 the second, stride n; axis 2 the third, stride 1).  Lane l stands for the
// triple whose exchanged component is node l.  work[(3 c + axis) T + t]: the fold of class c (0 local, 1 global; WL: local only).
template <int G>
__global__ __launch_bounds__(kBlock) void k3_fibre_kernel(int64_t num_fibres, int32_t num_list, const int32_t* __restrict__ graphs,
                                                          const int32_t* __restrict__ fib_ptr, int malkin,
                                                          const int32_t* __restrict__ node_ptr, const int32_t* __restrict__ tuple_ptr,
                                                          const u64* __restrict__ adj_bits, const u64* __restrict__ cin,
                                                          u64* __restrict__ work, int64_t T) {
    const int64_t gi = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / G;
    const int lane = (int)(threadIdx.x & 63), l = lane & (G - 1), base = lane & ~(G - 1);
    bool active = gi < num_fibres;
    int32_t n = 0, axis = 0;
    int64_t t_mine = 0;
    u64 key = ~0ull, bits = 0ull;
    if (active) {
        int32_t lo = 0, hi = num_list;                            // the last q with fib_ptr[q] <= gi
        while (hi - lo > 1) {
            const int32_t mid = lo + ((hi - lo) >> 1);
            if ((int64_t)fib_ptr[mid] <= gi) lo = mid;
            else hi = mid;
        }
        const int32_t g = graphs[lo];
        const int32_t first = node_ptr[g], t0 = tuple_ptr[g];
        n = node_ptr[g + 1] - first;
        const int32_t f = (int32_t)(gi - fib_ptr[lo]), nn = n * n;
        active = n >= 1 && n <= G && tuple_ptr[g + 1] - t0 == nn * n && f < 3 * nn;      // a graph of another class is left alone
        if (active) {
            axis = f / nn;
            const int32_t r = f - axis * nn, p = r / n, s = r - p * n;
            const int32_t start = axis == 0 ? p * n + s : axis == 1 ? p * nn + s : p * nn + s * n;
            const int32_t stride = axis == 0 ? nn : axis == 1 ? n : 1;
            if (l < n) {
                t_mine = (int64_t)t0 + start + (int64_t)l * stride;
                key = cin[t_mine];
                if (malkin) bits = adj_bits[first + l];
            }
        }
    }
    if (!active) n = 0;
    int src = l < n ? l : 255;
    // ascending by (key, source): padding (2^64 - 1, 255) ends behind a real entry of that value
#pragma unroll
    for (int k = 2; k <= G; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const u64 o = shfl64(key, lane ^ j);
            const int os = __shfl(src, lane ^ j, 64);
            const bool keep_min = ((l & k) == 0) == ((l & j) == 0);
            const bool less = key < o || (key == o && src < os);
            const bool take = keep_min != less;                  // keep_min and mine is the smaller, or keep_max and mine the larger: stay
            key = take ? o : key;
            src = take ? os : src;
        }
    }
    // lane l: the fold of its triple over the sorted fibre.  Its own entry: axis 0: six copies (DWL: global); else left out.  Every
    // other entry twice; DWL: local where bit (l, source) is set.  A fold starts from the LAST element of its class.
    const bool mine = l < n;
    int m_loc = -1, m_glo = -1;
    for (int i = 0; i < G; ++i) {
        const int s = __shfl(src, base + i, 64);
        if (!mine || i >= n) continue;
        const bool self = s == l;
        if (self && axis != 0) continue;
        const bool glob = malkin && (self || ((bits >> s) & 1ull) == 0ull);
        if (glob) m_glo = i;
        else m_loc = i;
    }
    const u64 top_loc = shfl64(key, base + (m_loc >= 0 ? m_loc : 0)), top_glo = shfl64(key, base + (m_glo >= 0 ? m_glo : 0));
    u64 a_loc = top_loc, a_glo = top_glo;
    for (int i = 0; i < G; ++i) {
        const int s = __shfl(src, base + i, 64);
        const u64 e = shfl64(key, base + i);
        if (!mine || i >= n) continue;
        const bool self = s == l;
        if (self && axis != 0) continue;
        const bool glob = malkin && (self || ((bits >> s) & 1ull) == 0ull);
        int copies = self ? 6 : 2;
        if (i == (glob ? m_glo : m_loc)) --copies;               // one copy of the class's maximum started the fold
        u64 acc = glob ? a_glo : a_loc;
        for (int c = 0; c < copies; ++c) acc = wl_pair(acc, e);
        if (glob) a_glo = acc;
        else a_loc = acc;
    }
    if (mine) {
        work[(int64_t)axis * T + t_mine] = a_loc;
        if (malkin) work[(int64_t)(3 + axis) * T + t_mine] = a_glo;
    }
}

// WL / DWL, the closing pass: a lane per triple of a graph of at most kMaxNodes nodes (the others are left alone)
__global__ __launch_bounds__(kBlock) void k3_close_kernel(int64_t T, int malkin, const int32_t* __restrict__ tup_v,
                                                          const int32_t* __restrict__ tup_w, const int32_t* __restrict__ tup_u,
                                                          const int32_t* __restrict__ node_graph, const int32_t* __restrict__ node_ptr,
                                                          const int32_t* __restrict__ ptr, const u64* __restrict__ cin,
                                                          const u64* __restrict__ work, u64* __restrict__ cout) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= T) return;
    const int32_t node[3] = {tup_v[t], tup_w[t], tup_u[t]};
    const int32_t g = node_graph[node[0]];
    const int32_t n = node_ptr[g + 1] - node_ptr[g];
    if (n > kMaxNodes) return;
    u64 fl[3], fg[3] = {0ull, 0ull, 0ull};
    bool hl[3], hg[3] = {false, false, false};
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const int32_t deg = ptr[node[ax] + 1] - ptr[node[ax]];
        fl[ax] = work[(int64_t)ax * T + t];
        if (malkin) {
            hl[ax] = deg > 0;
            fg[ax] = work[(int64_t)(3 + ax) * T + t];
            hg[ax] = ax == 0 || n - 1 - deg > 0;
        } else {
            hl[ax] = ax == 0 || n > 1;
        }
    }
    cout[t] = k3_combine(cin[t], fl, hl, fg, hg);
}

bool fits_i32(int64_t v) { return v > 0 && v <= 0x7fffffffLL; }

}  // namespace

extern "C" {

int32_t dn_k3wl_max_nodes(void) { return kMaxNodes; }
int32_t dn_k3wl_max_entries(void) { return kMaxEntries; }

int dn_k3wl_init_u64(int64_t num_nodes, int64_t num_items, int32_t connected, const int32_t* tup_v, const int32_t* tup_w,
                     const int32_t* tup_u, const int32_t* ptr, const int32_t* nbr, const int64_t* node_label, int64_t* colors_out,
                     dn_stream_t stream) {
    DN_REQUIRE(fits_i32(num_nodes) && fits_i32(num_items), "dn_k3wl_init: bad sizes");
    DN_REQUIRE(tup_v && tup_w && tup_u && ptr && nbr && colors_out, "dn_k3wl_init: NULL pointer");   // (labels may be NULL: not used)
    hipLaunchKernelGGL(k3_init_kernel, dim3((unsigned)dn_cdiv(num_items, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, num_items,
                       (int)connected, tup_v, tup_w, tup_u, ptr, nbr, reinterpret_cast<const u64*>(node_label),
                       reinterpret_cast<u64*>(colors_out));
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_k3wl_local_u64(int64_t num_nodes, int64_t num_items, int64_t num_list, const int32_t* items, int32_t group, int32_t lds_entries,
                      int32_t connected, const int32_t* tup_v, const int32_t* tup_w, const int32_t* tup_u, const int32_t* node_graph,
                      const int32_t* node_ptr, const int32_t* tuple_ptr, const int32_t* ptr, const int32_t* nbr, const int64_t* item_key,
                      const int32_t* item_slot, const int64_t* colors_in, int64_t* colors_out, dn_stream_t stream) {
    DN_REQUIRE(fits_i32(num_nodes) && fits_i32(num_items) && fits_i32(num_list) && num_list <= num_items, "dn_k3wl_local: bad sizes");
    DN_REQUIRE(group == 8 || group == 64 || group == 0, "dn_k3wl_local: group must be 8, 64 or 0 (a workgroup per triple), got %d", group);
    DN_REQUIRE(tup_v && tup_w && tup_u && node_graph && node_ptr && tuple_ptr && ptr && nbr && colors_in && colors_out,
               "dn_k3wl_local: NULL pointer");
    DN_REQUIRE(!connected || (item_key && item_slot), "dn_k3wl_local: NULL pointer (LWLC needs the sorted item keys and their slots)");
    DN_REQUIRE(items || num_list == num_items, "dn_k3wl_local: NULL pointer (an item list is needed unless it is every item)");
    DN_REQUIRE(colors_in != colors_out, "dn_k3wl_local: colors_out must not alias colors_in");
    const u64* cin = reinterpret_cast<const u64*>(colors_in);
    u64* cout = reinterpret_cast<u64*>(colors_out);
    hipStream_t st = (hipStream_t)stream;
    K3Local a;
    a.connected = (int)connected;
    a.tup_v = tup_v; a.tup_w = tup_w; a.tup_u = tup_u; a.node_graph = node_graph; a.node_ptr = node_ptr; a.tuple_ptr = tuple_ptr;
    a.ptr = ptr; a.nbr = nbr; a.item_slot = item_slot; a.item_key = item_key;
    if (group == 0) {
        DN_REQUIRE(lds_entries >= 1 && lds_entries <= 2 * kMaxEntries && (lds_entries & (lds_entries - 1)) == 0,
                   "dn_k3wl_local: lds_entries must be a power of two <= %d (got %d)", 2 * kMaxEntries, lds_entries);
        const size_t lds = (size_t)3 * lds_entries * sizeof(u64);
        hipLaunchKernelGGL(k3_local_block_kernel, dim3((unsigned)num_list), dim3(kBlock), lds, st, items, lds_entries, a, cin, cout);
    } else {
        const int64_t blocks = dn_cdiv(num_list * group, kBlock);
        DN_REQUIRE(blocks <= 0x7fffffffLL, "dn_k3wl_local: bad sizes");
        if (group == 8)
            hipLaunchKernelGGL(k3_local_group_kernel<8>, dim3((unsigned)blocks), dim3(kBlock), 0, st, num_list, items, a, cin, cout);
        else
            hipLaunchKernelGGL(k3_local_group_kernel<64>, dim3((unsigned)blocks), dim3(kBlock), 0, st, num_list, items, a, cin, cout);
    }
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_k3wl_global_u64(int64_t num_graphs, int64_t num_items, int64_t num_list, const int32_t* graphs, const int32_t* fib_ptr,
                       int64_t num_fibres, int32_t group, int32_t malkin, const int32_t* node_ptr, const int32_t* tuple_ptr,
                       const int64_t* adj_bits, const int64_t* colors_in, int64_t* work, dn_stream_t stream) {
    DN_REQUIRE(fits_i32(num_graphs) && fits_i32(num_items) && fits_i32(num_list) && num_list <= num_graphs && fits_i32(num_fibres),
               "dn_k3wl_global: bad sizes");
    DN_REQUIRE(group == 8 || group == 16 || group == 32 || group == 64, "dn_k3wl_global: group must be 8, 16, 32 or 64 (got %d)", group);
    DN_REQUIRE(graphs && fib_ptr && node_ptr && tuple_ptr && colors_in && work, "dn_k3wl_global: NULL pointer");
    DN_REQUIRE(!malkin || adj_bits, "dn_k3wl_global: NULL pointer (DWL needs the adjacency bit rows)");
    DN_REQUIRE(work != colors_in, "dn_k3wl_global: work must not alias colors_in");
    const int64_t blocks = dn_cdiv(num_fibres * group, kBlock);
    DN_REQUIRE(blocks <= 0x7fffffffLL, "dn_k3wl_global: bad sizes");
    const u64* cin = reinterpret_cast<const u64*>(colors_in);
    const u64* bits = reinterpret_cast<const u64*>(adj_bits);
    u64* wk = reinterpret_cast<u64*>(work);
    hipStream_t st = (hipStream_t)stream;
#define DN_K3_FIBRE(G)                                                                                                                   \
    hipLaunchKernelGGL(k3_fibre_kernel<G>, dim3((unsigned)blocks), dim3(kBlock), 0, st, num_fibres, (int32_t)num_list, graphs, fib_ptr, \
                       (int)malkin, node_ptr, tuple_ptr, bits, cin, wk, num_items)
    if (group == 8) DN_K3_FIBRE(8);
    else if (group == 16) DN_K3_FIBRE(16);
    else if (group == 32) DN_K3_FIBRE(32);
    else DN_K3_FIBRE(64);
#undef DN_K3_FIBRE
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_k3wl_close_u64(int64_t num_nodes, int64_t num_items, int32_t malkin, const int32_t* tup_v, const int32_t* tup_w, const int32_t* tup_u,
                      const int32_t* node_graph, const int32_t* node_ptr, const int32_t* ptr, const int64_t* colors_in, const int64_t* work,
                      int64_t* colors_out, dn_stream_t stream) {
    DN_REQUIRE(fits_i32(num_nodes) && fits_i32(num_items), "dn_k3wl_close: bad sizes");
    DN_REQUIRE(tup_v && tup_w && tup_u && node_graph && node_ptr && ptr && colors_in && work && colors_out, "dn_k3wl_close: NULL pointer");
    DN_REQUIRE(colors_in != colors_out && work != colors_in && work != colors_out, "dn_k3wl_close: colors_out and work must not alias");
    hipLaunchKernelGGL(k3_close_kernel, dim3((unsigned)dn_cdiv(num_items, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, num_items,
                       (int)malkin, tup_v, tup_w, tup_u, node_graph, node_ptr, ptr, reinterpret_cast<const u64*>(colors_in),
                       reinterpret_cast<const u64*>(work), reinterpret_cast<u64*>(colors_out));
    DN_CHECK_LAUNCH();
    return DN_OK;
}

}  // extern "C"
