// The shortest-path and graphlet graph kernels' feature extractors (graph_classification/graph_kernels: `gram --kernel SP | GR`):
// exact integer work on the deduplicated undirected CSR of a whole dataset (docs/LAB_NOTES.md "Graph kernels: SP / GR").  Both end
// in (graph, key, count) entries that the caller sorts into the feature CSR of dn_wl_gram_i64; there is no gram kernel here.
//
// SP.  One BFS per source node over BIT SETS: the newly reached set of level d, intersected with each label class of the graph,
// gives the count of (label of b, d) by population count -- no n x n distance matrix is written anywhere.  Two classes of graphs:
//     <= 64 nodes        one wavefront per graph, one lane per source; a lane holds its node's adjacency row as a 64-bit mask and
//                        a level ORs the rows of the frontier's set bits (a uniform loop of row broadcasts)
//     <= kSpLdsNodes     one workgroup per graph, the bit matrix (n * ceil(n / 64) words) in LDS, a wavefront per source in turn:
//                        lanes split the frontier's nodes and OR their rows into the next set with LDS atomics; per-class counts
//                        are an LDS histogram over the graph's local class ids
// Larger graphs are the caller's composed path.  A source emits one entry per (class, level) that is not empty, one for the nodes it
// cannot reach (distance INT_MAX) and one for itself (distance 2 where it has a neighbour, else INT_MAX, count 2: the reference's
// in-place Floyd-Warshall).  A source whose key base is negative is filtered (the reference drops lo32(label) 0 and INT_MAX).
// The entry count is not known in advance: the same kernel runs twice, first counting per source (offsets == NULL), then -- after
// the caller's exclusive scan -- filling.  Both passes walk the same order, so the fill is deterministic.
//
// GR.  A work item is a centre node v and a range of rows i of its ascending neighbour list; row i pairs u = nbr[i] with every
// later w = nbr[j].  (u, w) adjacent (binary search in u's list): a triangle, counted only where v < u (< w), its smallest node;
// else a wedge.  Every pair owns one slot of the caller's key workspace (graph id -1: nothing to count), which the caller reduces
// chunk by chunk.  Items of at most 8 pairs take 8 lanes, of at most 64 a wavefront, longer ones a workgroup.
#include <hip/hip_runtime.h>

#include "dn_common.h"
#include "dn_hip.h"
#include "dn_wl_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kSpLdsNodes = 512;         // the bit matrix of 512 nodes is 32 KiB; with the per-wave sets and histograms 41.8 KiB
constexpr int kIntMax = 0x7fffffff;

__device__ __forceinline__ int64_t sp_key(int64_t base, int32_t rb, int32_t d) { return (int64_t)(((u64)(base + rb) << 32) | (u64)(unsigned)d); }

// LDS written by some lanes of a wavefront and read by others: DS operations of one wavefront complete in order, so only the
// compiler has to be kept from moving them
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---------------------------------------------------------------------------------------------------------------- SP, <= 64 nodes
template <bool FILL>
__global__ __launch_bounds__(kBlock) void sp_wave_kernel(int64_t num, const int32_t* __restrict__ graphs, const int32_t* __restrict__ node_ptr,
                                                         const int32_t* __restrict__ ptr, const int32_t* __restrict__ nbr,
                                                         const int64_t* __restrict__ src_base, const int32_t* __restrict__ lcls,
                                                         const int32_t* __restrict__ cls_ptr, const int32_t* __restrict__ cls_rb,
                                                         int32_t* __restrict__ counts, const int64_t* __restrict__ offsets, int64_t out_cap,
                                                         int64_t* __restrict__ out_key, int32_t* __restrict__ out_cnt) {
    const int64_t wid = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const int lane = (int)(threadIdx.x & 63);
    if (wid >= num) return;                                   // (uniform per wavefront; no workgroup barrier below)
    const int32_t g = graphs[wid];
    const int32_t n0 = node_ptr[g], n = node_ptr[g + 1] - n0;
    if (n < 1 || n > 64) return;                              // (uniform) a graph of another class is left alone
    const bool node = lane < n;
    const int32_t c0 = cls_ptr[g], L = cls_ptr[g + 1] - c0;
    u64 adj = 0;
    int32_t mycls = -1;
    int64_t base = -1;
    if (node) {
        const int32_t v = n0 + lane;
        for (int32_t e = ptr[v]; e < ptr[v + 1]; ++e) {
            const int32_t w = nbr[e] - n0;
            if (w >= 0 && w < n && w != lane) adj |= 1ull << w;
        }
        mycls = lcls[v];
        base = src_base[v];
    }
    const bool src = node && base >= 0;
    const int64_t off = (FILL && src) ? offsets[n0 + lane] : 0;
    int32_t total = 0;
    u64 visited = node ? ((1ull << lane) | adj) : 0, frontier = adj;
    const u64 all = n == 64 ? ~0ull : ((1ull << n) - 1);
    for (int32_t d = 1;; ++d) {
        const bool last = __ballot(frontier != 0) == 0;       // no lane has anything new: emit the unreachable nodes and stop
        const u64 m = last ? (all & ~visited) : frontier;
        for (int32_t c = 0; c < L; ++c) {
            const u64 cm = __ballot(mycls == c);
            const int32_t k = __popcll(m & cm);
            if (src && k) {
                if (FILL && off + total < out_cap) {
                    out_key[off + total] = sp_key(base, cls_rb[c0 + c], last ? kIntMax : d);
                    out_cnt[off + total] = k;
                }
                ++total;
            }
        }
        if (last) break;
        u64 next = 0;
        for (int32_t j = 0; j < n; ++j) {
            const u64 row = shfl64(adj, j);
            if ((frontier >> j) & 1) next |= row;
        }
        frontier = next & ~visited;
        visited |= frontier;
    }
    if (src) {
        if (FILL && off + total < out_cap) {
            out_key[off + total] = sp_key(base, cls_rb[c0 + mycls], adj ? 2 : kIntMax);
            out_cnt[off + total] = 2;
        }
        ++total;
        if (!FILL) counts[n0 + lane] = total;
    }
}

// ------------------------------------------------------------------------------------------------- SP, the bit matrix fits in LDS
// one (class, count) entry per class whose histogram bucket is not empty; the buckets are left zero
template <bool FILL>
__device__ __forceinline__ int32_t sp_emit(int32_t L, int lane, int32_t* __restrict__ cnt, const int32_t* __restrict__ rb, int64_t base, int32_t d,
                                           int64_t off, int64_t out_cap, int32_t total, int64_t* __restrict__ out_key, int32_t* __restrict__ out_cnt) {
    for (int32_t cb = 0; cb < L; cb += 64) {
        const int32_t c = cb + lane;
        const int32_t k = c < L ? cnt[c] : 0;
        const u64 m = __ballot(k > 0);
        if (k > 0) {
            if (FILL) {
                const int64_t pos = off + total + __popcll(m & ((1ull << lane) - 1));
                if (pos < out_cap) {
                    out_key[pos] = sp_key(base, rb[c], d);
                    out_cnt[pos] = k;
                }
            }
            cnt[c] = 0;
        }
        total += __popcll(m);
    }
    return total;
}

template <bool FILL>
__global__ __launch_bounds__(kBlock) void sp_block_kernel(const int32_t* __restrict__ graphs, int32_t lds_nodes, const int32_t* __restrict__ node_ptr,
                                                          const int32_t* __restrict__ ptr, const int32_t* __restrict__ nbr,
                                                          const int64_t* __restrict__ src_base, const int32_t* __restrict__ lcls,
                                                          const int32_t* __restrict__ cls_ptr, const int32_t* __restrict__ cls_rb,
                                                          int32_t* __restrict__ counts, const int64_t* __restrict__ offsets, int64_t out_cap,
                                                          int64_t* __restrict__ out_key, int32_t* __restrict__ out_cnt) {
    extern __shared__ u64 gk_s[];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t g = graphs[blockIdx.x];
    const int32_t n0 = node_ptr[g], n = node_ptr[g + 1] - n0;
    if (n < 1 || n > lds_nodes) return;                       // (uniform) a graph larger than the launch's LDS is left alone
    const int32_t nw = (n + 63) >> 6, nwl = (lds_nodes + 63) >> 6;
    u64* adj = gk_s;                                          // [n][nw]
    u64* sets = gk_s + (size_t)lds_nodes * nwl + (size_t)wave * 3 * nwl;
    u64 *vis = sets, *fr = sets + nwl, *nx = sets + 2 * nwl;
    int32_t* cnt = reinterpret_cast<int32_t*>(gk_s + (size_t)lds_nodes * nwl + (size_t)kWaves * 3 * nwl) + (size_t)wave * lds_nodes;
    const int32_t c0 = cls_ptr[g], L = min(cls_ptr[g + 1] - c0, n);
    for (int32_t k = tid; k < n * nw; k += kBlock) adj[k] = 0;
    for (int32_t k = lane; k < n; k += 64) cnt[k] = 0;
    __syncthreads();
    for (int32_t a = tid; a < n; a += kBlock)                 // (a row belongs to one thread: plain read-modify-write)
        for (int32_t e = ptr[n0 + a]; e < ptr[n0 + a + 1]; ++e) {
            const int32_t w = nbr[e] - n0;
            if (w >= 0 && w < n && w != a) adj[a * nw + (w >> 6)] |= 1ull << (w & 63);
        }
    __syncthreads();                                          // the last workgroup barrier: the waves run apart from here on
    for (int32_t a = wave; a < n; a += kWaves) {
        const int64_t base = src_base[n0 + a];
        if (base < 0) continue;                               // (uniform per wavefront) a filtered source
        const int64_t off = FILL ? offsets[n0 + a] : 0;
        int32_t total = 0;
        u64 any = 0;
        for (int32_t w = lane; w < nw; w += 64) {
            const u64 self = (w == (a >> 6)) ? 1ull << (a & 63) : 0, f = adj[a * nw + w];
            vis[w] = self | f;
            fr[w] = f;
            nx[w] = 0;
            any |= f;
        }
        const bool has_nbr = __ballot(any != 0) != 0;
        wave_sync();
        for (int32_t d = 1;; ++d) {
            const bool last = __ballot(any != 0) == 0;
            if (last) {                                       // the nodes never reached, at distance INT_MAX
                for (int32_t w = lane; w < nw; w += 64) {
                    const u64 valid = (w == nw - 1 && (n & 63)) ? ((1ull << (n & 63)) - 1) : ~0ull;
                    fr[w] = valid & ~vis[w];
                }
                wave_sync();
            }
            for (int32_t b = lane; b < n; b += 64)
                if ((fr[b >> 6] >> (b & 63)) & 1) {
                    const int32_t c = lcls[n0 + b];
                    if (c >= 0 && c < L) atomicAdd(&cnt[c], 1);
                }
            wave_sync();
            total = sp_emit<FILL>(L, lane, cnt, cls_rb + c0, base, last ? kIntMax : d, off, out_cap, total, out_key, out_cnt);
            wave_sync();
            if (last) break;
            for (int32_t j = lane; j < n; j += 64)
                if ((fr[j >> 6] >> (j & 63)) & 1)
                    for (int32_t w = 0; w < nw; ++w) {
                        const u64 row = adj[j * nw + w];
                        if (row) atomicOr(&nx[w], row);
                    }
            wave_sync();
            any = 0;
            for (int32_t w = lane; w < nw; w += 64) {
                const u64 f = nx[w] & ~vis[w];
                fr[w] = f;
                vis[w] |= f;
                nx[w] = 0;
                any |= f;
            }
            wave_sync();
        }
        if (lane == 0) {
            if (FILL) {
                if (off + total < out_cap) {
                    out_key[off + total] = sp_key(base, cls_rb[c0 + lcls[n0 + a]], has_nbr ? 2 : kIntMax);
                    out_cnt[off + total] = 2;
                }
            } else {
                counts[n0 + a] = total + 1;
            }
        }
    }
}

size_t sp_lds_bytes(int32_t lds_nodes) {
    const size_t nwl = (size_t)(lds_nodes + 63) / 64;
    return ((size_t)lds_nodes * nwl + (size_t)kWaves * 3 * nwl) * sizeof(u64) + (size_t)kWaves * lds_nodes * sizeof(int32_t);
}

// ---------------------------------------------------------------------------------------------------------------------------- GR
struct GrArgs {
    const int32_t* ptr;
    const int32_t* nbr;
    const u64* nl;          // NULL: no node labels (keys 2 and 3, edge labels ignored)
    const u64* el;          // per slot, NULL: no edge labels
    const int32_t* node_graph;
    int64_t cap;
    int64_t* key;
    int32_t* gid;
};

// P(list) of the reference: the pairing fold over the list, started at the list's length
__device__ __forceinline__ u64 gk_fold3(u64 a, u64 b, u64 c) { return wl_pair(wl_pair(wl_pair(3ull, a), b), c); }
__device__ __forceinline__ u64 gk_fold5(u64 a, u64 b, u64 c, u64 d, u64 e) { return wl_pair(wl_pair(wl_pair(wl_pair(wl_pair(5ull, a), b), c), d), e); }
__device__ __forceinline__ u64 gk_min(u64 a, u64 b) { return a < b ? a : b; }

__device__ __forceinline__ u64 gk_fold6(u64 a, u64 b, u64 c, u64 d, u64 e, u64 f) {
    return wl_pair(wl_pair(wl_pair(wl_pair(wl_pair(wl_pair(6ull, a), b), c), d), e), f);
}

// the pair (slot eu, slot ew) of centre v, eu < ew: its key and graph into workspace slot pos
__device__ __forceinline__ void gr_pair(const GrArgs& A, int32_t v, int32_t eu, int32_t ew, int64_t pos) {
    if (pos < 0 || pos >= A.cap) return;                      // never outside the caller's workspace
    const int32_t u = A.nbr[eu], w = A.nbr[ew];
    int32_t lo = A.ptr[u], hi = A.ptr[u + 1];
    while (lo < hi) {                                         // the first slot of u whose neighbour is >= w
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (A.nbr[mid] < w) lo = mid + 1; else hi = mid;
    }
    const bool tri = lo < A.ptr[u + 1] && A.nbr[lo] == w;
    u64 key;
    int32_t g = A.node_graph[v];
    if (tri && !(v < u)) {
        key = 0;
        g = -1;                                               // this triangle is counted at its smallest node
    } else if (!A.nl) {
        key = tri ? 3ull : 2ull;
    } else {
        const u64 lu = A.nl[u], lv = A.nl[v], lw = A.nl[w];
        if (!tri) {
            if (A.el) {
                const u64 uv = A.el[eu], vw = A.el[ew];
                key = gk_min(gk_fold5(lu, uv, lv, vw, lw), gk_fold5(lw, vw, lv, uv, lu));
            } else {
                key = gk_min(gk_fold3(lu, lv, lw), gk_fold3(lw, lv, lu));
            }
        } else if (A.el) {
            const u64 uv = A.el[eu], vw = A.el[ew], uw = A.el[lo];
            key = gk_min(gk_min(gk_min(gk_fold6(lu, uv, lv, vw, lw, uw), gk_fold6(lu, uw, lw, vw, lv, uv)),
                                gk_min(gk_fold6(lv, uv, lu, uw, lw, vw), gk_fold6(lv, vw, lw, uw, lu, uv))),
                         gk_min(gk_fold6(lw, uw, lu, uv, lv, vw), gk_fold6(lw, vw, lv, uv, lu, uw)));
        } else {
            u64 a = lu, b = lv, c = lw, t;
            if (a > b) { t = a; a = b; b = t; }
            if (b > c) { t = b; b = c; c = t; }
            if (a > b) { t = a; a = b; b = t; }
            key = gk_fold3(a, b, c);
        }
    }
    A.key[pos] = (int64_t)key;
    A.gid[pos] = g;
}

// G lanes per item (G = 8 or 64): an item of at most G pairs, one pair per lane
template <int G>
__global__ __launch_bounds__(kBlock) void gr_group_kernel(int64_t num, const int32_t* __restrict__ it_node, const int32_t* __restrict__ it_i0,
                                                          const int32_t* __restrict__ it_i1, const int64_t* __restrict__ it_off, GrArgs A) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t item = t / G;
    const int32_t l = (int32_t)(t & (G - 1));
    if (item >= num) return;
    const int32_t v = it_node[item], beg = A.ptr[v], deg = A.ptr[v + 1] - beg;
    int32_t i = it_i0[item], r = l;
    const int32_t i1 = min(it_i1[item], deg);
    if (i < 0) return;
    while (i < i1 && r >= deg - 1 - i) {
        r -= deg - 1 - i;
        ++i;
    }
    if (i >= i1) return;                                      // (an item of more than G pairs leaves its tail unwritten: gid stays -1)
    gr_pair(A, v, beg + i, beg + i + 1 + r, it_off[item] + l);
}

// one workgroup per item: row after row, the threads over the row's pairs
__global__ __launch_bounds__(kBlock) void gr_block_kernel(const int32_t* __restrict__ it_node, const int32_t* __restrict__ it_i0,
                                                          const int32_t* __restrict__ it_i1, const int64_t* __restrict__ it_off, GrArgs A) {
    const int64_t item = blockIdx.x;
    const int32_t v = it_node[item], beg = A.ptr[v], deg = A.ptr[v + 1] - beg;
    const int32_t i0 = it_i0[item], i1 = min(it_i1[item], deg);
    if (i0 < 0) return;
    int64_t row = it_off[item];
    for (int32_t i = i0; i < i1; ++i) {
        for (int32_t j = i + 1 + (int32_t)threadIdx.x; j < deg; j += kBlock) gr_pair(A, v, beg + i, beg + j, row + (j - i - 1));
        row += deg - 1 - i;
    }
}

bool fits_i32(int64_t v) { return v > 0 && v <= 0x7fffffffLL; }

}  // namespace

extern "C" {

int32_t dn_gk_sp_lds_max_nodes(void) { return kSpLdsNodes; }

int dn_gk_sp_u64(int64_t num_graphs, int64_t num_list, const int32_t* graphs, int32_t group, int32_t lds_nodes, const int32_t* node_ptr,
                 const int32_t* ptr, const int32_t* nbr, const int64_t* src_base, const int32_t* local_class, const int32_t* class_ptr,
                 const int32_t* class_rank, int32_t* counts, const int64_t* offsets, int64_t out_entries, int64_t* out_key,
                 int32_t* out_count,
                 dn_stream_t stream) {
    DN_REQUIRE(fits_i32(num_graphs) && fits_i32(num_list) && num_list <= num_graphs, "dn_gk_sp: bad sizes");
    DN_REQUIRE(group == 64 || group == 0, "dn_gk_sp: group must be 64 (a wavefront per graph) or 0 (a workgroup per graph), got %d", group);
    DN_REQUIRE(graphs && node_ptr && ptr && nbr && src_base && local_class && class_ptr && class_rank, "dn_gk_sp: NULL pointer");
    DN_REQUIRE(offsets ? (out_key && out_count && out_entries > 0) : counts != nullptr,
               "dn_gk_sp: NULL pointer (counts for the counting pass, offsets with out_key and out_count for the fill)");
    hipStream_t st = (hipStream_t)stream;
    const bool fill = offsets != nullptr;
    if (group == 0) {
        DN_REQUIRE(lds_nodes >= 1 && lds_nodes <= kSpLdsNodes, "dn_gk_sp: lds_nodes must be 1 .. %d (got %d)", kSpLdsNodes, lds_nodes);
        const size_t lds = sp_lds_bytes(lds_nodes);
        if (fill)
            hipLaunchKernelGGL(sp_block_kernel<true>, dim3((unsigned)num_list), dim3(kBlock), lds, st, graphs, lds_nodes, node_ptr, ptr, nbr,
                               src_base, local_class, class_ptr, class_rank, counts, offsets, out_entries, out_key, out_count);
        else
            hipLaunchKernelGGL(sp_block_kernel<false>, dim3((unsigned)num_list), dim3(kBlock), lds, st, graphs, lds_nodes, node_ptr, ptr, nbr,
                               src_base, local_class, class_ptr, class_rank, counts, offsets, out_entries, out_key, out_count);
    } else {
        const unsigned blocks = (unsigned)dn_cdiv(num_list, kWaves);
        if (fill)
            hipLaunchKernelGGL(sp_wave_kernel<true>, dim3(blocks), dim3(kBlock), 0, st, num_list, graphs, node_ptr, ptr, nbr, src_base,
                               local_class, class_ptr, class_rank, counts, offsets, out_entries, out_key, out_count);
        else
            hipLaunchKernelGGL(sp_wave_kernel<false>, dim3(blocks), dim3(kBlock), 0, st, num_list, graphs, node_ptr, ptr, nbr, src_base,
                               local_class, class_ptr, class_rank, counts, offsets, out_entries, out_key, out_count);
    }
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_gk_gr_keys_u64(int64_t num_nodes, int64_t num_items, int32_t group, const int32_t* item_node, const int32_t* item_row0,
                      const int32_t* item_row1, const int64_t* item_offset, const int32_t* ptr, const int32_t* nbr, const int64_t* node_label,
                      const int64_t* edge_label, const int32_t* node_graph, int64_t workspace_keys, int64_t* ws_key, int32_t* ws_graph,
                      dn_stream_t stream) {
    DN_REQUIRE(fits_i32(num_nodes) && fits_i32(num_items), "dn_gk_gr_keys: bad sizes");
    DN_REQUIRE(group == 8 || group == 64 || group == 0, "dn_gk_gr_keys: group must be 8, 64 or 0 (a workgroup per item), got %d", group);
    DN_REQUIRE(workspace_keys > 0, "dn_gk_gr_keys: bad sizes (an empty key workspace)");
    DN_REQUIRE(item_node && item_row0 && item_row1 && item_offset && ptr && nbr && node_graph && ws_key && ws_graph,
               "dn_gk_gr_keys: NULL pointer");
    DN_REQUIRE(node_label || !edge_label, "dn_gk_gr_keys: edge labels need node labels (without them every key is 2 or 3)");
    GrArgs A{ptr, nbr, reinterpret_cast<const u64*>(node_label), reinterpret_cast<const u64*>(edge_label), node_graph, workspace_keys,
             ws_key, ws_graph};
    hipStream_t st = (hipStream_t)stream;
    if (group == 0) {
        hipLaunchKernelGGL(gr_block_kernel, dim3((unsigned)num_items), dim3(kBlock), 0, st, item_node, item_row0, item_row1, item_offset, A);
    } else {
        const int64_t blocks = dn_cdiv(num_items * group, kBlock);
        DN_REQUIRE(blocks <= 0x7fffffffLL, "dn_gk_gr_keys: bad sizes");
        if (group == 8)
            hipLaunchKernelGGL(gr_group_kernel<8>, dim3((unsigned)blocks), dim3(kBlock), 0, st, num_items, item_node, item_row0, item_row1,
                               item_offset, A);
        else
            hipLaunchKernelGGL(gr_group_kernel<64>, dim3((unsigned)blocks), dim3(kBlock), 0, st, num_items, item_node, item_row0, item_row1,
                               item_offset, A);
    }
    DN_CHECK_LAUNCH();
    return DN_OK;
}

}  // extern "C"
