// Weisfeiler-Lehman graph kernels at k = 1 (graph_classification/graph_kernels: `gram --k 1 --kernel WL | WLOA`): colour refinement
// and the gram matrices of all iterations, in exact 64-bit integer arithmetic (docs/LAB_NOTES.md "Graph kernels: WL / WLOA").
//
// Refinement.  A node's new colour is a sequential fold of Szudzik's pairing function over the ascending (unsigned) list of its
// entries: one entry c[n] per neighbour n, and with edge labels one more, pairing(c[n], label(v, n)).  Everything wraps mod 2^64.
// The caller sorts the nodes into classes by entry count once per dataset and launches one kernel per class:
//     <= 8 entries     8 lanes per node   (8 nodes per wavefront: the ordinary nodes of a molecule)
//     <= 64 entries    one wavefront per node; both sort one entry per lane with a bitonic network of xor shuffles
//     <= 8192 entries  one workgroup per node, bitonic sort in LDS (the dummy node: its list is as long as its graph)
// and above kMaxEntries the composed path: a device-wide segmented sort by the caller, then wl_fold_kernel.  The fold itself cannot
// be split (the pairing function is neither associative nor commutative), so one lane walks the sorted list.
//
// Gram.  The feature row of a graph is the value-sorted list of its distinct colours with a count and a step each; a colour common
// to graphs i and j contributes count_i * count_j (WL) or min(count_i, count_j) (WLOA) to matrix h for every h >= max(step_i,
// step_j).  One workgroup takes a 16 x 16 tile of pairs of the upper triangle, one thread a pair: a merge join of two sorted rows
// into S = H + 1 buckets held in LDS (a per-thread array indexed by the step would live in scratch), then the prefix sum over h and
// the two mirrored stores.  The rows stay in global memory: the 16 + 16 rows of a tile are consecutive in the feature CSR and are
// shared by its 256 joins, so they live in the CU's L1.  Staging them in LDS was built and measured slower at every stage size (the
// stage costs occupancy: docs/LAB_NOTES.md), so no row length is special.  Integer sums only: two runs give the same bits.
#include <hip/hip_runtime.h>

#include "dn_common.h"
#include "dn_hip.h"
#include "dn_wl_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxEntries = 8192;        // the longest list the workgroup kernel sorts (64 KiB of LDS)
constexpr int kMaxSteps = 16;            // H + 1 of the gram kernel (2 KiB of LDS buckets per step)
constexpr int kTile = 16;                // the gram kernel's pair tile: kTile x kTile pairs per workgroup

// entry k of a node whose slots start at beg: mult = 1: c[nbr]; mult = 2: odd k = pairing(c[nbr], label), even k = c[nbr]
__device__ __forceinline__ u64 wl_entry(int32_t beg, int32_t k, bool labelled, const int32_t* __restrict__ nbr,
                                        const u64* __restrict__ el, const u64* __restrict__ cin) {
    const int32_t e = beg + (labelled ? (k >> 1) : k);
    const u64 c = cin[nbr[e]];
    return (labelled && (k & 1)) ? wl_pair(c, el[e]) : c;
}

// G lanes per node (G = 8 or 64), one entry per lane; padding lanes hold 2^64 - 1 (dn_wl_common.h: wl_sort_group)
template <int G>
__global__ __launch_bounds__(kBlock) void wl_refine_group_kernel(int64_t num, const int32_t* __restrict__ nodes,
                                                                 const int32_t* __restrict__ ptr, const int32_t* __restrict__ nbr,
                                                                 const u64* __restrict__ el, const u64* __restrict__ cin,
                                                                 u64* __restrict__ cout) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t g = t / G;
    const int lane = (int)(threadIdx.x & 63), l = lane & (G - 1), base = lane & ~(G - 1);
    const bool labelled = el != nullptr;
    bool active = g < num;
    int32_t v = 0, beg = 0, cnt = 0;
    if (active) {
        v = nodes ? nodes[g] : (int32_t)g;
        beg = ptr[v];
        cnt = (ptr[v + 1] - beg) * (labelled ? 2 : 1);
        active = cnt >= 0 && cnt <= G;                       // a node of another class is left alone
        if (!active) cnt = 0;
    }
    u64 val = ~0ull;
    if (l < cnt) val = wl_entry(beg, l, labelled, nbr, el, cin);
    val = wl_sort_group<G>(val, lane, l);
    u64 c = active ? cin[v] : 0ull;
    for (int i = 0; i < G; ++i) {
        if (G == 64 && i >= cnt) break;                      // (one node per wavefront: cnt is uniform)
        const u64 e = shfl64(val, base + i);
        if (i < cnt) c = wl_pair(c, e);
    }
    if (active && l == 0) cout[v] = c;
}

// one workgroup per node: bitonic sort of the next power of two >= cnt in LDS (lds_entries: a power of two, the launch's capacity)
__global__ __launch_bounds__(kBlock) void wl_refine_block_kernel(const int32_t* __restrict__ nodes, int32_t lds_entries,
                                                                 const int32_t* __restrict__ ptr, const int32_t* __restrict__ nbr,
                                                                 const u64* __restrict__ el, const u64* __restrict__ cin,
                                                                 u64* __restrict__ cout) {
    extern __shared__ u64 wl_s[];
    const int tid = (int)threadIdx.x;
    const bool labelled = el != nullptr;
    const int32_t v = nodes ? nodes[blockIdx.x] : (int32_t)blockIdx.x;
    const int32_t beg = ptr[v];
    const int32_t cnt = (ptr[v + 1] - beg) * (labelled ? 2 : 1);
    if (cnt < 0 || cnt > lds_entries) return;                // (uniform) a list longer than the launch's LDS is left alone
    int32_t n2 = 1;
    while (n2 < cnt) n2 <<= 1;
    for (int32_t k = tid; k < n2; k += kBlock) wl_s[k] = k < cnt ? wl_entry(beg, k, labelled, nbr, el, cin) : ~0ull;
    __syncthreads();
    wl_sort_block<kBlock>(wl_s, n2, tid);
    if (tid == 0) {
        u64 c = cin[v];
        for (int32_t i = 0; i < cnt; ++i) c = wl_pair(c, wl_s[i]);
        cout[v] = c;
    }
}

// the composed path's fold: segment s = sorted[seg_ptr[s] .. seg_ptr[s + 1]) already ascending, one thread per segment
__global__ __launch_bounds__(kBlock) void wl_fold_kernel(int64_t num, const int32_t* __restrict__ nodes, const int64_t* __restrict__ seg_ptr,
                                                         const u64* __restrict__ sorted, const u64* __restrict__ cin,
                                                         u64* __restrict__ cout) {
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= num) return;
    const int32_t v = nodes ? nodes[s] : (int32_t)s;
    u64 c = cin[v];
    for (int64_t i = seg_ptr[s]; i < seg_ptr[s + 1]; ++i) c = wl_pair(c, sorted[i]);
    cout[v] = c;
}

// the merge join of rows [a, ae) and [b, be) of the feature CSR into this thread's buckets acc[h * kBlock]
template <bool MIN>
__device__ __forceinline__ void wl_join(const u64* __restrict__ col, const int32_t* __restrict__ cnt, const int32_t* __restrict__ step,
                                        int32_t a, int32_t ae, int32_t b, int32_t be, int32_t S, int64_t* __restrict__ acc) {
    if (a >= ae || b >= be) return;
    u64 ca = col[a], cb = col[b];
    for (;;) {
        if (ca == cb) {
            const int32_t h = max(step[a], step[b]);
            const int64_t na = cnt[a], nb = cnt[b];
            if (h >= 0 && h < S) acc[h * kBlock] += MIN ? (na < nb ? na : nb) : na * nb;
            if (++a >= ae || ++b >= be) break;
            ca = col[a];
            cb = col[b];
        } else if (ca < cb) {
            if (++a >= ae) break;
            ca = col[a];
        } else {
            if (++b >= be) break;
            cb = col[b];
        }
    }
}

template <bool MIN>
__global__ __launch_bounds__(kBlock) void wl_gram_kernel(int32_t B, int32_t S, const int32_t* __restrict__ fptr, const u64* __restrict__ fcol,
                                                         const int32_t* __restrict__ fcnt, const int32_t* __restrict__ fstep,
                                                         int64_t* __restrict__ out) {
    const int32_t ti = (int32_t)blockIdx.y, tj = (int32_t)blockIdx.x;
    if (tj < ti) return;                                     // the upper triangle of tiles; the stores mirror it
    extern __shared__ int64_t wl_acc[];
    int64_t* acc = wl_acc + threadIdx.x;                     // bucket h of this thread: acc[h * kBlock] (no other thread touches it)
    const int tid = (int)threadIdx.x;
    const int32_t i = ti * kTile + (tid >> 4), j = tj * kTile + (tid & (kTile - 1));
    if (i >= B || j >= B || i > j) return;
    for (int32_t h = 0; h < S; ++h) acc[h * kBlock] = 0;
    wl_join<MIN>(fcol, fcnt, fstep, fptr[i], fptr[i + 1], fptr[j], fptr[j + 1], S, acc);
    const size_t BB = (size_t)B * B, ij = (size_t)i * B + j, ji = (size_t)j * B + i;
    int64_t run = 0;
    for (int32_t h = 0; h < S; ++h) {
        run += acc[h * kBlock];
        out[h * BB + ij] = run;
        out[h * BB + ji] = run;
    }
}

bool fits_i32(int64_t v) { return v > 0 && v <= 0x7fffffffLL; }

}  // namespace

extern "C" {

int32_t dn_wl_max_entries(void) { return kMaxEntries; }
int32_t dn_wl_max_steps(void) { return kMaxSteps; }
int32_t dn_wl_gram_tile(void) { return kTile; }

int dn_wl_refine_u64(int64_t num_nodes, int64_t num_list, const int32_t* nodes, int32_t group, int32_t lds_entries, const int32_t* ptr,
                     const int32_t* nbr, const int64_t* edge_label, const int64_t* colors_in, int64_t* colors_out, dn_stream_t stream) {
    DN_REQUIRE(fits_i32(num_nodes) && fits_i32(num_list) && num_list <= num_nodes, "dn_wl_refine: bad sizes");
    DN_REQUIRE(group == 8 || group == 64 || group == 0, "dn_wl_refine: group must be 8, 64 or 0 (a workgroup per node), got %d", group);
    DN_REQUIRE(ptr && nbr && colors_in && colors_out, "dn_wl_refine: NULL pointer");
    DN_REQUIRE(nodes || num_list == num_nodes, "dn_wl_refine: NULL pointer (a node list is needed unless it is every node)");
    DN_REQUIRE(colors_in != colors_out, "dn_wl_refine: colors_out must not alias colors_in");
    const u64* el = reinterpret_cast<const u64*>(edge_label);
    const u64* cin = reinterpret_cast<const u64*>(colors_in);
    u64* cout = reinterpret_cast<u64*>(colors_out);
    hipStream_t st = (hipStream_t)stream;
    if (group == 0) {
        DN_REQUIRE(lds_entries >= 1 && lds_entries <= kMaxEntries && (lds_entries & (lds_entries - 1)) == 0,
                   "dn_wl_refine: lds_entries must be a power of two <= %d (got %d)", kMaxEntries, lds_entries);
        hipLaunchKernelGGL(wl_refine_block_kernel, dim3((unsigned)num_list), dim3(kBlock), (size_t)lds_entries * sizeof(u64), st, nodes,
                           lds_entries, ptr, nbr, el, cin, cout);
    } else {
        const int64_t blocks = dn_cdiv(num_list * group, kBlock);
        DN_REQUIRE(blocks <= 0x7fffffffLL, "dn_wl_refine: bad sizes");
        if (group == 8)
            hipLaunchKernelGGL(wl_refine_group_kernel<8>, dim3((unsigned)blocks), dim3(kBlock), 0, st, num_list, nodes, ptr, nbr, el, cin, cout);
        else
            hipLaunchKernelGGL(wl_refine_group_kernel<64>, dim3((unsigned)blocks), dim3(kBlock), 0, st, num_list, nodes, ptr, nbr, el, cin, cout);
    }
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_wl_fold_u64(int64_t num_nodes, int64_t num_list, const int32_t* nodes, const int64_t* seg_ptr, const int64_t* sorted_entries,
                   const int64_t* colors_in, int64_t* colors_out, dn_stream_t stream) {
    DN_REQUIRE(fits_i32(num_nodes) && fits_i32(num_list) && num_list <= num_nodes, "dn_wl_fold: bad sizes");
    DN_REQUIRE(seg_ptr && colors_in && colors_out, "dn_wl_fold: NULL pointer");       // (sorted_entries may be NULL: no entries at all)
    DN_REQUIRE(nodes || num_list == num_nodes, "dn_wl_fold: NULL pointer (a node list is needed unless it is every node)");
    DN_REQUIRE(colors_in != colors_out, "dn_wl_fold: colors_out must not alias colors_in");
    hipLaunchKernelGGL(wl_fold_kernel, dim3((unsigned)dn_cdiv(num_list, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, num_list, nodes,
                       seg_ptr, reinterpret_cast<const u64*>(sorted_entries), reinterpret_cast<const u64*>(colors_in),
                       reinterpret_cast<u64*>(colors_out));
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_wl_gram_i64(int64_t num_graphs, int32_t num_steps, int32_t use_min, const int32_t* feat_ptr, const int64_t* feat_color,
                   const int32_t* feat_count, const int32_t* feat_step, int64_t* out, dn_stream_t stream) {
    DN_REQUIRE(fits_i32(num_graphs) && dn_cdiv(num_graphs, kTile) <= 65535, "dn_wl_gram: bad sizes (1 <= graphs <= %d)", 65535 * kTile);
    DN_REQUIRE(num_steps >= 1 && num_steps <= kMaxSteps, "dn_wl_gram: 1 <= steps <= %d (got %d)", kMaxSteps, num_steps);
    DN_REQUIRE(feat_ptr && feat_color && feat_count && feat_step && out, "dn_wl_gram: NULL pointer");
    const size_t lds = (size_t)num_steps * kBlock * sizeof(int64_t);
    const unsigned T = (unsigned)dn_cdiv(num_graphs, kTile);
    const u64* col = reinterpret_cast<const u64*>(feat_color);
    if (use_min)
        hipLaunchKernelGGL(wl_gram_kernel<true>, dim3(T, T), dim3(kBlock), lds, (hipStream_t)stream, (int32_t)num_graphs, num_steps, feat_ptr,
                           col, feat_count, feat_step, out);
    else
        hipLaunchKernelGGL(wl_gram_kernel<false>, dim3(T, T), dim3(kBlock), lds, (hipStream_t)stream, (int32_t)num_graphs, num_steps, feat_ptr,
                           col, feat_count, feat_step, out);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

}  // extern "C"
