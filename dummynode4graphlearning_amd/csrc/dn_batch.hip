// Mini-batch assembly from a device-resident dataset (dn_batch_assemble): the collate of every training step -- PyG's
// Batch.from_data_list behind DataLoader (graph_classification/graph_neural_networks/main.py:245-247), batchify -> dgl.batch
// (subgraph_isomorphism/dataset.py:1321-1328, 1605-1611) -- as ONE launch: a batched ragged copy with optional integer re-basing.
//
// Work is cut over OUTPUT BYTES, not over graphs: every column's destination, seen from the 16-byte boundary at or below its first
// byte, is a run of 16-byte units; a workgroup takes kChunk bytes of one column, a thread one unit at a time.  A unit finds the
// graph of its first byte by a binary search in the batch's row pointers (narrowed to the chunk's graphs by two searches per
// workgroup) and then takes one of two roads:
//   whole unit inside one graph  -> 16 source bytes in the widest pieces the SOURCE address allows (16 / 4 / 2 / 1; the two
//                                   sides generally differ modulo 16), one 16-byte store;
//   a column's head or tail, or a unit that spans graphs -> element by element (1 byte, or one integer of a re-based column),
//                                   walking the graph boundaries, empty graphs included.
// Nothing outside [src range of the graph] / [dst range of the column] is touched: a partial unit is never read or written whole.
// A graph with an id outside the dataset, or whose planned size is not the dataset's, is left out.  No atomics, no workspace.
#include "dn_common.h"
#include "../../include/dn_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kUnitsPerThread = 2;
constexpr int64_t kChunk = (int64_t)kThreads * 16 * kUnitsPerThread;      // destination bytes of one workgroup

enum { kCopy = 0, kRebase = 1, kFill = 2 };

struct BaCol {
    const char* src;
    char* dst;
    int64_t total;                                 // bytes of the column in the batch
    int32_t row_bytes, level, mode, rebase, width, src_global, ptr_tail;
    int32_t a0;                                    // dst & 15: the column starts a0 bytes into its first unit
};

struct BaArgs {
    BaCol col[DN_BATCH_MAX_COLS + 1];              // (+ 1: the `batch` vector)
    int64_t chunk0[DN_BATCH_MAX_COLS + 2];         // first workgroup of column c; [ncols] = all of them
    int32_t ncols;
};

struct BaTables {
    const int32_t *ids, *out_node_ptr, *out_edge_ptr, *ds_node_ptr, *ds_edge_ptr;
    int32_t B, G, N, E;
};

// the rows of output graph k in one column, as destination bytes [g_lo, g_hi), and what its bytes turn into
struct BaGraph {
    int64_t g_lo, g_hi;
    int64_t s_off;                                 // source byte of destination byte o = o + s_off
    int64_t delta;                                 // kRebase: added to every value; kFill: the value
    bool ok;
};

__device__ __forceinline__ int64_t ba_out_row(const BaCol& c, const BaTables& t, int32_t k) {
    return c.level == DN_BATCH_LEVEL_GRAPH ? (int64_t)k : (int64_t)(c.level == DN_BATCH_LEVEL_NODE ? t.out_node_ptr : t.out_edge_ptr)[k];
}

__device__ __forceinline__ BaGraph ba_graph(const BaCol& c, const BaTables& t, int32_t k) {
    BaGraph g;
    const int64_t o0 = ba_out_row(c, t, k), o1 = ba_out_row(c, t, k + 1);
    g.g_lo = o0 * c.row_bytes;
    g.g_hi = o1 * c.row_bytes;
    g.s_off = 0;
    g.delta = k;
    const int32_t i = t.ids[k];
    g.ok = (uint32_t)i < (uint32_t)t.G;
    if (g.ok && c.mode != kFill) {
        int64_t d0 = i, d1 = (int64_t)i + 1;
        if (c.level != DN_BATCH_LEVEL_GRAPH) {
            const int32_t* dp = c.level == DN_BATCH_LEVEL_NODE ? t.ds_node_ptr : t.ds_edge_ptr;
            d0 = dp[i];
            d1 = dp[i + 1];
        }
        g.ok = d0 >= 0 && d1 - d0 == o1 - o0;
        g.s_off = d0 * c.row_bytes - g.g_lo;
        if (c.mode == kRebase) {
            const bool node = c.rebase == DN_BATCH_REBASE_NODE;
            const int64_t base_out = (node ? t.out_node_ptr : t.out_edge_ptr)[k];
            const int64_t base_in = c.src_global ? (int64_t)(node ? t.ds_node_ptr : t.ds_edge_ptr)[i] : 0;
            g.delta = base_out - base_in;
        }
    }
    return g;
}

// the last k in [lo, hi] whose rows start at or before row r (r < the column's rows, so that graph holds row r)
__device__ __forceinline__ int32_t ba_find(const BaCol& c, const BaTables& t, int64_t r, int32_t lo, int32_t hi) {
    if (c.level == DN_BATCH_LEVEL_GRAPH) return (int32_t)r;
    const int32_t* op = c.level == DN_BATCH_LEVEL_NODE ? t.out_node_ptr : t.out_edge_ptr;
    while (lo < hi) {
        const int32_t mid = (int32_t)(((int64_t)lo + hi + 1) >> 1);
        if ((int64_t)op[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ int64_t ba_row_of(const BaCol& c, int64_t o) {
    return c.total < (int64_t)0xffffffffLL ? (int64_t)((uint32_t)o / (uint32_t)c.row_bytes) : o / c.row_bytes;
}

// 16 bytes from an address of any alignment, all of them inside the source range
__device__ __forceinline__ uint4 ba_load16(const char* p) {
    const uintptr_t a = (uintptr_t)p;
    if ((a & 15) == 0) return *reinterpret_cast<const uint4*>(p);
    uint32_t w[4];
    if ((a & 3) == 0) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = q[j];
    } else if ((a & 1) == 0) {
        const uint16_t* q = reinterpret_cast<const uint16_t*>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = (uint32_t)q[2 * j] | ((uint32_t)q[2 * j + 1] << 16);
    } else {
        const uint8_t* q = reinterpret_cast<const uint8_t*>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            w[j] = (uint32_t)q[4 * j] | ((uint32_t)q[4 * j + 1] << 8) | ((uint32_t)q[4 * j + 2] << 16) | ((uint32_t)q[4 * j + 3] << 24);
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ __launch_bounds__(kThreads) void batch_assemble_kernel(const BaArgs a, const BaTables t) {
    const int64_t b = blockIdx.x;
    const int tid = (int)threadIdx.x;
    if (b >= a.chunk0[a.ncols]) {                  // the one workgroup behind the chunks: closing entries of the pointer columns
        if (tid == 0) {
            for (int c = 0; c < a.ncols; ++c) {
                const BaCol& col = a.col[c];
                if (!col.ptr_tail) continue;
                const int64_t v = col.rebase == DN_BATCH_REBASE_NODE ? t.N : t.E;
                if (col.width == 4) *reinterpret_cast<int32_t*>(col.dst + col.total) = (int32_t)v;
                else *reinterpret_cast<int64_t*>(col.dst + col.total) = v;
            }
        }
        return;
    }
    int ci = 0;
    while (b >= a.chunk0[ci + 1]) ++ci;
    const BaCol& c = a.col[ci];
    // the chunk in "virtual" bytes: v = a0 + (byte of the column), so that v = 0 (mod 16) is a 16-byte boundary of dst
    const int64_t v_beg = (b - a.chunk0[ci]) * kChunk, v_stop = c.a0 + c.total;
    const int64_t v_end = v_beg + kChunk < v_stop ? v_beg + kChunk : v_stop;
    __shared__ int32_t s_k[2];
    if (tid < 2) {                                 // the graphs of the chunk's first and last byte bound every search below
        const int64_t o = tid == 0 ? (v_beg > c.a0 ? v_beg - c.a0 : 0) : v_end - 1 - c.a0;
        s_k[tid] = ba_find(c, t, ba_row_of(c, o), 0, t.B - 1);
    }
    __syncthreads();
    const int32_t k_lo = s_k[0], k_hi = s_k[1];
    const int64_t step = c.mode == kCopy ? 1 : c.width;
#pragma unroll 1
    for (int q = 0; q < kUnitsPerThread; ++q) {
        const int64_t vu = v_beg + 16 * (int64_t)(tid + kThreads * q);
        const int64_t lo = vu > c.a0 ? vu : c.a0, hi = vu + 16 < v_end ? vu + 16 : v_end;
        if (lo >= hi) continue;
        int64_t o = lo - c.a0;
        const int64_t o_hi = hi - c.a0;
        int32_t k = ba_find(c, t, ba_row_of(c, o), k_lo, k_hi);
        BaGraph g = ba_graph(c, t, k);
        if (o_hi - o == 16 && o >= g.g_lo && o_hi <= g.g_hi) {    // a whole unit of one graph: dst + o is 16-byte aligned
            if (!g.ok) continue;
            uint4 v;
            if (c.mode == kFill) {
                v = make_uint4((uint32_t)g.delta, (uint32_t)((uint64_t)g.delta >> 32), (uint32_t)g.delta, (uint32_t)((uint64_t)g.delta >> 32));
            } else {
                v = ba_load16(c.src + o + g.s_off);
                if (c.mode == kRebase) {
                    if (c.width == 4) {
                        const uint32_t d = (uint32_t)g.delta;
                        v.x += d; v.y += d; v.z += d; v.w += d;
                    } else {
                        const uint64_t e0 = ((uint64_t)v.y << 32 | v.x) + (uint64_t)g.delta, e1 = ((uint64_t)v.w << 32 | v.z) + (uint64_t)g.delta;
                        v = make_uint4((uint32_t)e0, (uint32_t)(e0 >> 32), (uint32_t)e1, (uint32_t)(e1 >> 32));
                    }
                }
            }
            *reinterpret_cast<uint4*>(c.dst + o) = v;
            continue;
        }
        for (; o < o_hi; o += step) {              // head / tail of the column, or a unit that spans graphs
            while (o >= g.g_hi && k + 1 < t.B) g = ba_graph(c, t, ++k);      // (empty graphs are passed)
            if (!g.ok || o < g.g_lo || o >= g.g_hi) continue;             // (a table that does not add up to N / E: nothing is read)
            if (c.mode == kCopy) {
                c.dst[o] = c.src[o + g.s_off];
            } else if (c.width == 4) {
                const int32_t x = c.mode == kFill ? 0 : *reinterpret_cast<const int32_t*>(c.src + o + g.s_off);
                *reinterpret_cast<int32_t*>(c.dst + o) = (int32_t)((uint32_t)x + (uint32_t)g.delta);
            } else {
                const int64_t x = c.mode == kFill ? 0 : *reinterpret_cast<const int64_t*>(c.src + o + g.s_off);
                *reinterpret_cast<int64_t*>(c.dst + o) = (int64_t)((uint64_t)x + (uint64_t)g.delta);
            }
        }
    }
}

}  // namespace

int dn_batch_assemble(int64_t B, const int32_t* table, const int32_t* ds_node_ptr, const int32_t* ds_edge_ptr, int64_t num_ds_graphs,
                      int64_t N, int64_t E, const dn_batch_col* host_cols, int32_t num_cols, int64_t* batch_out, dn_stream_t stream) {
    const int64_t lim = (int64_t)1 << 31;
    DN_REQUIRE(B >= 0 && N >= 0 && E >= 0 && num_ds_graphs >= 0 && num_cols >= 0 && B < lim - 1 && N < lim && E < lim && num_ds_graphs < lim - 1,
               "dn_batch_assemble: bad sizes");
    DN_REQUIRE(num_cols <= DN_BATCH_MAX_COLS, "dn_batch_assemble: too many columns (%d, at most %d)", (int)num_cols, DN_BATCH_MAX_COLS);
    if (B == 0) return DN_OK;
    DN_REQUIRE(table && ds_node_ptr && ds_edge_ptr && (num_cols == 0 || host_cols), "dn_batch_assemble: NULL pointer");
    BaArgs a;
    a.ncols = 0;
    a.chunk0[0] = 0;
    bool tails = false;
    for (int32_t i = 0; i <= num_cols; ++i) {
        BaCol c;
        if (i < num_cols) {
            const dn_batch_col& h = host_cols[i];
            DN_REQUIRE(h.row_bytes >= 1 && h.level >= DN_BATCH_LEVEL_NODE && h.level <= DN_BATCH_LEVEL_GRAPH &&
                           h.rebase >= DN_BATCH_REBASE_NONE && h.rebase <= DN_BATCH_REBASE_EDGE,
                       "dn_batch_assemble: bad sizes (column %d: row_bytes / level / rebase)", (int)i);
            const bool rb = h.rebase != DN_BATCH_REBASE_NONE;
            DN_REQUIRE(!rb || ((h.int_width == 4 || h.int_width == 8) && h.row_bytes % h.int_width == 0 && h.level != DN_BATCH_LEVEL_GRAPH),
                       "dn_batch_assemble: bad sizes (column %d: a re-based column holds 4- or 8-byte integers of a node or edge level)", (int)i);
            DN_REQUIRE(rb || !h.ptr_tail, "dn_batch_assemble: bad sizes (column %d: ptr_tail needs a re-based column)", (int)i);
            const int64_t rows = h.level == DN_BATCH_LEVEL_NODE ? N : (h.level == DN_BATCH_LEVEL_EDGE ? E : B);
            DN_REQUIRE((rows == 0 || (h.src && h.dst)) && (!h.ptr_tail || h.dst), "dn_batch_assemble: NULL pointer");
            DN_REQUIRE(!rb || (((uintptr_t)h.src | (uintptr_t)h.dst) & (uintptr_t)(h.int_width - 1)) == 0,
                       "dn_batch_assemble: column %d is not aligned to its integers", (int)i);
            c.src = (const char*)h.src; c.dst = (char*)h.dst;
            c.total = rows * h.row_bytes;
            c.row_bytes = h.row_bytes; c.level = h.level; c.mode = rb ? kRebase : kCopy; c.rebase = h.rebase;
            c.width = rb ? h.int_width : 1; c.src_global = h.src_global ? 1 : 0; c.ptr_tail = h.ptr_tail ? 1 : 0;
        } else {
            if (batch_out == nullptr || N == 0) break;
            DN_REQUIRE(((uintptr_t)batch_out & 7) == 0, "dn_batch_assemble: batch_out is not aligned to its integers");
            c.src = nullptr; c.dst = (char*)batch_out;
            c.total = N * 8;
            c.row_bytes = 8; c.level = DN_BATCH_LEVEL_NODE; c.mode = kFill; c.rebase = DN_BATCH_REBASE_NONE;
            c.width = 8; c.src_global = 0; c.ptr_tail = 0;
        }
        c.a0 = (int32_t)((uintptr_t)c.dst & 15);
        tails = tails || c.ptr_tail;
        a.col[a.ncols] = c;
        a.chunk0[a.ncols + 1] = a.chunk0[a.ncols] + (c.total > 0 ? dn_cdiv(c.a0 + c.total, kChunk) : 0);
        ++a.ncols;
    }
    const int64_t grid = a.chunk0[a.ncols] + (tails ? 1 : 0);
    DN_REQUIRE(grid < lim, "dn_batch_assemble: bad sizes (more than 2^31 workgroups)");
    if (grid == 0) return DN_OK;
    BaTables t;
    t.ids = table; t.out_node_ptr = table + B; t.out_edge_ptr = table + 2 * B + 1;
    t.ds_node_ptr = ds_node_ptr; t.ds_edge_ptr = ds_edge_ptr;
    t.B = (int32_t)B; t.G = (int32_t)num_ds_graphs; t.N = (int32_t)N; t.E = (int32_t)E;
    hipLaunchKernelGGL(batch_assemble_kernel, dim3((unsigned)grid), dim3(kThreads), 0, (hipStream_t)stream, a, t);
    DN_CHECK_LAUNCH();
    return DN_OK;
}
