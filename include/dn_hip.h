/* dn_hip.h -- C ABI of libdn_hip.so: the MI355X (gfx950) hot path of
 * HKUST-KnowComp/DummyNode4GraphLearning (dummy-node / edge-to-vertex index builds and the
 * gather -> segment-reduce message passing of the GIN / RGCN / RGIN layers).
 *
 * The reference has NO C/FFI interface for this path: the arithmetic runs inside third-party
 * engines (DGL update_all / torch-scatter) behind Python nn.Modules.  The entry
 * points below are therefore exactly what a ctypes binding on the reference side would bind in
 * place of those engine calls; each one cites the reference call site it replaces
 * (paths relative to the reference root).  INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - plain pointers + sizes only; every pointer is a DEVICE pointer unless named host_*.
 *   - the caller (PyTorch) owns every buffer: inputs, outputs and workspace; the library never
 *     allocates, frees or retains a pointer.  Workspace sizes come from *_workspace_bytes().
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing else orders it.
 *   - return 0 on success, <0 on error (DN_ERR_*); dn_last_error() gives the thread-local message.
 *   - re-entrant, no global mutable state, no environment access of its own (the experiment knobs of the kernels are
 *     compile-time constants; only a -DDN_TUNING_ENV build reads DN_* variables.  rocPRIM, which the index builds call,
 *     consults the environment for its own target selection), deterministic: no floating-point atomics anywhere,
 *     every sum has a fixed order (bitwise reproducible run to run).
 *   - node / edge ids are int32 on the device (N, E < 2^31); the Python boundary converts the
 *     reference's int64 ids.
 *   - feature matrices are row-major [rows, H]; `_f32` = float, `_bf16` = bfloat16 storage with
 *     fp32 accumulation.
 */
#ifndef DN_HIP_H
#define DN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DN_OK 0
#define DN_ERR_ARG (-1)
#define DN_ERR_HIP (-2)
#define DN_ERR_WORKSPACE (-3)
#define DN_ERR_UNSUPPORTED (-4)

typedef void* dn_stream_t; /* hipStream_t */

int dn_version(void);
const char* dn_last_error(void);
/* Returns 0 iff `device_ptr` is device memory known to the HIP runtime this library resolved to
 * (guards against a second libamdhip64 being loaded next to PyTorch's). */
int dn_runtime_probe(const void* device_ptr);

/* ------------------------------------------------------------------------------------------
 * Gather + segment-sum (the message-passing core).
 *   out[s,:] = self_coef * self_in[s,:] + sum_{i in [ptr[s], ptr[s+1])} scale[i] * in[idx[i],:]
 * idx == NULL -> idx[i] = i;  ptr == NULL -> segment s = {s} (pure row gather, S == M);
 * scale == NULL -> 1;  self_in == NULL -> no self term.  M = number of gathered elements.
 * mean != 0 divides the gathered sum (not the self term) by the segment length (0 for empty segments).
 * Replaces: PyG GINConv.propagate / RGCNConv.propagate = x.index_select(0, src) + torch_scatter
 *   (graph_classification/graph_neural_networks/models/gconv.py:212, rgconv.py:40-41,121) and
 *   DGL update_all(msg, fn.sum) (subgraph_isomorphism/models/rgin.py:159, rgcn.py:196).
 * The backward of this operator w.r.t. `in` is the same call on the transposed index.
 * ------------------------------------------------------------------------------------------ */
int dn_gather_segsum_f32(const float* in, int64_t in_rows, int32_t H, const int32_t* idx,
                         const float* scale, const int32_t* ptr, int64_t S, int64_t M, float* out,
                         const float* self_in, float self_coef, int32_t mean, dn_stream_t stream);
int dn_gather_segsum_bf16(const void* in, int64_t in_rows, int32_t H, const int32_t* idx,
                          const float* scale, const int32_t* ptr, int64_t S, int64_t M, void* out,
                          const void* self_in, float self_coef, int32_t mean, dn_stream_t stream);

/* Per-graph readouts over CONTIGUOUS rows: out[g,:] = reduce_{v in [ptr[g], ptr[g+1])} in[v,:].
 * Replaces: torch_geometric global_add_pool / global_mean_pool / global_max_pool
 *   (gconv.py:53,95,148,210,213; rgconv.py:42,119,124) and SI SumPredictNet's sum over the padded
 *   node dimension (subgraph_isomorphism/models/pred.py:215-216).
 * mean: empty segments give 0.  max: empty segments give 0 and argmax -1; ties keep the lowest row
 *   (argmax [S,H] int32 is the row index, used by dn_segment_max_bwd_*). */
int dn_segment_sum_f32(const float* in, int32_t H, const int32_t* ptr, int64_t S, float* out, dn_stream_t stream);
int dn_segment_sum_bf16(const void* in, int32_t H, const int32_t* ptr, int64_t S, void* out, dn_stream_t stream);
int dn_segment_mean_f32(const float* in, int32_t H, const int32_t* ptr, int64_t S, float* out, dn_stream_t stream);
int dn_segment_mean_bf16(const void* in, int32_t H, const int32_t* ptr, int64_t S, void* out, dn_stream_t stream);
int dn_segment_max_f32(const float* in, int32_t H, const int32_t* ptr, int64_t S, float* out, int32_t* argmax,
                       dn_stream_t stream);
int dn_segment_max_bf16(const void* in, int32_t H, const int32_t* ptr, int64_t S, void* out, int32_t* argmax,
                        dn_stream_t stream);
/* grad_in[v,h] = (argmax[g(v),h] == v) ? grad_out[g(v),h] : 0, rows of segment g contiguous. */
int dn_segment_max_bwd_f32(const float* grad_out, const int32_t* argmax, int32_t H, const int32_t* ptr, int64_t S,
                           float* grad_in, dn_stream_t stream);
int dn_segment_max_bwd_bf16(const void* grad_out, const int32_t* argmax, int32_t H, const int32_t* ptr, int64_t S,
                            void* grad_in, dn_stream_t stream);

/* Per-edge dot product (SDDMM): out[e] = < a[ia[e], :], b[ib[e], :] >, fp32 out; ia / ib may be NULL (row e).
 * The gradient of a per-edge scalar weight w_e in  out[dst] += w_e * x[src]  is < x[src_e], grad_out[dst_e] >: this
 * is what lets the reference's trainable dummy-edge weight (gconv.py:29-34,46-49: edge_attr[is_dummy_edge] =
 * dummy_weight, passed to GCNConv) receive its gradient without PyG's autograd through index_select / scatter. */
int dn_edge_dot_f32(const float* a, const int32_t* ia, const float* b, const int32_t* ib, int32_t H, int64_t E,
                    float* out, dn_stream_t stream);
int dn_edge_dot_bf16(const void* a, const int32_t* ia, const void* b, const int32_t* ib, int32_t H, int64_t E,
                     float* out, dn_stream_t stream);

/* Gather + segment MAX: out[s, h] = max_{i in [ptr[s], ptr[s+1])} in[idx[i], h]; argmax[s, h] = that slot i (-1 and
 * out 0 for an empty segment; ties keep the lowest slot).  Replaces PyG SAGEConv's 'max' neighbour aggregation
 * (gconv.py:130-132 `conv.aggr = self.aggregation`).  Backward: grad_in[u, h] = sum over the slots i that gathered
 * row u (tptr [rows+1], tslot: slots grouped by gathered row; seg_of_slot [M]) of
 * (argmax[seg(i), h] == i ? grad_out[seg(i), h] : 0) -- a gather over the transposed index, no atomics. */
int dn_gather_segmax_f32(const float* in, const int32_t* idx, const int32_t* ptr, int64_t S, int32_t H, float* out,
                         int32_t* argmax, dn_stream_t stream);
int dn_gather_segmax_bf16(const void* in, const int32_t* idx, const int32_t* ptr, int64_t S, int32_t H, void* out,
                          int32_t* argmax, dn_stream_t stream);
int dn_gather_segmax_bwd_f32(const float* grad_out, const int32_t* argmax, const int32_t* tptr, const int32_t* tslot,
                             const int32_t* seg_of_slot, int64_t rows, int32_t H, float* grad_in, dn_stream_t stream);
int dn_gather_segmax_bwd_bf16(const void* grad_out, const int32_t* argmax, const int32_t* tptr, const int32_t* tslot,
                              const int32_t* seg_of_slot, int64_t rows, int32_t H, void* grad_in, dn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * One-shot device-side index builds.
 * ------------------------------------------------------------------------------------------ */

/* Stable grouping of element indices by integer key in [0, num_keys):
 *   ptr[k] .. ptr[k+1] = positions in `perm` of the elements with key k, ascending element index.
 * This is the CSR/CSC build DGL / torch-scatter perform internally for the call sites above. */
size_t dn_csr_build_workspace_bytes(int64_t M, int64_t num_keys);
int dn_csr_build_i32(const int32_t* key, int64_t M, int64_t num_keys, int32_t* ptr /*[num_keys+1]*/,
                     int32_t* perm /*[M]*/, void* workspace, size_t workspace_bytes, dn_stream_t stream);

/* Dummy-node augmentation of a batched graph (disjoint union; node_ptr/edge_ptr [G+1]; src/dst global
 * ids; edges of a graph contiguous in eid order).  Outputs: N' = N + G nodes, E' = E + 2N edges.
 * GC layout -- replaces load_graph_data_from_TUDatadir(with_dummy=True)'s per-graph igraph build
 *   (graph_classification/data_processing/tu_data_processing.py:186-200,213-214): dummy vertex n with
 *   label 0; edges = m originals then INTERLEAVED (n,v),(v,n), label 0, IS_DUMMY 1; ids = local index. */
int dn_dummy_augment_gc_i32(int64_t G, int64_t N, int64_t E, const int32_t* node_ptr, const int32_t* edge_ptr,
                            const int32_t* src, const int32_t* dst, const int32_t* node_label,
                            const int32_t* edge_label, int32_t* out_node_ptr, int32_t* out_edge_ptr,
                            int32_t* out_src, int32_t* out_dst, int32_t* out_node_label, int32_t* out_edge_label,
                            uint8_t* out_is_dummy_node, uint8_t* out_is_dummy_edge, int32_t* out_node_id,
                            int32_t* out_edge_id, dn_stream_t stream);
/* SI layout -- replaces add_dummy_nodes_edges, GraphAdj branch (subgraph_isomorphism/train.py:404-474):
 *   dummy node (id = max_nv, label = max_nvl); 2n edges BLOCKED: all (u -> dummy) then all (dummy -> u);
 *   edge id max_ne / max_ne+1; relation max_nel / max_nel+1; is_dummy 1; is_reversed 0 / 1.
 *   in_is_reversed may be NULL (treated as 0). */
int dn_dummy_augment_si_i32(int64_t G, int64_t N, int64_t E, const int32_t* node_ptr, const int32_t* edge_ptr,
                            const int32_t* src, const int32_t* dst, const int32_t* node_id,
                            const int32_t* node_label, const int32_t* edge_id, const int32_t* edge_label,
                            const uint8_t* in_is_reversed, int32_t max_nv, int32_t max_nvl, int32_t max_ne,
                            int32_t max_nel, int32_t* out_node_ptr, int32_t* out_edge_ptr, int32_t* out_src,
                            int32_t* out_dst, int32_t* out_node_id, int32_t* out_node_label,
                            int32_t* out_edge_id, int32_t* out_edge_label, uint8_t* out_is_dummy_node,
                            uint8_t* out_is_dummy_edge, uint8_t* out_is_reversed, dn_stream_t stream);

/* Edge-to-vertex ("conjugate") transform L_Phi of a batched graph.
 * Replaces convert_conjugate_graph_forward (tu_data_processing.py:223-338; mode DN_CONJ_GC, and
 * DN_CONJ_LINE for graphs without the IS_DUMMY attribute) and convert_conjugate_graph, igraph branch
 * (subgraph_isomorphism/utils/graph.py:177-267; mode DN_CONJ_SI).  Bit-exact incl. output order.
 *   step 1  dn_conjugate_count_i32: *host_num_raw = sum_e in_deg(src(e)) (synchronises the stream).
 *   step 2  dn_conjugate_build_i32: outputs sized by the upper bounds N'<=E, E'<=num_raw;
 *           host_counts[0] = N' (conj vertices), host_counts[1] = E' (conj edges) (synchronises).
 *   rep_edge[k]    input edge whose attributes conj-vertex k copies (first edge carrying that id)
 *   shared_node[t] input vertex whose attributes conj-edge t copies (the vertex the 2-path goes through)
 *   edge_id: per-graph edge ids (SI: edata["id"], dummies share ids); NULL = local edge index (GC). */
#define DN_CONJ_GC 0
#define DN_CONJ_SI 1
#define DN_CONJ_LINE 2
/* num_raw = -1 sizes the workspace for the count step only. */
size_t dn_conjugate_workspace_bytes(int64_t G, int64_t N, int64_t E, int64_t num_raw);
int dn_conjugate_count_i32(int64_t N, int64_t E, const int32_t* src, const int32_t* dst, int64_t* host_num_raw,
                           void* workspace, size_t workspace_bytes, dn_stream_t stream);
int dn_conjugate_build_i32(int32_t mode, int64_t G, int64_t N, int64_t E, int64_t num_raw,
                           const int32_t* node_ptr, const int32_t* edge_ptr, const int32_t* src,
                           const int32_t* dst, const int32_t* node_label, const int32_t* edge_id,
                           const uint8_t* is_dummy_edge, int32_t* out_cnode_ptr /*[G+1]*/,
                           int32_t* out_cedge_ptr /*[G+1]*/, int32_t* out_csrc /*[num_raw]*/,
                           int32_t* out_cdst /*[num_raw]*/, int32_t* out_rep_edge /*[E]*/,
                           int32_t* out_shared_node /*[num_raw]*/, int64_t* host_counts /*[2]*/,
                           void* workspace, size_t workspace_bytes, dn_stream_t stream);

/* Graph-local neighbour sum on the matrix cores, for the rows of the listed tiles only:
 *   out[v, :] = self_coef * x[v, :] + sum_{i in [ptr[v], ptr[v+1])} x[idx[i], :]
 * -- GINConv's aggregation (graph_classification/graph_neural_networks/models/gconv.py:197: PyG propagate(aggr="add") plus
 * (1 + eps) x_i) and, on the transposed index, its input gradient.  tiles [num_tiles][4] = {first row, end row, ptr[first row],
 * ptr[end row]} of runs of WHOLE graphs with at most 64 rows each; seg (may be NULL) = the row every index entry belongs to
 * (saves a search in the tile's bounds): every idx of a tile's rows must lie inside the tile (else *bad |= 1 and that entry is
 * skipped; tiles that leave [0, num_rows) or hold more than 64 rows are flagged the same way and not touched; *bad must be
 * zeroed by the caller).  x / out have num_rows rows, idx num_entries entries.  A tile's rows are read once, split into three bf16 planes (hi + mid + lo = the
 * fp32 value to rounding), the tile's adjacency counts form a bf16 matrix in LDS and the sum is a dense product with fp32
 * accumulation: same value as dn_gather_segsum_f32 up to fp32 summation order for FINITE inputs; a non-finite element turns its
 * column of the whole tile into NaN (0 x Inf in the dense product, Inf - Inf in the split), where the gather would pass it to its
 * neighbours only.  fp32 rows, H in {64, 128, 256}. */
int dn_graph_tile_sum_f32(const float* x, int64_t num_rows, int32_t H, const int32_t* ptr, const int32_t* idx,
                          const int32_t* seg, int64_t num_entries, const int32_t* tiles, int64_t num_tiles,
                          float self_coef, float* out, int32_t* bad, dn_stream_t stream);

/* The same sum for a LIST of rows, straight from the full CSR (no compacted copy of lists or rows): the companion of
 * dn_graph_tile_sum_f32 for the rows of graphs too large for a tile.  rows [num_listed]: row ids (rows_are_records = 0) or
 * 16-byte records {row, ptr[row], ptr[row + 1], 0} (rows_are_records = 1: saves the ptr round trip), each row listed once; any
 * list length (an empty list gives self_coef * x[s]).  workgroup_per_row = 0: one lane group per
 * listed row; 1: one workgroup per listed row, its lane groups sharing the list (hubs: hundreds of entries), partial rows added
 * in fixed order.  Rows not listed are left untouched.  Replaces the same PyG aggregation (gconv.py:197). */
int dn_gather_rows_sum_f32(const float* x, int32_t H, const int32_t* ptr, const int32_t* idx, const int32_t* rows,
                           int32_t rows_are_records, int64_t num_listed, int32_t workgroup_per_row, float self_coef,
                           float* out, dn_stream_t stream);

/* Host-side tile packing for dn_graph_tile_sum_f32 (no GPU): greedy runs of whole graphs with at most max_rows rows each
 * (node_ptr [G+1] on the HOST); graphs with more rows are left out (their rows go to dn_gather_rows_sum_f32).  tiles receives
 * {first row, end row} pairs, *num_tiles their number; DN_ERR_WORKSPACE when cap pairs do not suffice (G always do). */
int dn_graph_tiles_host(const int32_t* node_ptr, int64_t G, int32_t max_rows, int32_t* tiles, int64_t cap, int64_t* num_tiles);

/* Relation-aware segment index for the aggregate-then-transform form of the RGCN/RGIN message pass
 *   sum_e x[src_e] W[etype_e]  ==  sum_r ( sum_{e in r, dst=v} x[src_e] ) W_r      
 * which replaces the reference's per-edge weight gather + bmm (subgraph_isomorphism/models/rgin.py:102-120,
 * rgcn.py:100-122) and PyG RGCNConv's per-relation mask/propagate loop (rgconv.py:17-18,96).
 * Segments p = distinct (rel, dst) pairs, ordered by (rel, dst); P = number of segments (<= E).
 *   perm1 [E]      edge ids sorted by (rel, dst), stable;  src1 [E] = src[perm1]
 *   seg_ptr [P+1]  (allocate E+1) edge range of each segment in perm1 order;  seg_dst [P] (allocate E)
 *   rel_ptr [R+1]  segment range of each relation (also copied to host_rel_ptr)
 *   dptr [N+1], sperm [P] (allocate E)   segments grouped by destination, ascending relation
 *   optr [N+1], operm [E]                edges grouped by source, ascending edge id
 *   seg_by_src [E]                       segment of edge operm[i]
 * Synchronises the stream (P and rel_ptr are returned to the host). */
size_t dn_rel_index_workspace_bytes(int64_t N, int64_t R, int64_t E);
int dn_rel_index_build_i32(int64_t N, int64_t R, int64_t E, const int32_t* src, const int32_t* dst,
                           const int32_t* etype, int32_t* perm1, int32_t* src1, int32_t* seg_ptr,
                           int32_t* seg_dst, int32_t* rel_ptr, int32_t* dptr, int32_t* sperm, int32_t* optr,
                           int32_t* operm, int32_t* seg_by_src, int64_t* host_P, int32_t* host_rel_ptr,
                           void* workspace, size_t workspace_bytes, dn_stream_t stream);

/* Row factorisation of the relation-wise message pass for the bf16 matrix-core path:
 *   out[v] = sum_{e: dst(e)=v} x[src(e)] W[etype(e)]   ==   sum over rows p with v in out(p) of  in_row(p) @ W[rel(p)]
 * Every row has ONE input row.  Per relation r (E_r edges, D_r distinct destinations, S_r distinct sources):
 *   EDGE (min(D_r,S_r) > edge_frac*E_r): one row per edge, in = x[src], out -> dst
 *   AGG  (D_r <= S_r): one row per distinct dst, in = N + a (a-th pre-aggregated row: sum of x[src] over the segment), out -> dst
 *   TF   (else):       one row per distinct src, in = x[src], out = N + b (the b-th backward pre-aggregated row) and the
 *                       product is added to every dst of that (rel, src)
 * Edge rows are relation-major (host_rel_ptr [R+1]); with self_loop != 0, N more rows (relation R, in = out = v) follow.
 * Outputs (device, caller-allocated upper bounds): row_in / row_out [E+N]; aux_f_ptr [E+1], aux_f_idx [E] (lists of x
 * rows per AGG row); aux_b_ptr [E+1], aux_b_idx [E] (lists of destination rows per TF row); dst_ptr [N+2], dst_rows [2E+N]
 * (rows contributing to each node, forward); src_ptr [N+2], src_rows [2E+N] (rows contributing to each node's input
 * gradient); only the first N+1 ptr entries are meaningful.  host_counts[5] = {#edge rows P, #AGG rows, #TF rows,
 * #AGG edges, #TF edges}; host_modes [R] (0 EDGE, 1 AGG, 2 TF).  Synchronises the stream.
 * This is the index the reference's DGL path never needs because it materialises a per-edge [E,H,H] weight tensor instead
 * (subgraph_isomorphism/models/rgin.py:109-110). */
size_t dn_row_index_workspace_bytes(int64_t N, int64_t R, int64_t E);
int dn_row_index_build_i32(int64_t N, int64_t R, int64_t E, const int32_t* src, const int32_t* dst,
                           const int32_t* etype, int32_t self_loop, float edge_frac, int32_t* row_in,
                           int32_t* row_out, int32_t* aux_f_ptr, int32_t* aux_f_idx, int32_t* aux_b_ptr,
                           int32_t* aux_b_idx, int32_t* dst_ptr, int32_t* dst_rows, int32_t* src_ptr,
                           int32_t* src_rows, int64_t* host_counts, int32_t* host_rel_ptr, int32_t* host_modes,
                           void* workspace, size_t workspace_bytes, dn_stream_t stream);

/* The same tables as dn_row_index_build_i32, bit for bit, for a batch that is a disjoint union of G graphs: node_ptr [G+1] /
 * edge_ptr [G+1] (device) give every graph a contiguous node range and a contiguous edge range (node_ptr[G] == N,
 * edge_ptr[G] == E) -- the layout dgl.batch / the PyG collate produce (subgraph_isomorphism/dataset.py:1605-1611,
 * graph_classification main.py:245-247).  Every ordering the general builder establishes with device-wide radix sorts is local
 * to a graph in such a batch, so one wavefront rank-sorts one graph in LDS and the only batch-wide step is one exclusive scan
 * of the packed counts: 3 kernels + 1 scan instead of ~60 launches.  Graphs of more than 1024 edges (up to 8191 edges and 8191
 * nodes; round 6) are taken by a second launch of the statistics and fill passes, one 1024-thread workgroup per graph -- a
 * PER-GRAPH fallback: the rest of the batch stays on the one-wavefront kernels.  R <= 64.  *host_status = 1 (outputs undefined) when the
 * batch does not qualify -- a graph of 8192 edges or more (or over 16384 nodes), an endpoint outside its graph's node range, a relation id
 * outside [0, R), ranges that do not tile [0, N) / [0, E): the caller then runs dn_row_index_build_i32.  Other arguments and
 * outputs as dn_row_index_build_i32.  rel_ptr_dev (device, may be NULL; round 5): [R + 2] = the relation offsets of host_rel_ptr
 * followed by the end of the self-loop rows (P + N), for the device-side table builders -- no upload of what the device already
 * has.  host_absorb (host int32 [2], may be NULL; round 5) with tile_ptr_f / _b (device [G + 1]) and fold_info_f / _b (device
 * [G][12], 16-byte aligned): the builder also answers, per direction, whether dn_rows_close_bf16 can ABSORB the fold of this batch
 * -- exactly one collapsed relation in the direction (mode AGG forward / TF backward) owning all the direction's aux lists, with
 * a self loop, and its segments passing dn_fold_graph_tiles_build_i32's test with the relation's own rows as targets -- and
 * leaves that call's tile_ptr / fold_info behind (host_absorb[d] bit 0); bit 1 (round 6): the segments pass the test WITHOUT the
 * 32-node limit (dn_fold_graph_tiles_multi_build_i32 would say yes); host_absorb[2] / [3] = the nodes / edges of the batch's
 * largest graph (what dn_conv_graphs_bf16 asks before it takes a batch); host_absorb: int32 [4]; all ride in the builder's ONE read-back.
 * Synchronises the stream (one read-back). */
size_t dn_row_index_local_workspace_bytes(int64_t G, int64_t N, int64_t R, int64_t E);
int dn_row_index_build_local_i32(int64_t G, int64_t N, int64_t R, int64_t E, const int32_t* node_ptr,
                                 const int32_t* edge_ptr, const int32_t* src, const int32_t* dst, const int32_t* etype,
                                 int32_t self_loop, float edge_frac, int32_t* row_in, int32_t* row_out,
                                 int32_t* aux_f_ptr, int32_t* aux_f_idx, int32_t* aux_b_ptr, int32_t* aux_b_idx,
                                 int32_t* dst_ptr, int32_t* dst_rows, int32_t* src_ptr, int32_t* src_rows,
                                 int64_t* host_counts, int32_t* host_rel_ptr, int32_t* host_modes, int32_t* host_status, int32_t* rel_ptr_dev,
                                 int32_t* tile_ptr_f, int32_t* fold_info_f, int32_t* tile_ptr_b, int32_t* fold_info_b,
                                 int32_t* host_absorb,
                                 void* workspace, size_t workspace_bytes, dn_stream_t stream);

/* One launch per direction of a relational conv on a batch of SMALL graphs at the reference's default width (round 6; H = 64
 * bf16, the CLI default `--hid_dim` of subgraph_isomorphism/config.py:456-461, BASELINE config 3):
 *   out[v, :] = sum_{e: key_out[e] = v} X[key_in[e], :] @ W[etype[e]] + X[v, :] @ W_loop (+ bias)
 * = message UDF + fn.sum + self loop of rgin.py:102-160 / rgcn.py:160-196 with (key_in, key_out) = (src, dst); the input gradient
 * with (dst, src) and w_kn = 0.  W [num_rels][H][H] and W_loop [H][H]: w_kn = 1: stored [k][n] (the parameters `weight` /
 * `loop_weight` as they are: out = x @ W); w_kn = 0: the same memory read as [n][k] (out = x @ W^T: the input-gradient pass on the
 * untransposed parameters).  One workgroup takes one graph straight from the batch's raw arrays (node_ptr / edge_ptr [num_graphs + 1],
 * key_in / key_out / etype [E], global node ids, every edge inside its graph's node range): no row index, no intermediate rows in
 * HBM; every relation is taken edge by edge.  Limits: every graph within dn_conv_graphs_max_nodes() = 64 nodes and
 * dn_conv_graphs_max_edges() = 1024 edges (ask dn_row_index_build_local_i32's host_absorb[2..3]), num_rels <= 16; a graph outside
 * them, or an edge outside its graph / relation range, sets *dev_err (device int32, OR-ed; its rows are left unwritten).
 * aux (may be NULL): [num_graphs][H], aux[j] = bf16 column sum of the INPUT rows of segment j = nodes seg_nodes[seg_ptr[j] ..
 * seg_ptr[j+1]) (a contiguous run inside graph j: the pre-aggregated operand dn_rows_wgrad_bf16 takes for a collapsed relation).
 * fp32 accumulation in a fixed order (bitwise repeatable), every per-edge product rounded to bf16 once, the output row once. */
/* dn_layer_graphs_fwd_bf16 / _bwd_bf16: a whole RGIN layer (rgin.py:102-160 + the MLP of rgin.py:50-57,147-151: Linear - act - Linear
 * - act with act = ReLU (act_slope 0) or leaky ReLU) around the same per-graph conv, ONE launch each way:
 *   fwd: conv_out = conv(X) (+ bias), mid = act(conv_out @ W1^T + b1), out = act(mid @ W2^T + b2); bits1 / bits2 [N][H / 8] = the
 *        sign bits (> 0) of mid / out; aux as in dn_conv_graphs_bf16 (column sums of X).  W / W_loop stored [k][n] (the parameters),
 *        W1 / W2 [out][in] (nn.Linear.weight).
 *   bwd: G = the gradient of out: g_mid = mask1(mask2(G) @ W2), g_conv = g_mid @ W1, g_in = the conv's input gradient of g_conv
 *        (edges dst -> src, W read transposed); aux = column sums of g_conv over the segments (the weight gradient's operand).
 * Same limits, error flag and numerics as dn_conv_graphs_bf16; every row tensor [N][H] bf16. */
int dn_layer_graphs_fwd_bf16(const void* X, int32_t H, const void* W, const void* W_loop, const void* bias, int32_t num_rels,
                             const void* W1, const void* b1, const void* W2, const void* b2, float act_slope, const int32_t* node_ptr,
                             const int32_t* edge_ptr, const int32_t* src, const int32_t* dst, const int32_t* etype, int64_t num_graphs,
                             int64_t N, void* conv_out, void* mid, void* out, void* bits1, void* bits2, const int32_t* seg_ptr,
                             const int32_t* seg_nodes, void* aux, int32_t* dev_err, dn_stream_t stream);
int dn_layer_graphs_bwd_bf16(const void* G, int32_t H, const void* W, const void* W_loop, int32_t num_rels, const void* W1,
                             const void* W2, float act_slope, const void* bits1, const void* bits2, const int32_t* node_ptr,
                             const int32_t* edge_ptr, const int32_t* src, const int32_t* dst, const int32_t* etype, int64_t num_graphs,
                             int64_t N, void* g_mid, void* g_conv, void* g_in, const int32_t* seg_ptr, const int32_t* seg_nodes,
                             void* aux, int32_t* dev_err, dn_stream_t stream);
int32_t dn_conv_graphs_max_nodes(void);
int32_t dn_conv_graphs_max_edges(void);
int dn_conv_graphs_bf16(const void* X, int32_t H, const void* W, int32_t w_kn, const void* W_loop, const void* bias, int32_t num_rels,
                        const int32_t* node_ptr, const int32_t* edge_ptr, const int32_t* key_in, const int32_t* key_out,
                        const int32_t* etype, int64_t num_graphs, int64_t N, void* out, const int32_t* seg_ptr, const int32_t* seg_nodes,
                        void* aux, int32_t* dev_err, dn_stream_t stream);

/* The per-batch index of the H = 256 bf16 conv path as ONE call on one arena (round 5) -- what dgl.batch + update_all pay per step
 * in the reference (subgraph_isomorphism/dataset.py:1605-1611; models/rgin.py:156-160): dn_row_index_build_local_i32 (same
 * arguments and outputs, rel_ptr_dev and the absorbed-fold buffers required) and, queued behind it BEFORE the one read-back,
 *   - the unit streams of both closing launches with the graphs as tiles and the AGG units appended (dn_close_units_build_i32 with
 *     tile_ptr_f / _b, agg_units = 1, xcd_order = close_xcd_order, the folded relation's rows dropped): unit_ptr_* [num_wg + 1], units_* [unit_capacity][4]
 *     (16-byte aligned; unit_capacity >= dn_close_units_capacity(G, E + N, num_wg)), ent_row_* / ent_mask_* [E + N];
 *   - the sweep orders of both transform launches with the folded relation skipped (dn_sweep_tables_build_i32):
 *     sweep_f / sweep_b [8 * sweep_wg_per_group * sweep_tiles_per_wg][4] as CAPACITY (sized by E, a bound of the rows): the
 *     builder lays each table out with the slots its fullest group needs, host_plan[4] / host_plan[5] (forward / backward) slots per
 *     workgroup -- the table is [8 * sweep_wg_per_group * host_plan[4 + d]][4] -- or -1 when not even the plain order fits;
 *     sweep_tiles_per_wg = 0: none;
 * the counts these builders need (edge rows, the folded relation and its row range) are read from device memory.  They serve the
 * batches whose fold can be absorbed -- host_plan[0] (forward) / host_plan[1] (backward) != 0: the build is valid, the direction
 * has its one collapsed relation (host_absorb != 0: bit 0 = every block within 32 nodes, bit 1 = the segments pass the test without
 * that limit) and its segments are the batch's G graphs.  host_plan[d] = 1: the tables above, the graphs as tiles.  host_plan[d] = 2
 * (round 6; a graph over 32 nodes, chunks_per_wg > 0): the SAME launches have built the chunked form instead -- chunk_tile_* /
 * chunk_graph_* [chunks_per_wg * num_wg + 1], tile_ptr_m* [tile_capacity + 1], fold_info_m* [tile_capacity][12] as
 * dn_fold_graph_tiles_multi_build_i32 leaves them (tile_capacity >= dn_fold_graph_tiles_multi_capacity(N, chunks_per_wg * num_wg)),
 * unit streams in order 2 + close_xcd_order (unit_capacity and the workspace then cover max(G, tile_capacity) tiles); which form was
 * needed is decided on the device.  For a direction with 0 its tables are left untouched and the caller builds them with the
 * separate entry points.  chunks_per_wg = 0: no chunked form (the eight pointers may be NULL).  After the read-back the split-K chunk table of the weight gradient over all rows
 * (dn_row_tables_build_i32 with piece_ptr) is queued: host_plan[2] = rows per chunk -- the smallest multiple of 64 (>= 256, <=
 * wgrad_max_chunk_rows) for which the chunks of all relations fit one round of wgrad_workgroups -- host_plan[3] = its entries
 * (rows / chunk + relations + 1 <= chunk_capacity); chunk_table [chunk_capacity][4], chunk_ptr [R + 2]; host_plan: int32 [6].
 * *host_status != 0 as for
 * dn_row_index_build_local_i32 (nothing else is valid).  workspace: 256-byte aligned.  Synchronises the stream once. */
size_t dn_conv_index_workspace_bytes(int64_t G, int64_t N, int64_t R, int64_t E, int32_t num_wg, int64_t tile_capacity);
int dn_conv_index_build_i32(int64_t G, int64_t N, int64_t R, int64_t E, const int32_t* node_ptr, const int32_t* edge_ptr,
                            const int32_t* src, const int32_t* dst, const int32_t* etype, int32_t self_loop, float edge_frac,
                            int32_t* row_in, int32_t* row_out, int32_t* aux_f_ptr, int32_t* aux_f_idx, int32_t* aux_b_ptr,
                            int32_t* aux_b_idx, int32_t* dst_ptr, int32_t* dst_rows, int32_t* src_ptr, int32_t* src_rows,
                            int64_t* host_counts, int32_t* host_rel_ptr, int32_t* host_modes, int32_t* host_status,
                            int32_t* rel_ptr_dev, int32_t* tile_ptr_f, int32_t* fold_info_f, int32_t* tile_ptr_b,
                            int32_t* fold_info_b, int32_t* host_absorb, int32_t num_wg, int32_t close_xcd_order, int64_t unit_capacity, int32_t* unit_ptr_f,
                            int32_t* units_f, int32_t* ent_row_f, uint32_t* ent_mask_f, int32_t* unit_ptr_b, int32_t* units_b,
                            int32_t* ent_row_b, uint32_t* ent_mask_b, int32_t chunks_per_wg, int64_t tile_capacity, int32_t* chunk_tile_f,
                            int32_t* chunk_graph_f, int32_t* tile_ptr_mf, int32_t* fold_info_mf, int32_t* chunk_tile_b,
                            int32_t* chunk_graph_b, int32_t* tile_ptr_mb, int32_t* fold_info_mb, int32_t sweep_wg_per_group,
                            int32_t sweep_tiles_per_wg,
                            int32_t* sweep_f, int32_t* sweep_b, int32_t wgrad_workgroups, int32_t wgrad_max_chunk_rows,
                            int64_t chunk_capacity, int32_t* chunk_table, int32_t* chunk_ptr, int32_t* host_plan, void* workspace,
                            size_t workspace_bytes, dn_stream_t stream);

/* Tile / chunk tables of relation-major rows for dn_rows_transform_* (step = 32 rows) and dn_rows_wgrad_* (step = the
 * split-K chunk size), built on the device from rel_ptr [num_rels + 1] (device): entry i = {rel, beg, end, 0}.  The caller
 * sizes `table` by the upper bound max_entries >= rows / step + num_rels; unused entries become empty pieces (beg == end) of
 * the last relation.  piece_ptr (may be NULL) receives the [num_rels + 1] piece ranges per relation (dn_rows_wgrad_*'s
 * chunk_ptr).  skip_mask: bit r set (r < 64) leaves relation r out of the table (no pieces) -- the relation a caller handles
 * in a launch of its own.  Replaces the per-batch bookkeeping DGL does inside dgl.batch / update_all
 * (subgraph_isomorphism/dataset.py:1605-1611, models/rgin.py:156-160); no device -> host synchronisation. */
int dn_row_tables_build_i32(int32_t num_rels, const int32_t* rel_ptr, int32_t step, int64_t max_entries, int32_t* table,
                            int32_t* piece_ptr, uint64_t skip_mask, dn_stream_t stream);

/* L2-blocked ("sweep") tile order of relation-major rows for the persistent launch of dn_rows_transform_bf16 (H = 256: one
 * workgroup per CU, 256 in all).  The batch is cut into 8 contiguous key ranges (key of row p = the node it belongs to:
 * row_out[p] when < num_nodes, else row_in[p]; non-decreasing inside a relation for the tables of dn_row_index_build_*); group x
 * is walked by the workgroups b = j * 8 + x (blocks b, b + 8, ... share an XCD and its L2).  Inside a group most workgroups serve
 * ONE relation for the whole launch (weights stay in registers) and take every k-th of its tiles, so all of them move through
 * the group's graphs at the same pace and a source row fetched for one relation is still in that XCD's L2 when the other
 * relations ask for it; a few helper workgroups take the left-overs of several relations one after the other (their tiles cost
 * more -- rows out of phase with the group's sweep, a weight reload per relation -- so the quota of the others grows by a few tiles
 * until both kinds finish together; the transform launch does not walk a workgroup's trailing empty slots).  Groups with fewer
 * than 64 tiles per workgroup (an eighth of BASELINE config 5: 32) have no such workgroups: the group's tile line, relation-major,
 * is cut into equal segments (at most two relations per workgroup when a relation has more tiles than a segment) -- a helper's
 * weight reloads, one per relation of the group, were a third of such a launch.
 * table: [8 * workgroups_per_group][tiles_per_workgroup][4] int32 {rel, beg, end, 0}, unused slots empty -- pass it to
 * dn_rows_transform_bf16 with num_tiles = 8 * workgroups_per_group * tiles_per_workgroup and workgroups_per_group = 32 (the
 * launch then gives workgroup b the entries [b * tiles_per_workgroup, (b + 1) * tiles_per_workgroup)).  Every row of every
 * relation not in skip_mask is covered exactly once whatever the keys are (placement is a speed matter only).  When a group
 * needs more than tiles_per_workgroup slots the table holds the plain relation-major order instead (always valid provided
 * 8 * workgroups_per_group * tiles_per_workgroup >= rows / 32 + num_rels); info (may be NULL) receives {0: sweep order, 1: plain order taken, 2: plain
 * order taken AND the table cannot hold all its tiles (8 * workgroups_per_group * tiles_per_workgroup < sum over relations of
 * ceil(rows / 32)): rows would go untransformed, size the table as stated; slots the largest group needs}.  One launch, no host synchronisation.  Replaces nothing in the reference (DGL's update_all has no
 * notion of a traversal order, models/rgin.py:156-160): it is the order in which the replacement reads x. */
int dn_sweep_tables_build_i32(int32_t num_rels, const int32_t* rel_ptr, const int32_t* row_in, const int32_t* row_out,
                              int64_t num_nodes, int32_t workgroups_per_group, int32_t tiles_per_workgroup, uint64_t skip_mask,
                              int32_t* table, int32_t* info, dn_stream_t stream);

/* Fixed-width slot table of per-node row lists for dn_rows_selfsum_bf16 (one-shot index build, ONE launch, no workspace, no
 * host synchronisation; replaces the reference's per-node reduce bookkeeping inside `g.update_all(..., fn.sum(...))`,
 * subgraph_isomorphism/models/rgin.py:137).
 * list_ptr [N+1] / list_rows: CSR of row ids per node (dn_row_index_build_i32's dst_ptr/dst_rows or src_ptr/src_rows).
 * Rows >= num_edge_rows (the self-loop rows) and rows in [drop_beg, drop_end) (a relation the caller adds in a launch of its
 * own; drop_beg == drop_end for none) are dropped; drop_enable (device, may be NULL) switches the drop range off when
 * *drop_enable == 0 -- the verdict dn_fold_tables_build_async_i32 leaves on the device, so the tables of both directions of a
 * batch are queued back to back (the per-batch bookkeeping of subgraph_isomorphism/dataset.py:1605-1611).
 * slots [N, K]: the kept rows in list order, -1 padded; a node with MORE than K kept rows keeps its first K-1 and gets -2 in
 * slot K-1 and 1 in overflow[v] (uint8 [N], may be NULL; 0 for every other node): dn_overflow_rows_add_bf16 adds the rest
 * straight from the node's list after the closing launch (pass it `overflow`, the same list and the drop range). */
int dn_slot_table_build_i32(int64_t N, int32_t num_edge_rows, int32_t K, const int32_t* list_ptr, const int32_t* list_rows,
                            int32_t drop_beg, int32_t drop_end, const int32_t* drop_enable, int32_t* slots, uint8_t* overflow,
                            dn_stream_t stream);

/* Weight gradient of the relation-wise transform Y[p] = A[p] W[rel(p)] on the matrix cores (bf16 in, fp32 acc):
 *   out[r] = sum_{p in relation r} A[idx_a[p], :]^T G[idx_g[p], :]            ([Hi x Ho] per relation)
 * Replaces autograd's backward of the reference's per-edge `th.bmm(x[src], W[etype])`
 * (subgraph_isomorphism/models/rgin.py:109-110,117-118) / PyG RGCNConv's `h @ weight[i]` (rgconv.py:96).
 * Rows are relation-major; the caller splits them into row chunks {rel, beg, end, 0} (int32 x4 each, any chunk
 * inside one relation, chunks of a relation contiguous: chunk_ptr [R+1]).  One workgroup per chunk accumulates the
 * whole Hi x Ho tile; partials (workspace, fp32 [num_chunks, Hi, Ho]) are then added in chunk order: deterministic.
 * idx_a / idx_g may be NULL (row p itself); A2/na1 and G2/ng1 give each operand a second row source exactly as
 * in dn_rows_transform_bf16.  Supported: Hi == Ho in {64, 128, 256}.  out is fp32 or bf16.
 * colsum_of = 1 (A) or 2 (G) also returns out_colsum[r, :] = sum over relation r's rows of that operand (fp32 [R, H]):
 * the bias gradient, taken from the rows while they are staged (0 = off, out_colsum may be NULL).  dn_rows_wgrad_bf16 takes
 * (r + 1) << 8 on top: the column sums of relation r's rows ONLY (the other rows of out_colsum are returned as zeros) -- the
 * reference's bias sees one relation's rows (the self loop's, rgin.py:156-160), and summing the rest costs a sixth of the launch.
 * mask_a (may be NULL; needs A2 == NULL): A rows are first zeroed where mask_a[row, k] <= 0 (ReLU backward folded into the
 * staging); a_out (may be NULL; needs idx_a == NULL) receives those masked rows, so the elementwise pass disappears.
 * mask_a_bits (may be NULL; excludes mask_a, A2 and idx_a: the bit-masked operand is read in row order): the same mask as
 * a bit tensor, uint8 [rows of A, Hi/8], bit i of byte (row, c) = keep element (row, 8c + i) -- the bits1 / bits2 outputs of
 * dn_rows_chain2_bf16.
 * out_colsum_lp (may be NULL; needs colsum_of): a second copy of the column sums in out's element type ([R, H]): the bias
 * gradient in the parameter's dtype without a cast launch. */
size_t dn_rows_wgrad_workspace_bytes(int64_t num_chunks, int32_t Hi, int32_t Ho);
int dn_rows_wgrad_bf16(const void* A, const void* A2, int32_t na1, const int32_t* idx_a, const void* G,
                       const void* G2, int32_t ng1, const int32_t* idx_g, int32_t Hi, int32_t Ho, int64_t R,
                       const int32_t* chunks, int64_t num_chunks, const int32_t* chunk_ptr, void* out,
                       int32_t out_is_f32, int32_t colsum_of, float* out_colsum, const void* mask_a, void* a_out,
                       const void* mask_a_bits, void* out_colsum_lp, float act_slope, void* workspace, size_t workspace_bytes,
                       dn_stream_t stream);

/* Several weight gradients in ONE launch + ONE reduce (round 6): the jobs' relations are numbered through -- job k owns relations
 * [first_rel_k, first_rel_{k+1}) of R -- and their rows lie end to end in one virtual row space (job k's row p is virtual row row0_k
 * + p), so ONE chunk table (dn_row_tables_build_i32 over the virtual relation offsets) and one chunk_ptr cover them; operands,
 * indices, colsum_of, mask_a_bits and act_slope per job as in dn_rows_wgrad_bf16 (no mask_a / a_out here).  out [R][H][H],
 * out_colsum [R][H] fp32 (zeros for a job with colsum_of = 0), out_colsum_lp [R][H] in out's type or NULL.  H = 64 / 128: the
 * widths at which a layer's three weight-gradient launches and their reduces are launch latency (BASELINE config 3: the whole
 * backward of an RGIN layer then needs one weight-gradient launch, subgraph_isomorphism/models/rgin.py:50-67,102-160).
 * H = 256 (rows_wgrad_ls_multi_kernel): a job is gathered on both sides (idx_a and idx_g; second sources allowed), or in row order
 * on both, with or without mask_a_bits; colsum_of may carry (relation + 1) << 8 -- a relation of THAT job, counted from its
 * first_rel -- as in dn_rows_wgrad_bf16; any chunk table over the virtual rows serves (the host side gives the row-order jobs
 * chunks of half the rows: ops.wide_layer_chunks).  One launch for a layer's three gradients pays on small batches only -- an
 * eighth of BASELINE config 5, one rank's share at 8 GPUs: 175 -> 150 us -- where the fixed costs of a launch count; every one of
 * them is HBM-bound. */
typedef struct dn_wgrad_job {
    const void *A, *A2;
    const int32_t* idx_a;
    const void *G, *G2;
    const int32_t* idx_g;
    const void* mask_a_bits;
    int32_t na1, ng1, colsum_of, first_rel, row0;
    float act_slope;
} dn_wgrad_job;
int dn_rows_wgrad_multi_bf16(const dn_wgrad_job* jobs, int32_t num_jobs, int32_t H, int64_t R, const int32_t* chunks, int64_t num_chunks,
                             const int32_t* chunk_ptr, void* out, int32_t out_is_f32, float* out_colsum, void* out_colsum_lp,
                             void* workspace, size_t workspace_bytes, dn_stream_t stream);
/* The same for fp32 rows on the 3-term bf16 split (dn_rows_wgrad_f32 with precision 0): A / A2 / G / G2 of a job are float tensors;
 * a job's mask_a_bits, when not NULL, points to a FLOAT tensor [rows of A, H] -- the saved activation, dn_rows_wgrad_f32's mask_a:
 * A rows are kept where it is > 0 and multiplied by act_slope elsewhere (needs A2 == NULL and idx_a == NULL).  out [R][H][H] and
 * out_colsum [R][H] fp32.  H = 64 / 128.  With this the
 * backward of an fp32 RGIN layer at the reference's default width (config.py:456-461) takes one weight-gradient launch and one
 * reduce instead of three of each (rgin.py:102-160's three parameter groups: weight / loop_weight + bias, mlp[0], mlp[2]). */
int dn_rows_wgrad_multi_f32(const dn_wgrad_job* jobs, int32_t num_jobs, int32_t H, int64_t R, const int32_t* chunks, int64_t num_chunks,
                            const int32_t* chunk_ptr, float* out, float* out_colsum, void* workspace, size_t workspace_bytes,
                            dn_stream_t stream);

/* Two dense layers in ONE pass over fp32 rows (3-term bf16 split; H = 64 / 128):
 *   X0 = mask0 ? keep_or_scale(X, mask0) : X;   Y1 = keep_or_scale?(epi1(X0 @ W1n^T), mask1);   Y2 = epi2(Y1 @ W2n^T)
 * epi = (+ bias) then the optional activation (relu flag, act_slope as in dn_rows_transform_f32); mask0 / mask1 (may be NULL) are
 * float tensors [N, H]: elements are kept where the mask is > 0 and multiplied by act_slope elsewhere.  w_kn bit i: weight i is given
 * [in][out] (the parameter of the OTHER direction as stored) instead of [out][in].  Forward of the reference MLP
 * (subgraph_isomorphism/models/rgin.py:50-57: Linear, act, Linear + the layer's activation :147-151) and -- with mask0 = the saved
 * output, W1n = Linear 2's weight, mask1 = the saved hidden rows, W2n = Linear 1's weight, w_kn = 3 -- autograd's input-gradient
 * chain through both, each as one launch (the fp32 twin of dn_rows_chain2_bf16; its masks are the saved activations, not bits).
 * residual / Y2_plus (both or neither; float [N, H]): Y2_plus = Y2 + residual is written next to Y2 -- the representation net's
 * residual connection (rgin.py:243-245: `outputs[-1] + o`) without a launch of its own; Y2 stays the activation the backward masks by. */
int dn_rows_chain2_f32(const float* X, int32_t H, const float* W1n, const float* b1, int32_t relu1, const float* mask0,
                       const float* mask1, const float* W2n, const float* b2, int32_t relu2, int64_t N, float* Y1, float* Y2,
                       int32_t w_kn, float act_slope, const float* residual, float* Y2_plus, dn_stream_t stream);

/* Relation-wise transform of gathered rows on the matrix cores (bf16 in, fp32 acc, bf16 out):
 *   Y[p, n] = epi( sum_k Xcat[idx[p], k] * Wn[rel(p)][n][k] ),  epi = (+ bias[rel(p)][n]) then optional ReLU
 * Xcat is the virtual concatenation of X (rows [0, n1)) and X2 (rows n1, n1+1, ...): an index i >= n1 reads
 * X2[i - n1]; pass X2 = NULL with n1 = INT32_MAX for a single source.  idx == NULL means row p itself.
 * Wn[r] is [Ho][Hi] with k contiguous (i.e. W_r transposed for Y = X W_r).  Rows are relation-major and the caller
 * provides the tile table {rel, beg, end, 0} (int32 x4; a tile has at most 32 rows and lies inside one relation).
 * Replaces the reference's per-edge `weight.index_select(0, etype)` + `th.bmm` message function
 * (subgraph_isomorphism/models/rgin.py:102-120, rgcn.py:100-122), its self-loop matmul (rgin.py:141) and, in the
 * backward direction (X = grad rows, Wn = W_r), autograd's transposed product.  Ho == Hi in {64, 128, 256}.
 * mask_pos (may be NULL): after epi, elements where mask_pos[p, n] <= 0 are zeroed.
 * act_slope: the activation of `relu` / `mask_pos` generalised to leaky ReLU -- relu: max(v, 0) + act_slope * min(v, 0); mask_pos:
 * elements whose saved activation is <= 0 are multiplied by act_slope instead of zeroed.  0 = ReLU; 1 / 5.5 = the reference's
 * default `leaky_relu` (subgraph_isomorphism/utils/act.py:466, constants.py:10).  The same argument, with the same meaning for
 * their ReLU flags / masks / mask bits, is taken by dn_rows_wgrad_*, dn_rows_chain2_bf16 and dn_relu_bwd_*.
 * w_kn != 0 (Hi == 256: with idx != NULL or X2 == NULL only, DN_ERR_UNSUPPORTED otherwise; Hi == 64 / 128: round 5, transposed through
 * LDS at every change of relation): Wn[r] is stored [k][n] -- the layout
 * of the reference's `weight` parameter (rgin.py:61-67), so the forward pass needs no transposed copy of the weights. */
int dn_rows_transform_bf16(const void* X, const void* X2, int32_t n1, const int32_t* idx, int32_t Hi, int32_t Ho,
                           const void* Wn, const void* bias, int32_t relu, const void* mask_pos,
                           const int32_t* tiles, int64_t num_tiles, void* Y, int32_t w_kn, float act_slope, dn_stream_t stream);

/* Closing launch of the row-factorised message pass (bf16 in, fp32 acc, bf16 out):
 *   out[v, :] = X[v, :] @ Wn^T (+ bias)  +  sum_{k < num_slots} Scat[slots[v * num_slots + k], :]
 * i.e. the self-loop transform `th.matmul(node_feat, self.loop_weight)` + bias (subgraph_isomorphism/models/rgin.py:
 * 140-145, rgcn.py:168-182) fused with the per-node sum of the transformed rows (the reference's `fn.sum(msg, out)`
 * reduce, rgin.py:137 / rgcn.py:166) -- and, in the backward direction, the same for the input gradient.
 * Wn is [H][H] with k contiguous (w_kn = 0) or [k][n] as the parameter `loop_weight` stores it (w_kn = 1, round 5: no transposed
 * copy in front of the launch).  slots is an [N, num_slots] int32 table of row ids into Scat = S (rows [0, n1))
 * followed by S2 (row n1, n1+1, ...; S2 = NULL with n1 = INT32_MAX for none); negative ids are empty slots.  A node with
 * more than num_slots rows carries -2 in its last slot (dn_slot_table_build_i32) and is finished by dn_overflow_rows_add_bf16
 * right after this launch -- or, with list_ptr / list_rows (the lists the slot table was built from, may be NULL) and the builder's
 * filter (num_edge_rows, drop_beg, drop_end), INSIDE this launch (round 5): the node's thread walks its list and adds the rows behind
 * the first num_slots - 1 kept ones in fp32 before the one rounding.  For small batches, where a second launch costs more than the
 * walk; large ones keep dn_overflow_rows_add_bf16 (the walk stalled every other tile: + 130 us at config 5).  num_slots must be 6.
 * H in {64, 128, 256}.
 * Folded pre-aggregation (fold_info != NULL): the launch also sums the X rows it reads per SEGMENT -- the input row of a
 * collapsed relation (all nodes of a graph -> its dummy node: one row per graph whose input is the sum of the graph's rows,
 * the reference's per-edge messages of the dummy edge type, rgin.py:102-120 on dataset.py:1563-1603's dummy edges) -- so the
 * separate pass over X that dn_gather_segsum_bf16 would make disappears.  Segments must be CONTIGUOUS ascending row ranges;
 * the caller numbers the (segment, 32-row tile) pairs that share a row ("partial rows"), segment-major, so that a tile's pairs
 * are consecutive.  fold_info (dn_fold_tables_build_i32) holds one 12-word record per tile: 32 bytes = each row's partial row
 * minus the tile's first one (255: the row belongs to no segment), then {first partial row, number of partial rows, 0, 0}.
 * The launch writes the fp32 column sums of every pair to seg_part[pair * H ...] (one extra MFMA per wave with a 0/1 indicator
 * operand); dn_fold_tail_bf16 adds a segment's partial rows in tile order: deterministic. */
int dn_rows_selfsum_bf16(const void* X, int32_t H, const void* Wn, const void* bias, const void* S, const void* S2,
                         int32_t n1, const int32_t* slots, int32_t num_slots, int64_t N, void* out,
                         const int32_t* fold_info, float* seg_part, int32_t w_kn, const int32_t* list_ptr,
                         const int32_t* list_rows, int32_t num_edge_rows, int32_t drop_beg, int32_t drop_end, dn_stream_t stream);

/* Nodes with more rows than slots: out[v, :] += sum of the rows of v's list beyond the first num_slots - 1 kept ones, for every
 * node with overflow[v] != 0 (dn_slot_table_build_i32's byte per node).  The walk applies the table builder's filter (rows >= num_edge_rows
 * and rows in [drop_beg, drop_end) are not edge rows of this launch) in list order; fp32 sum added to the bf16 row, one rounding.
 * Runs after dn_rows_selfsum_bf16 on the same `out` (the remainder of the reference's fn.sum reduce for high in-degree nodes,
 * subgraph_isomorphism/models/rgin.py:137).  In the closing launch itself the walk -- dependent loads of a few nodes -- stalled
 * every other tile (measured: + 130 us per config-5 launch); as a launch of its own it is a screen of N ints and a few thousand
 * short lists.  H in {64, 128, 256}. */
int dn_overflow_rows_add_bf16(const void* S, int32_t H, const uint8_t* overflow, int32_t num_slots, int64_t N, const int32_t* list_ptr,
                              const int32_t* list_rows, int32_t num_edge_rows, int32_t drop_beg, int32_t drop_end, void* out,
                              dn_stream_t stream);

/* The closing launch at H = 256 as a stream of 32-row units (csrc/dn_close.hip; same result as dn_rows_selfsum_bf16 +
 * dn_overflow_rows_add_bf16, with no slot limit and no second launch):
 *   out[v, :] = X[v, :] @ W_loop (+ bias)  +  sum over the kept rows p of v's list of S[p, :]
 * (the reference's `fn.sum(msg, out)` reduce + `th.matmul(node_feat, self.loop_weight)` + bias,
 * subgraph_isomorphism/models/rgin.py:137-146 / rgcn.py:166-182; backward direction: the same for the input gradient).
 *
 * dn_close_units_build_i32 (one-shot index build per batch and direction, three launches, no host synchronisation; the
 * bookkeeping dgl.batch + update_all do per step, subgraph_isomorphism/dataset.py:1605-1611): nodes are cut into num_tiles
 * tiles of at most 32 -- tile t = nodes [tile_ptr[t], tile_ptr[t+1]) (device, [num_tiles + 1]), or the 32-node windows when
 * tile_ptr == NULL (num_tiles = ceil(N / 32)).  For every tile the DISTINCT kept rows of its nodes' lists (list_ptr [N+1] /
 * list_rows as in dn_slot_table_build_i32, same num_edge_rows / drop range / drop_enable filter), sorted by row, are written to
 * ent_row with a 32-bit membership mask in ent_mask (bit i: node tile_ptr[t] + i adds the row; a row that ONE node lists twice
 * stays a second entry), from the offset list_ptr[tile_ptr[t]] onwards -- so ent_row / ent_mask need num_list_entries elements.
 * units [unit_capacity][4] int32 records {flags, beg, end, aux} in WORKGROUP-MAJOR order (its records are
 * units[unit_ptr[w] .. unit_ptr[w+1])).  xcd_order = 0: workgroup w of num_wg takes tiles w, w + num_wg, ... (one front walking the
 * batch upwards); xcd_order = 1 (round 5; num_wg a multiple of 8): workgroup w = 8 j + x -- dispatched to XCD x -- takes the tiles
 * of the x-th EIGHTH of the batch, [floor(x T / 8), floor((x + 1) T / 8)), DOWNWARDS from its end: end - 1 - (j + (num_wg / 8) n).
 * The transform launch in front of the closing launch walks the eighth of XCD x upwards (dn_sweep_tables_build_i32), so the closing
 * launch begins on the rows the transform wrote and gathered last (that XCD's L2, the Infinity Cache): -2 % on the pair at config 5.
 * Per tile one X record {rows << 8 | 2 if no entries,
 * first node, end node, tile} followed by one record per 32 entries {rows << 8 | 1 | 2 on the last, first entry, end entry, first
 * node}; with agg_units != 0 a workgroup's tiles are followed by 8 records {8, 0, 1, 0} (a gap) and one record {4 | 2, n, n', 0}
 * ({4 | 2 | 16, n, n', num_tiles} with xcd_order = 1) per 32 of its tiles (the n-th .. n'-th of them): the AGG units of the absorbed
 * fold below.
 * unit_capacity >= dn_close_units_capacity(num_tiles, num_list_entries, num_wg) = 3 num_tiles + num_list_entries / 32 + 1 + 9 num_wg.
 *
 * dn_fold_graph_tiles_build_i32 (one launch): the tiles of a batch of GRAPHS for the absorbed fold.  Segment j = the nodes
 * seg_nodes[seg_ptr[j] .. seg_ptr[j+1]) as in dn_fold_tables_build_i32; block j = [first node of segment j (0 for j = 0), first
 * node of segment j + 1 (N for the last)).  *dev_ok (device) stays non-zero when every segment is a non-empty contiguous
 * ascending run, the segments ascend, every block has at most 32 nodes and (add_idx != NULL, device [num_segments]: the output
 * row the segment's product is added to, i.e. the agg_idx of dn_rows_close_bf16) add_idx[j] lies inside block j -- the AGG unit
 * of tile j is a read-modify-write of out[add_idx[j]] by the workgroup that stored tile j, so a target in another block (the
 * dummy node in front of its graph, all dummy nodes at the end of the batch) keeps the partial rows + dn_fold_tail_bf16.  Then
 * tile_ptr [num_segments + 1] = the block starts (tile j = block j) and fold_info [num_segments][12] = per tile {32 bytes: 0 for a node of the segment, 255 otherwise; j; 1; 2; 0}.
 *
 * dn_fold_graph_tiles_multi_build_i32 (round 6; three launches, no read-back): the same for graphs of ANY size -- TU graphs are
 * not all within 32 nodes (graph_classification/data_processing/tu_data_processing.py:179-218 keeps whatever sizes the dataset
 * has; PROTEINS reaches 620).  The batch is cut into num_chunks CHUNKS at graph boundaries -- graph j (block start b0_j) belongs to
 * chunk floor(b0_j num_chunks / N) -- and every chunk into consecutive 32-node tiles that run ACROSS the graphs inside it (only a
 * chunk's last tile is partial: T <= N / 32 + num_chunks).  chunk_tile [num_chunks + 1] = a chunk's first tile (chunk_tile[num_chunks]
 * = T, known on the device only), chunk_graph [num_chunks + 1] = its first graph, tile_ptr [T + 1], fold_info [T][12] = per tile
 * {32 bytes: the local number of the node's segment in order of appearance, 255 outside every segment; the first such segment (=
 * graph = aux row); how many; bit 0 = the first one continues the previous tile's column sum | bit 1 = the last one ends in this
 * tile; 0}.  The tables must hold tile_capacity >= dn_fold_graph_tiles_multi_capacity(N, num_chunks) tiles; nothing is written for
 * an invalid batch (*dev_ok = 0).  Same validity test as above without the 32-node limit.  num_chunks < 16384.
 * dn_close_units_build_i32 with xcd_order = 2 / 3 takes these tables (tile_ptr, chunk_tile, chunk_graph, chunks_per_wg = K with
 * num_chunks = K num_wg; num_tiles = the capacity the tables were sized by) and deals the CHUNKS to the workgroups as xcd_order 0 / 1
 * deal tiles (K each), so that a graph's tiles stay in ONE stream: a segment's column sum continues from tile to tile in the
 * workgroup (fp32, one rounding) and the AGG unit's read-modify-write of out[add_idx[j]] stays inside the workgroup that stored
 * that row -- while the launch still sweeps the batch as a front of short runs.  A workgroup's stream = the tiles of its chunks,
 * the gap, and per chunk one AGG record {4 | 2 | 32, first graph, end graph, 0} per 32 graphs (the aux rows themselves).
 *
 * dn_rows_close_bf16: one persistent workgroup per entry of unit_ptr (launch num_wg = the builder's).  W: the self-loop weight,
 * w_kn = 0: [H][H] with k contiguous (W_loop transposed, as dn_rows_selfsum_bf16 takes it), w_kn = 1: [k][n] as the
 * parameter stores it (`loop_weight`, rgin.py:61) -- no transposed copy needed.  bias may be NULL.  fold_info + seg_part: the
 * folded pre-aggregation exactly as in dn_rows_selfsum_bf16 (fp32 partial rows, finished by dn_fold_tail_bf16).
 * fold_info + W_agg + aux + agg_idx (seg_part NULL; tables built with tile_ptr / agg_units from dn_fold_graph_tiles_build_i32):
 * the ABSORBED fold -- every segment lies inside one tile, so its column sum leaves as the bf16 row aux[segment] (kept by the
 * caller: the collapsed relation's operand of dn_rows_wgrad_bf16), and the workgroup's AGG units multiply its segments' aux rows
 * by W_agg (same layout flag as W) and add each product to out[agg_idx[segment]] -- what dn_fold_tail_bf16 does, inside this
 * launch.  A non-finite element of S turns its column of the whole tile into NaN (0 x Inf inside the selection product).
 * H must be 256. */
int64_t dn_close_units_capacity(int64_t num_tiles, int64_t num_list_entries, int32_t num_wg);
size_t dn_close_units_workspace_bytes(int64_t num_tiles, int32_t num_wg);
int dn_close_units_build_i32(int64_t N, int32_t num_edge_rows, int32_t num_wg, const int32_t* tile_ptr, int64_t num_tiles,
                             int32_t agg_units, int32_t xcd_order, const int32_t* list_ptr, const int32_t* list_rows, int64_t num_list_entries,
                             int32_t drop_beg, int32_t drop_end, const int32_t* drop_enable, int32_t* unit_ptr, int32_t* units,
                             int64_t unit_capacity, int32_t* ent_row, uint32_t* ent_mask, const int32_t* chunk_tile,
                             const int32_t* chunk_graph, int32_t chunks_per_wg, void* workspace, size_t workspace_bytes,
                             dn_stream_t stream);
int64_t dn_fold_graph_tiles_multi_capacity(int64_t N, int32_t num_chunks);
int dn_fold_graph_tiles_multi_build_i32(int64_t N, int64_t num_segments, const int32_t* seg_ptr, const int32_t* seg_nodes,
                                        const int32_t* add_idx, int32_t num_chunks, int32_t* chunk_tile, int32_t* chunk_graph,
                                        int32_t* tile_ptr, int32_t* fold_info, int64_t tile_capacity, int32_t* dev_ok,
                                        dn_stream_t stream);
int dn_fold_graph_tiles_build_i32(int64_t N, int64_t num_segments, const int32_t* seg_ptr, const int32_t* seg_nodes,
                                  const int32_t* add_idx, int32_t* tile_ptr, int32_t* fold_info, int32_t* dev_ok,
                                  dn_stream_t stream);
int dn_rows_close_bf16(const void* X, int32_t H, const void* W, int32_t w_kn, const void* bias, const void* S,
                       const int32_t* unit_ptr, const int32_t* units, int32_t num_wg, const int32_t* ent_row,
                       const uint32_t* ent_mask, int64_t N, void* out, const int32_t* fold_info, float* seg_part,
                       const void* W_agg, void* aux, const int32_t* agg_idx, dn_stream_t stream);

/* Tables of a folded pre-aggregation (one-shot index build, like dn_slot_table_build_i32): segment j = the rows
 * seg_nodes[seg_ptr[j] .. seg_ptr[j+1]) (dn_row_index_build_i32's aux_f_ptr/aux_f_idx or aux_b_ptr/aux_b_idx: the nodes of a graph
 * that feed / are fed by its dummy node, subgraph_isomorphism/dataset.py:1563-1603).  host_ok = 1 when every segment is a
 * non-empty contiguous ascending run of rows and the segments ascend -- otherwise the outputs are undefined and the caller keeps
 * the separate dn_gather_segsum pass.  Outputs: fold_info [ceil(N/32)][12] int32 as dn_rows_selfsum_bf16 reads it, part_ptr
 * [num_segments + 1] = the partial-row range of each segment (dn_fold_tail_bf16).  The number of partial rows is at most
 * 2 * num_segments + N / 32 + 1.  The call synchronises the stream. */
size_t dn_fold_tables_workspace_bytes(int64_t num_segments);
int dn_fold_tables_build_i32(int64_t N, int64_t num_segments, const int32_t* seg_ptr, const int32_t* seg_nodes,
                             int32_t* fold_info, int32_t* part_ptr, int32_t* host_ok, void* workspace, size_t workspace_bytes,
                             dn_stream_t stream);
/* The same build without the read-back: *dev_ok (device) ends up non-zero when the tables are valid, 0 otherwise. */
int dn_fold_tables_build_async_i32(int64_t N, int64_t num_segments, const int32_t* seg_ptr, const int32_t* seg_nodes,
                                   int32_t* fold_info, int32_t* part_ptr, int32_t* dev_ok, void* workspace,
                                   size_t workspace_bytes, dn_stream_t stream);

/* Tail of a folded pre-aggregation, one launch:  aux[j, :] = bf16( sum_{k in [part_ptr[j], part_ptr[j+1])} part[k, :] ) in k
 * order (kept by the caller: the collapsed relation's operand of dn_rows_wgrad_bf16), then the relation's transform of those
 * rows added to their one output row each:  out[idx[j], :] += aux[j, :] @ Wn^T   (Wn [H][H], k contiguous; idx distinct; the
 * fp32 product is added to the bf16 row and rounded once).  H in {64, 128, 256}.  w_kn != 0: Wn is stored [k][n]. */
int dn_fold_tail_bf16(const float* part, const int32_t* part_ptr, int64_t num_segments, int32_t H, const void* Wn,
                      const int32_t* idx, void* aux, void* out, int32_t w_kn, dn_stream_t stream);

/* Block-diagonal relation weights (regularizer "bdd", the reference CLI's default: subgraph_isomorphism/config.py:145-158):
 * blocks [R, B, si, so] (the layer's `weight` parameter viewed per relation, rgin.py:68-78) -> dense [R, B*si, B*so] with the B
 * blocks of a relation on its diagonal and zeros elsewhere, so that `bdd` runs on the same relation-transform kernels as `basis`
 * (the reference multiplies per block, rgin.py:114-120; the zeros add nothing).  dn_bdd_extract is the gradient: the diagonal
 * blocks of a dense [R, B*si, B*so] gradient.  elem_bytes = 2 (bf16) or 4 (f32).  One launch each. */
int dn_bdd_compose(const void* blocks, int64_t R, int32_t B, int32_t si, int32_t so, int32_t elem_bytes, void* dense,
                   dn_stream_t stream);
int dn_bdd_extract(const void* dense, int64_t R, int32_t B, int32_t si, int32_t so, int32_t elem_bytes, void* blocks,
                   dn_stream_t stream);

/* Two dense layers in one pass over the rows (bf16 in, fp32 acc, bf16 out):
 *   Y1 = epi1(m0(X) @ W1n^T),  Y2 = epi2(Y1 @ W2n^T)
 *   m0   = zero the elements of X whose bit in mask0_bits is clear (mask0_bits may be NULL)
 *   epi1 = (+ b1), ReLU if relu1, then zero where the bit in mask1_bits is clear (mask1_bits may be NULL)
 *   epi2 = (+ b2), ReLU if relu2
 *   bits1 / bits2 (may be NULL): bit tensors of Y1 / Y2, bit set where the element is > 0
 * Bit tensors are uint8 [N, H/8]: bit i of byte (p, c) belongs to element (p, 8c + i).
 * Forward of the reference's two-layer MLP after the aggregate (subgraph_isomorphism/models/rgin.py:50-57 followed by the
 * layer activation, :147-151: Linear-ReLU-Linear-ReLU), emitting the ReLU masks as bits, and -- with mask0 = bits of the
 * output activation, mask1 = bits of the hidden one -- the input-gradient chain of its backward.  W1n / W2n are [H][H]
 * with k contiguous (nn.Linear.weight for the forward); b1 / b2 may be NULL.  w_kn: bit 0 / bit 1 = W1n / W2n is stored
 * [k][n] instead -- the backward chain takes the Linear weights as they are (its first product is g @ W2, k = W2's rows), so no
 * transposed copies are made.  Y1 is written but never re-read.  H in {64, 128, 256}. */
int dn_rows_chain2_bf16(const void* X, int32_t H, const void* W1n, const void* b1, int32_t relu1, const void* mask0_bits,
                        const void* mask1_bits, const void* W2n, const void* b2, int32_t relu2, int64_t N, void* Y1, void* Y2,
                        void* bits1, void* bits2, int32_t w_kn, float act_slope, dn_stream_t stream);

/* One Linear's whole backward in ONE pass over its rows (bf16, H = 256): weight gradient, bias gradient and input gradient.
 *   Gm     = mask_in_bits ? keep_or_scale(G, mask_in_bits) : G
 *   out_w  = sum_p Gm[p, :]^T A[p, :]   ([H, H], fp32 or bf16: out_is_f32)      out_colsum = colsum(Gm)  (fp32 [H])
 *   g_next = mask_out_bits ? keep_or_scale(Gm @ W_kn, mask_out_bits) : Gm @ W_kn          (bf16 [N, H])
 * G: the gradient of the Linear's (activated) output, A: the Linear's input rows, W_kn: nn.Linear.weight as the parameter
 * stores it ([out = k][in = n]).  mask_in_bits / mask_out_bits (both or neither): the bit tensors of dn_rows_chain2_bf16 (uint8
 * [N, H/8]) -- the activation behind this Linear and the one in front of it; act_slope as everywhere (0 = ReLU).
 * chunks / chunk_ptr: a split-K row-chunk table of ONE relation over rows [0, N) as dn_rows_wgrad_bf16 takes it; workspace:
 * dn_rows_wgrad_workspace_bytes(num_chunks, H, H).  out_colsum_lp (may be NULL): the column sums again in out_w's element type.
 * The reference MLP's backward (subgraph_isomorphism/models/rgin.py:50-57 + the layer activation) is this call twice -- layer 2
 * with both masks, layer 1 on its g_next without -- and every result is bit-identical to dn_rows_wgrad_bf16 (mask_a_bits) +
 * dn_rows_chain2_bf16 (w_kn = 3, both masks) + dn_rows_wgrad_bf16 on the same chunk table: same tiles, same order, same rounding. */
int dn_mlp_bwd_fused_bf16(const void* G, const void* A, const void* W_kn, const void* mask_in_bits, const void* mask_out_bits,
                          int64_t N, int32_t H, const int32_t* chunks, int64_t num_chunks, const int32_t* chunk_ptr, void* out_w,
                          int32_t out_is_f32, float* out_colsum, void* out_colsum_lp, void* g_next, float act_slope,
                          void* workspace, size_t workspace_bytes, dn_stream_t stream);

/* ReLU backward of the post-aggregate MLP (act_func "relu": utils/act.py:463; applied at rgin.py:56,147-151):
 * out = (y > 0) ? g : 0 on bf16 tensors of `numel` elements (multiple of 8).  The same mask is available as the
 * `mask_pos` epilogue of dn_rows_transform_bf16 ([rows, Ho] saved activations), so a Linear's input gradient comes
 * out already masked for the ReLU in front of it. */
int dn_relu_bwd_bf16(const void* g, const void* y, void* out, int64_t numel, float act_slope, dn_stream_t stream);

/* fp32 twins of the three entry points above: same semantics and argument meaning, float tensors, float partials /
 * outputs -- the path that keeps the reference's fp32 numerics (outputs within 1e-4) while still avoiding its [E,H,H]
 * per-edge weight gather.  `precision` selects the arithmetic:
 *   0  3-term bf16 split on the fast matrix path: operands cut into hi = bf16(x), lo = bf16(x - hi) as they are staged,
 *      products evaluated as hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_bf16 with f32 accumulation (O(2^-16) relative
 *      per product, 1e-5-level agreement with the reference; 3/16 of the exact path's matrix time);
 *   1  exact f32 (v_mfma_f32_16x16x4_f32, bit for bit an fmaf chain): the checker.
 * dn_rows_transform_f32 reads the layer's parameters where they lie (rgin.py:61-67: weight [R, in, out], loop_weight
 * [in, out], h_bias [out]), so a step needs no concatenated / transposed weight copy and no padded bias matrix:
 *   W_loop / loop_rel  tiles of relation `loop_rel` use the matrix W_loop instead of Wn[loop_rel] (loop_rel < 0 or W_loop
 *                      NULL: every relation indexes Wn);
 *   bias_rel           >= 0: `bias` is ONE row [Ho] that only tiles of that relation add (the self-loop rows, rgin.py:146);
 *                      < 0: `bias` is [R, Ho], one row per relation (as dn_rows_transform_bf16);
 *   w_kn               1: every matrix is [k = in][n = out] (parameter layout), 0: [n][k]. */
int dn_rows_transform_f32(const float* X, const float* X2, int32_t n1, const int32_t* idx, int32_t Hi, int32_t Ho,
                          const float* Wn, const float* bias, int32_t relu, const float* mask_pos,
                          const int32_t* tiles, int64_t num_tiles, float* Y, int32_t precision, float act_slope,
                          const float* W_loop, int32_t loop_rel, int32_t bias_rel, int32_t w_kn, dn_stream_t stream);
int dn_rows_wgrad_f32(const float* A, const float* A2, int32_t na1, const int32_t* idx_a, const float* G,
                      const float* G2, int32_t ng1, const int32_t* idx_g, int32_t Hi, int32_t Ho, int64_t R,
                      const int32_t* chunks, int64_t num_chunks, const int32_t* chunk_ptr, float* out,
                      int32_t colsum_of, float* out_colsum, const float* mask_a, float* a_out, int32_t precision,
                      float act_slope, void* workspace, size_t workspace_bytes, dn_stream_t stream);
int dn_relu_bwd_f32(const float* g, const float* y, float* out, int64_t numel, float act_slope, dn_stream_t stream);

/* Relation-grouped dense products for ANY widths (what PyG's RGCNConv computes with a Python loop over relations,
 * `for i in range(num_relations): out += h @ weight[i]`; call sites graph_classification/graph_neural_networks/models/
 * rgconv.py:17-18,96): rows p relation-major, pieces from dn_row_tables_build_i32 (step 64 for the tiles).
 *   dn_rows_gemm_*       Y[p,:] = A[p,:] @ Wr (+ bias[rel]),  Wr[k][n] = transposed ? W[rel][n][k] : W[rel][k][n]   (A [P,K], Y [P,N];
 *                        bias [R,N] in the storage type, may be NULL)
 *   dn_rows_wgrad_any_*  out[r] = sum_{p in relation r} A[p,:]^T G[p,:]   ([K,N] per relation; split-K chunks, partials added
 *                        in chunk order; workspace from dn_rows_wgrad_any_workspace_bytes); colsum_out (fp32 [R,K], may be NULL)
 *                        = sum_{p in relation r} A[p,:], the bias gradient of a Linear layer whose output gradient is A
 * fp32 accumulation, plain FMA tiles (the widths here are the ones the matrix-core kernels do not cover). */
int dn_rows_gemm_f32(const float* A, const float* W, const float* bias, int32_t K, int32_t N, int32_t transposed, const int32_t* tiles,
                     int64_t num_tiles, float* Y, dn_stream_t stream);
int dn_rows_gemm_bf16(const void* A, const void* W, const void* bias, int32_t K, int32_t N, int32_t transposed, const int32_t* tiles,
                      int64_t num_tiles, void* Y, dn_stream_t stream);
size_t dn_rows_wgrad_any_workspace_bytes(int64_t num_chunks, int32_t K, int32_t N);
int dn_rows_wgrad_any_f32(const float* A, const float* G, int32_t K, int32_t N, int64_t R, const int32_t* chunks, int64_t num_chunks,
                          const int32_t* chunk_ptr, float* out, float* colsum_out, void* workspace, size_t workspace_bytes,
                          dn_stream_t stream);
int dn_rows_wgrad_any_bf16(const void* A, const void* G, int32_t K, int32_t N, int64_t R, const int32_t* chunks, int64_t num_chunks,
                           const int32_t* chunk_ptr, void* out, float* colsum_out, void* workspace, size_t workspace_bytes,
                           dn_stream_t stream);

/* BatchNorm over the rows of [N, C] node features, training mode (batch statistics), optionally with the ReLU that follows it
 * -- the `BatchNorm1d, ReLU` pairs inside the MLPs of the GC models (graph_classification/graph_neural_networks/models/
 * gconv.py:187-194, rgconv.py:85-93).
 *   forward:   mean / var (biased) / rstd [C] over the rows;  Y = act((X - mean) * rstd * weight + bias), act = ReLU when relu != 0
 *              (weight / bias may be NULL)
 *   backward:  DY' = DY where Y > 0 (relu; Y is recomputed from X), else DY;  sum_dy [C] (= dbias), sum_dy_xhat [C] (= dweight)
 *              of DY';  DX = weight * rstd * (DY' - sum_dy / N - xhat * sum_dy_xhat / N)
 * fp32 statistics whatever the storage type; C a multiple of 4, <= 1024; deterministic.  running_mean / running_var (fp32 [C],
 * both or neither; NULL: skipped) receive torch's update r = (1 - momentum) r + momentum * new with the unbiased variance;
 * num_batches_tracked (int64 [1] on the device, may be NULL) is incremented by the same launch (BatchNorm1d's buffer of that name). */
size_t dn_batchnorm_rows_workspace_bytes(int64_t N, int32_t C);
int dn_batchnorm_rows_f32(const float* X, int64_t N, int32_t C, const float* weight, const float* bias, float eps, float* Y, float* mean,
                          float* var, float* rstd, float* running_mean, float* running_var, float momentum, int32_t relu,
                          int64_t* num_batches_tracked, void* workspace, size_t workspace_bytes, dn_stream_t stream);
int dn_batchnorm_rows_bf16(const void* X, int64_t N, int32_t C, const float* weight, const float* bias, float eps, void* Y, float* mean,
                           float* var, float* rstd, float* running_mean, float* running_var, float momentum, int32_t relu,
                           int64_t* num_batches_tracked, void* workspace, size_t workspace_bytes, dn_stream_t stream);
int dn_batchnorm_rows_bwd_f32(const float* DY, const float* X, int64_t N, int32_t C, const float* mean, const float* rstd,
                              const float* weight, const float* bias, int32_t relu, float* DX, float* sum_dy, float* sum_dy_xhat,
                              void* workspace, size_t workspace_bytes, dn_stream_t stream);
int dn_batchnorm_rows_bwd_bf16(const void* DY, const void* X, int64_t N, int32_t C, const float* mean, const float* rstd,
                               const float* weight, const float* bias, int32_t relu, void* DX, float* sum_dy, float* sum_dy_xhat,
                               void* workspace, size_t workspace_bytes, dn_stream_t stream);

/* RGCN degree normalisation.  Replaces RGCNLayer._node_init_func/_edge_init_func
 * (subgraph_isomorphism/models/rgcn.py:132-165): in_norm = 1/(in_deg+1) with self-loop else 1/in_deg
 * (0 for isolated), same for out; edge norm = in_norm[dst] ("in", mode 1) or
 * sqrt(out_norm[src]*in_norm[dst]) ("both", mode 2).  Any output may be NULL. */
int dn_edge_norm_f32(int32_t mode, int32_t self_loop, int64_t N, int64_t E, const int32_t* src,
                     const int32_t* dst, const int32_t* in_deg, const int32_t* out_deg, float* in_norm,
                     float* out_norm, float* edge_norm, dn_stream_t stream);
/* in_deg / out_deg by counting (graph.in_degrees() / out_degrees(), rgcn.py:134,144). */
int dn_degrees_i32(int64_t N, int64_t E, const int32_t* src, const int32_t* dst, int32_t* in_deg,
                   int32_t* out_deg, dn_stream_t stream);

/* ---- SI count models (RGIN / RGCN): the glue of GraphAdjModel.forward around the rep nets (dn_simodel.hip) ----
 * Batches are ragged: node_ptr [B + 1] per side, rows of graph b = [node_ptr[b], node_ptr[b + 1]).  fp32 accumulation,
 * fixed-order sums, no float atomics.  dummy (uint8 [N], may be NULL): the is_dummy node flag. */
#define DN_SI_BAD_LABEL 1
#define DN_SI_BAD_ID 2
#define DN_SI_ZERO_PATTERN 4
#define DN_SI_ZERO_GRAPH 8
#define DN_SI_BAD_PTR 16
/* Label filter + batch metadata.  Replaces ScalarFilter + get_filter_gate (subgraph_isomorphism/models/filter.py:10-16,
 * basemodel.py:830-847) and the length / range facts the forward needs.  meta (int32 [4], zeroed here) = {Lp, Lg, flags, 0}:
 * the longest pattern / graph and the DN_SI_* bits (labels / ids outside [0, table rows), zero-node graphs, inconsistent ptrs).
 * gate (may be NULL; [Ng]) = 1 where the label of graph node v occurs in pattern b, or is 0 while pattern b is shorter than Lp
 * (the reference front-pads patterns with label 0 before it compares), else 0. */
int dn_si_filter_meta_f32(int64_t B, const int32_t* p_ptr, const int32_t* p_label, const int32_t* p_id, int64_t Np,
                          const int32_t* g_ptr, const int32_t* g_label, const int32_t* g_id, int64_t Ng, int32_t p_nlab,
                          int32_t p_nid, int32_t g_nlab, int32_t g_nid, float* gate, int32_t* meta, dn_stream_t stream);
int dn_si_filter_meta_bf16(int64_t B, const int32_t* p_ptr, const int32_t* p_label, const int32_t* p_id, int64_t Np,
                           const int32_t* g_ptr, const int32_t* g_label, const int32_t* g_id, int64_t Ng, int32_t p_nlab,
                           int32_t p_nid, int32_t g_nlab, int32_t g_nid, void* gate, int32_t* meta, dn_stream_t stream);
/* Code embedding.  Replaces get_*_enc + get_*_emb (basemodel.py:849-873): out[v] = enc1[key1[v]] @ W1 (+ enc2[key2[v]] @ W2
 * when key2 != NULL), enc [rows, K] the frozen encoder tables, W [K, H] (staged in LDS: (K1 + K2) * H <= 16384; H <= 256,
 * K <= 64). */
int dn_si_embed_fwd_f32(int64_t N, int32_t H, const int32_t* key1, const float* enc1, int32_t rows1, int32_t K1,
                        const float* W1, const int32_t* key2, const float* enc2, int32_t rows2, int32_t K2, const float* W2,
                        float* out, dn_stream_t stream);
int dn_si_embed_fwd_bf16(int64_t N, int32_t H, const int32_t* key1, const void* enc1, int32_t rows1, int32_t K1,
                         const void* W1, const int32_t* key2, const void* enc2, int32_t rows2, int32_t K2, const void* W2,
                         void* out, dn_stream_t stream);
/* Its weight gradient dW [K, H] = enc[key]^T @ G over the N rows (H <= 256, K <= 64): fixed 32-row partial sums, then an
 * ordered reduction. */
size_t dn_si_embed_wgrad_workspace_bytes(int64_t N, int32_t K, int32_t H);
int dn_si_embed_wgrad_f32(int64_t N, int32_t H, const int32_t* key, const float* enc, int32_t rows, int32_t K,
                          const float* G, float* dW, void* workspace, size_t workspace_bytes, dn_stream_t stream);
int dn_si_embed_wgrad_bf16(int64_t N, int32_t H, const int32_t* key, const void* enc, int32_t rows, int32_t K,
                           const void* G, void* dW, void* workspace, size_t workspace_bytes, dn_stream_t stream);
/* Ragged Sum / Mean head pooling.  Replaces the concatenation, padding and masking in front of the pred net
 * (basemodel.py:914-954, pred.py:17-216): pooled [B, D] fp32 = sum over the non-dummy rows of graph b of
 * [enc_v(id) | enc_vl(label) | out_deg | in_deg | rep] (id / label / degree parts optional: NULL leaves them out), count [B]
 * = the number of those rows.  Backward: drep[v] = dpooled[graph(v), col0 : col0 + H], 0 at dummy rows. */
int dn_si_pool_sum_f32(int64_t B, const int32_t* node_ptr, const uint8_t* dummy, const int32_t* id, const float* enc_v,
                       int32_t rows_v, int32_t Kv, const int32_t* label, const float* enc_vl, int32_t rows_vl, int32_t Kvl,
                       const int32_t* out_deg, const int32_t* in_deg, const float* rep, int32_t H, float* pooled,
                       int32_t* count, dn_stream_t stream);
int dn_si_pool_sum_bf16(int64_t B, const int32_t* node_ptr, const uint8_t* dummy, const int32_t* id, const void* enc_v,
                        int32_t rows_v, int32_t Kv, const int32_t* label, const void* enc_vl, int32_t rows_vl, int32_t Kvl,
                        const int32_t* out_deg, const int32_t* in_deg, const void* rep, int32_t H, float* pooled,
                        int32_t* count, dn_stream_t stream);
int dn_si_pool_sum_bwd_f32(int64_t B, const int32_t* node_ptr, const uint8_t* dummy, const float* dpooled, int32_t D,
                           int32_t col0, int32_t H, float* drep, dn_stream_t stream);
int dn_si_pool_sum_bwd_bf16(int64_t B, const int32_t* node_ptr, const uint8_t* dummy, const float* dpooled, int32_t D,
                            int32_t col0, int32_t H, void* drep, dn_stream_t stream);
/* Ragged Max head pooling (MaxPredictNet.agg_graph, pred.py:219-236, on the padded masked rows): out [B, C] = max of Y [N, C]
 * (g_fc applied per row) over the non-dummy rows of graph b, with bias[c] as one more candidate when graph b has fewer of
 * them than L (a zeroed padded row gives the bias).  argmax [B, C] = the winning row, -1 for the bias; first maximum wins.
 * Backward: dY[argmax[b, c], c] = dout[b, c] (dY zeroed by the caller). */
int dn_si_pool_max_f32(int64_t B, const int32_t* node_ptr, const uint8_t* dummy, const float* Y, int32_t C,
                       const float* bias, int32_t L, float* out, int32_t* argmax, dn_stream_t stream);
int dn_si_pool_max_bf16(int64_t B, const int32_t* node_ptr, const uint8_t* dummy, const void* Y, int32_t C,
                        const void* bias, int32_t L, void* out, int32_t* argmax, dn_stream_t stream);
int dn_si_pool_max_bwd_f32(int64_t B, int32_t C, const int32_t* argmax, const float* dout, float* dY, dn_stream_t stream);
int dn_si_pool_max_bwd_bf16(int64_t B, int32_t C, const int32_t* argmax, const void* dout, void* dY, dn_stream_t stream);
/* The padded node mask [B, L] (uint8) of batch_convert_len_to_mask(pre_pad=True) with the dummy positions cleared
 * (utils/dl.py:113-127, basemodel.py:892-912), in one launch instead of a fill per graph. */
int dn_si_len_mask_u8(int64_t B, int32_t L, const int32_t* node_ptr, const uint8_t* dummy, uint8_t* mask,
                      dn_stream_t stream);

/* ---- dual (node + edge) message passing of the SI models CompGCN / DMPNN, and the ragged edge head (dn_dual.hip) ----
 * Dual aggregation, one pass over a grouped edge list (CSR by destination: perm = the edges grouped by dst):
 *     out[d][v] = sum over e in list(v) with rev_e == d of scale_e * m_e,   d = 0 (forward) | 1 (reversed),  out = [2, N, H]
 *     m_e = ef_e (DN_DUAL_EDGE) | x[src_e] - ef_e (DN_DUAL_SUB) | x[src_e] * ef_e (DN_DUAL_MULT)
 * rev (uint8 [E]) and scale (fp32 [E], edge order) may be NULL.  units = int32 [U, 4] records {segment, first entry, end entry,
 * slot}: slot < 0 = the unit is the whole segment and writes out[.][segment]; slot >= 0 = one chunk of a long segment, its two
 * fp32 partial rows go to part [P, 2, H] (the caller folds the chunks of a segment in order).  fp32 sums in list order, no
 * atomics.  out_f32 != 0: out holds the fp32 sums whatever the row dtype (for a caller that adds two passes before it rounds).
 * Nothing is read outside [0, E) / [0, N): such an entry counts as zero.  H <= 256. */
#define DN_DUAL_EDGE 0
#define DN_DUAL_SUB 1
#define DN_DUAL_MULT 2
int dn_dual_agg_f32(int32_t mode, int64_t N, int64_t E, int32_t H, int64_t U, const int32_t* units, const int32_t* perm,
                    const int32_t* src, const uint8_t* rev, const float* scale, const float* ef, const float* x, float* out,
                    int32_t out_f32, float* part, int64_t P, dn_stream_t stream);
int dn_dual_agg_bf16(int32_t mode, int64_t N, int64_t E, int32_t H, int64_t U, const int32_t* units, const int32_t* perm,
                     const int32_t* src, const uint8_t* rev, const float* scale, const void* ef, const void* x, void* out,
                     int32_t out_f32, float* part, int64_t P, dn_stream_t stream);
/* Backward, with G_e = scale_e * g[rev_e][dst_e] (g = [2, N, H]):
 * edge: d_ef[e] = G_e | -G_e | G_e * x[src_e];   node (sub / mult only): dx[u] = sum over the out-list of u (units / perm of
 * the CSC by source) of G_e | G_e * ef_e, partial rows part [P, H]. */
int dn_dual_agg_bwd_edge_f32(int32_t mode, int64_t N, int64_t E, int32_t H, const int32_t* src, const int32_t* dst,
                             const uint8_t* rev, const float* scale, const float* g, const float* x, float* d_ef,
                             dn_stream_t stream);
int dn_dual_agg_bwd_edge_bf16(int32_t mode, int64_t N, int64_t E, int32_t H, const int32_t* src, const int32_t* dst,
                              const uint8_t* rev, const float* scale, const void* g, const void* x, void* d_ef,
                              dn_stream_t stream);
int dn_dual_agg_bwd_node_f32(int32_t mode, int64_t N, int64_t E, int32_t H, int64_t U, const int32_t* units,
                             const int32_t* perm, const int32_t* dst, const uint8_t* rev, const float* scale, const float* g,
                             const float* ef, float* dx, float* part, int64_t P, dn_stream_t stream);
int dn_dual_agg_bwd_node_bf16(int32_t mode, int64_t N, int64_t E, int32_t H, int64_t U, const int32_t* units,
                              const int32_t* perm, const int32_t* dst, const uint8_t* rev, const float* scale, const void* g,
                              const void* ef, void* dx, float* part, int64_t P, dn_stream_t stream);
/* DMP edge update (dmpnn.py:111-169): out[e] = (p_loop[e] + coef[dst_e] * p_diff[e]) + (xd[a_e] - xs[b_e]) + ebias with
 * p_loop = ef W_eloop, p_diff = ef (W_src - W_dst) ([E, H]), xd = x W_dst, xs = x W_src ([N, H]), coef [N] fp32
 * (= 2 (1 + log2(1 + out_deg))), (a, b) = (dst, src) on forward edges and (src, dst) on reversed ones (rev may be NULL), ebias
 * [H] or NULL.  Backward piece: d_diff[e] = coef[dst_e] * g[e]. */
int dn_dual_edge_update_f32(int64_t N, int64_t E, int32_t H, const int32_t* src, const int32_t* dst, const uint8_t* rev,
                            const float* coef, const float* p_loop, const float* p_diff, const float* xd, const float* xs,
                            const float* ebias, float* out, dn_stream_t stream);
int dn_dual_edge_update_bf16(int64_t N, int64_t E, int32_t H, const int32_t* src, const int32_t* dst, const uint8_t* rev,
                             const float* coef, const void* p_loop, const void* p_diff, const void* xd, const void* xs,
                             const void* ebias, void* out, dn_stream_t stream);
int dn_dual_edge_update_bwd_f32(int64_t N, int64_t E, int32_t H, const int32_t* dst, const float* coef, const float* g,
                                float* d_diff, dn_stream_t stream);
int dn_dual_edge_update_bwd_bf16(int64_t N, int64_t E, int32_t H, const int32_t* dst, const float* coef, const void* g,
                                 void* d_diff, dn_stream_t stream);
/* Ragged Sum / Mean pooling of the edge head rows (basemodel.py:1622-1667): pooled [B, D] fp32 = sum over the edges e = (u, v) of
 * graph b with skip[e] == 0 (skip = is_dummy | is_reversed, may be NULL) of
 * [enc_v(id[u]) | enc_v(id[v]) | enc_vl(vlabel[u]) | enc_el(elabel[e]) | enc_vl(vlabel[v]) | out_deg[u] | in_deg[v] | rep[e]]
 * (the encoder part: all three keys or none; the degree part optional), count [B] = the kept edges.  The backward is
 * dn_si_pool_sum_bwd_* on edge_ptr and skip. */
int dn_sie_pool_sum_f32(int64_t B, const int32_t* edge_ptr, const uint8_t* skip, const int32_t* src, const int32_t* dst, int64_t N,
                        const int32_t* id, const float* enc_v, int32_t rows_v, int32_t Kv, const int32_t* vlabel,
                        const float* enc_vl, int32_t rows_vl, int32_t Kvl, const int32_t* elabel, const float* enc_el,
                        int32_t rows_el, int32_t Kel, const int32_t* out_deg, const int32_t* in_deg, const float* rep, int32_t H,
                        float* pooled, int32_t* count, dn_stream_t stream);
int dn_sie_pool_sum_bf16(int64_t B, const int32_t* edge_ptr, const uint8_t* skip, const int32_t* src, const int32_t* dst, int64_t N,
                         const int32_t* id, const void* enc_v, int32_t rows_v, int32_t Kv, const int32_t* vlabel,
                         const void* enc_vl, int32_t rows_vl, int32_t Kvl, const int32_t* elabel, const void* enc_el,
                         int32_t rows_el, int32_t Kel, const int32_t* out_deg, const int32_t* in_deg, const void* rep, int32_t H,
                         float* pooled, int32_t* count, dn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Mini-batch assembly from a device-resident dataset: ONE launch builds a batch's tensors from the packed dataset's columns
 * (a batched ragged copy with optional integer re-basing).
 * Replaces: the host-side collate of every training step -- DataLoader + torch_geometric Batch.from_data_list
 *   (graph_classification/graph_neural_networks/main.py:245-247) and batchify -> dgl.batch
 *   (subgraph_isomorphism/dataset.py:1321-1328, 1605-1611).
 * The dataset keeps, per column, the rows of graph i in [ds_ptr[i], ds_ptr[i+1]) -- ds_node_ptr for node-level columns,
 * ds_edge_ptr for edge-level ones, row i for graph-level ones; num_ds_graphs = the number of graphs behind those arrays.
 * table = {ids [B], out_node_ptr [B+1], out_edge_ptr [B+1]} int32, one device array: output graph k = dataset graph ids[k]
 * (any order, duplicates allowed), its rows go to [out_ptr[k], out_ptr[k+1]) of every column; N = out_node_ptr[B],
 * E = out_edge_ptr[B] (the caller planned them on the host).  A graph whose id is outside [0, num_ds_graphs) or whose planned
 * size differs from the dataset's is skipped, never read.
 * Column c copies row_bytes (>= 1, any value) bytes per row from src to dst; the two sides may be aligned differently.
 * rebase != DN_BATCH_REBASE_NONE: the rows are integers of int_width (4 or 8) bytes, row_bytes a multiple of it, src and dst
 * aligned to it, and every value v is written as  v - base_in + base_out:  base_out = out_node_ptr[k] (REBASE_NODE) or
 * out_edge_ptr[k] (REBASE_EDGE); base_in = 0 when the dataset stores graph-local values (src_global == 0: the endpoints of an
 * edge list), ds_node_ptr[i] / ds_edge_ptr[i] when it stores dataset-global ones (src_global != 0: a CSR built over the whole
 * dataset).  ptr_tail != 0 (re-based columns only): one more value behind the column's last row, = N or E by `rebase` (the closing
 * entry of a CSR pointer array).  batch_out (may be NULL) [N] int64: k for every node of output graph k (the PyG `batch` vector).
 * num_cols <= DN_BATCH_MAX_COLS.  No atomics, no workspace; B == 0 or nothing to write: returns 0 without a launch. */
#define DN_BATCH_MAX_COLS 32
#define DN_BATCH_LEVEL_NODE 0
#define DN_BATCH_LEVEL_EDGE 1
#define DN_BATCH_LEVEL_GRAPH 2
#define DN_BATCH_REBASE_NONE 0
#define DN_BATCH_REBASE_NODE 1
#define DN_BATCH_REBASE_EDGE 2
typedef struct dn_batch_col {
    const void* src;
    void* dst;
    int32_t row_bytes, level, rebase, int_width, src_global, ptr_tail;
} dn_batch_col;
int dn_batch_assemble(int64_t B, const int32_t* table, const int32_t* ds_node_ptr, const int32_t* ds_edge_ptr,
                      int64_t num_ds_graphs, int64_t N, int64_t E, const dn_batch_col* host_cols, int32_t num_cols,
                      int64_t* batch_out, dn_stream_t stream);

/* ---- LRP (local relational pooling) of the SI count model LRP: ego-net permutation index and pooling (dn_lrp.hip) ----
 * The ego index of a batch: uptr [N + 1] / unbr / ueid = the sorted, duplicate-free out-neighbour lists over the edges that count
 * (is_reversed == 0) with the LAST edge id of every (u, w) -- built by the caller -- and, from dn_lrp_ego_index_i32:
 *     upos  [uptr[N]]  per node the positions (into its neighbour list) of its non-dummy neighbours, then of its dummy neighbours
 *     ego   [N, 2]     {kind, dummy neighbours}: kind 0 = permutations of the neighbours, 1 = the node is a dummy (combinations),
 *                      2 = the node has dummy neighbours (permutations of the others, one dummy neighbour last)
 *     count [N] int64  sequences of the node for sequence length L (2, 3 or 4); saturates at INT64_MAX
 *     err   [2]        caller-initialised {INT32_MAX, 0}: [0] = the smallest node with a self-loop, [1] bit 0 = a count saturated
 * dummy (uint8 [N]) may be NULL.  N == 0: returns 0 without a launch (as every entry point below). */
int dn_lrp_ego_index_i32(int64_t N, int32_t L, const int32_t* uptr, const int32_t* unbr, const uint8_t* dummy, int32_t* upos,
                         int32_t* ego, int64_t* count, int32_t* err, dn_stream_t stream);
/* The materialised index: perm_nodes [P, L] and perm_edges [P, L * L] (-1 = empty) for perm_ptr [N + 1] = the exclusive scan of
 * count; sequence p of node v fills slot k (L + 1) with its k-th node and slot a L + b with eid(node a, node b) where that edge
 * exists.  Order: the reference's (subgraph_isomorphism/dataset.py:1750-1823).  P * L * L must fit int32. */
int dn_lrp_perm_fill_i32(int64_t N, int32_t L, const int32_t* uptr, const int32_t* unbr, const int32_t* ueid, const int32_t* upos,
                         const int32_t* ego, const int64_t* count, const int32_t* perm_ptr, int64_t P, int32_t* perm_nodes,
                         int32_t* perm_edges, dn_stream_t stream);
/* The collapsed index of DMPLRP (subgraph_isomorphism/models/dmplrp.py:180-185: the contraction of the sequences of
 * dataset.py:1843-1886 is pooled with nothing non-linear in between, so the pooled row of a node is a weighted sum of table rows).
 * Per node the distinct table rows its sequences touch, each with its number of occurrences, from closed forms in the ego index
 * (nothing is enumerated or sized by the sequence count).  Rows: node u at position k -> u L + k; edge eid in slot (a, b), a != b
 * -> N L + eid L (L - 1) + a (L - 1) + (b > a ? b - 1 : b); N L + E L (L - 1) must fit int32.  count -> scan -> fill:
 *     dn_lrp_collapse_count_i32   col_count [N] int64 = the rows of every node
 *     dn_lrp_collapse_fill_i32    col_rows [Q] int32 / col_cnt [Q] int64 for col_ptr [N + 1] = the exclusive scan of col_count
 * Slots come from workgroup scans (no atomics: two builds store the same lists); the rows of a node are stored in the kernel's
 * candidate order, not ascending.  dummy (uint8 [N]) may be NULL.  The index must be free of self-loops (dn_lrp_ego_index_i32). */
int dn_lrp_collapse_count_i32(int64_t N, int64_t E, int32_t L, const int32_t* uptr, const int32_t* unbr, const int32_t* ueid,
                              const int32_t* upos, const int32_t* ego, const int64_t* count, const uint8_t* dummy, int64_t* col_count,
                              dn_stream_t stream);
int dn_lrp_collapse_fill_i32(int64_t N, int64_t E, int32_t L, const int32_t* uptr, const int32_t* unbr, const int32_t* ueid,
                             const int32_t* upos, const int32_t* ego, const int64_t* count, const uint8_t* dummy, const int32_t* col_ptr,
                             int64_t Q, int32_t* col_rows, int64_t* col_cnt, dn_stream_t stream);
/* LDS budget of the pooling kernels: an ego of d + 1 nodes keeps its T_node rows in LDS when (d + 1) L H 4 <= dn_lrp_stage_bytes()
 * and its pair -> edge table when d + 1 <= dn_lrp_pair_nodes(); larger egos read through L2. */
int32_t dn_lrp_stage_bytes(void);
int32_t dn_lrp_pair_nodes(void);
/* out [N, H] = act2(pool_p(act(sum_k t_node[node_k(p)][k] + sum_(a != b) t_edge[eid_ab(p)][slot(a, b)] + bias)) * factor), one
 * workgroup per node, the sequences enumerated in the kernel from the ego index; nothing of size P is stored.
 * t_node [N, L, H] (x times the diagonal slots of the weight), t_edge [E, L (L - 1), H] (edge features times the off-diagonal
 * slots, in slot order); bias [H] and factor [N, H] may be NULL (no factor: no scale and no second activation); pool_mean: mean
 * instead of sum; act_on: leaky ReLU of `slope` (0: ReLU), else the identity.  pooled [N, H] (may be NULL) receives the pooled
 * value in front of the factor (the backward needs it when factor is given).  H a multiple of 16, 16 <= H <= 256. */
int dn_lrp_pool_fwd_f32(int64_t N, int64_t E, int32_t H, int32_t L, const int32_t* uptr, const int32_t* unbr, const int32_t* ueid,
                        const int32_t* upos, const int32_t* ego, const int64_t* count, const float* t_node, const float* t_edge,
                        const float* bias, const float* factor, int32_t pool_mean, int32_t act_on, float slope, float* pooled,
                        float* out, dn_stream_t stream);
/* Backward: recomputes every sequence and ADDS its gradient rows into d_tnode [N, L, H], d_tedge [E, L (L - 1), H] and d_bias [H]
 * (may be NULL) with fp32 atomics -- the caller zeroes them; sums across egos are exact but their order is not fixed.  d_factor
 * [N, H] is stored (needs factor and pooled). */
int dn_lrp_pool_bwd_f32(int64_t N, int64_t E, int32_t H, int32_t L, const int32_t* uptr, const int32_t* unbr, const int32_t* ueid,
                        const int32_t* upos, const int32_t* ego, const int64_t* count, const float* t_node, const float* t_edge,
                        const float* bias, const float* factor, int32_t pool_mean, int32_t act_on, float slope, const float* pooled,
                        const float* g, float* d_tnode, float* d_tedge, float* d_bias, float* d_factor, dn_stream_t stream);

/* ---- HGT edge-softmax attention of the SI count model HGT (dn_hgt.hip) ----
 * The edges sorted by (destination, edge type).  A pair is a (destination, edge type) with at least one edge, numbered in that
 * order: dst_ptr [N + 1] bounds the pairs of every destination, pair_ptr [P + 1] the edges of every pair, pair_rel [P] is the pair's
 * edge type.  The per-pair tensors are stored grouped by edge type (the order of the relation-grouped products): pair_row [P] is
 * the row of a pair; src_s / et_s / row_s [E] are the source, the type and the pair's row of every edge in sorted order.
 * Qp [P, H] holds the query of the pair's destination already multiplied by the type's block-diagonal attention matrix, K / V
 * [N, H] the plain key and value rows, pri [R, heads].  Per destination and head
 *     logit_e = <Qp[row_e, h], K[src_e, h]> * pri[et_e, h] * scale,   a = softmax over ALL in-edges of dst (max subtracted)
 *     att [E, heads] = a (sorted order),   U [P, H]: U[pair_row[p]] = sum over the edges of pair p of a_e * V[src_e]
 * One workgroup per destination, nothing of size E x H is stored.  heads in {1, 2, 4, 8}, H <= 256, H / heads a multiple of 4.
 * N == 0: returns 0 without a launch. */
int dn_hgt_attn_fwd_f32(int64_t N, int64_t E, int64_t P, int32_t H, int32_t heads, const int32_t* dst_ptr, const int32_t* pair_ptr,
                        const int32_t* pair_row, const int32_t* src_s, const int32_t* et_s, const int32_t* row_s, const float* Qp,
                        const float* K, const float* V, const float* pri, float scale, float* att, float* U, dn_stream_t stream);
/* Backward in destination order from dU [P, H]: dl [E, heads] = the gradient of the raw dot products (softmax backward
 * a (da - sum a da), times pri and scale), dQp [P, H], and dpri_part [P, heads] = every pair's partial of d pri, both at the
 * pair's row (the caller sums the rows of each type).  No atomics. */
int dn_hgt_attn_bwd_dst_f32(int64_t N, int64_t E, int64_t P, int32_t H, int32_t heads, const int32_t* dst_ptr, const int32_t* pair_ptr,
                            const int32_t* pair_rel, const int32_t* pair_row, const int32_t* src_s, const int32_t* row_s, const float* Qp,
                            const float* K, const float* V, const float* pri, float scale, const float* att, const float* dU, float* dl,
                            float* dQp, float* dpri_part, dn_stream_t stream);
/* Backward in source order over the reverse CSR out_ptr [N + 1] with, per entry, the edge's position in the destination order
 * (out_pos) and the row of its pair (out_row): dK[s] = sum dl_e Qp[row_e], dV[s] = sum a_e dU[row_e].  No atomics. */
int dn_hgt_attn_bwd_src_f32(int64_t N, int64_t E, int64_t P, int32_t H, int32_t heads, const int32_t* out_ptr, const int32_t* out_pos,
                            const int32_t* out_row, const float* Qp, const float* dU, const float* att, const float* dl, float* dK,
                            float* dV, dn_stream_t stream);

/* ---- an RGIN layer's backward with Linear 1's weight gradient derived from the conv's (dn_chain_wgrad.hip; bf16, H = 256) ----
 * Nothing lies between the conv's output h and the MLP's first Linear, so with g1 = the gradient of z1 = h W1^T + b1,
 * M_r = A_r^T g1 (the conv's weight-gradient launch run on g1 instead of g0 = g1 W1; r = 0 .. R - 1, then the self loop) and
 * c = colsum(g1):   dWc_r = M_r W1,  db = c W1,  dW1 = sum_r M_r^T Wc_r + c b^T,  db1 = c.
 *
 * dn_layer_chain_dgrad_bf16: G0 = G1 @ W_kn (the dense ring transform: bit-identical to dn_mlp_bwd_fused_bf16's g_next without
 * masks) over `tiles` [T, 4] = {0, first row, end row, s0 | s1 << 8}: consecutive row ranges of at most 32 rows (a graph each) that
 * cover the rows the caller wants; seg_sums [T, H] (bf16) receives per tile the sum of G1's rows first + s0 .. first + s1 - 1 taken
 * in row order in fp32 from zero and rounded once -- dn_gather_segsum_bf16 over the same contiguous lists, from the launch
 * that reads every G1 row anyway.  0 <= s0 <= s1 <= end - first.  N = the rows of G1 / G0 (every tile must lie inside [0, N): checked
 * by the caller, the launch reads the table on the device).  Tiles must not be empty: a trailing run of empty tiles of a workgroup
 * is not walked, and their rows of seg_sums stay unwritten (an empty tile in front of a live one gets a zero row). */
int dn_layer_chain_dgrad_bf16(const void* G1, const void* W_kn, int64_t N, int32_t H, const int32_t* tiles, int64_t num_tiles, void* G0,
                              void* seg_sums, dn_stream_t stream);
/* dn_layer_chain_wgrad_combine: M fp32 [R + 1, H, H] (the self loop last), c fp32 [H], W1 [out, in] as nn.Linear stores it, Wc
 * [R, in, out] and Wc_loop [in, out] as the layer stores them, bias [H] (may be NULL) -> dWc [R + 1, H, H], db [H] (may be NULL),
 * dW1 [H, H], db1 [H] (may be NULL), all bf16 with ONE rounding each.  M is never rounded: the products of its fp32 values with the
 * bf16 weights (32 significant bits) are accumulated in fp64 FMA tiles, where they are exact, so an output that cancels far below its
 * terms is still within one bf16 ulp of the exact value.  dW1's K = (R + 1) H is split over the relations; the fp64 partial products
 * are summed in relation order: no atomics.  workspace: dn_layer_chain_wgrad_combine_workspace_bytes(R, H) (16-byte aligned). */
size_t dn_layer_chain_wgrad_combine_workspace_bytes(int64_t R, int32_t H);
int dn_layer_chain_wgrad_combine(const float* M, const float* c, const void* W1, const void* Wc, const void* Wc_loop, const void* bias,
                                 int64_t R, int32_t H, void* dWc, void* db, void* dW1, void* db1, void* workspace,
                                 size_t workspace_bytes, dn_stream_t stream);

/* ---- Weisfeiler-Lehman graph kernels at k = 1: WL and WLOA (dn_wl.hip) ----
 * Colours are unsigned 64-bit values carried as int64 bit patterns; all arithmetic wraps mod 2^64 and every comparison is
 * unsigned.  pairing(a, b) = a >= b ? a a + a + b : a + b b.  The graph is the deduplicated undirected CSR of a whole dataset:
 * ptr [num_nodes + 1], nbr [ptr[num_nodes]] (global node ids), edge_label [ptr[num_nodes]] per slot or NULL.
 *
 * dn_wl_refine_u64: one refinement step for the nodes nodes[0 .. num_list) (NULL: every node, num_list == num_nodes).  A node's
 * entries are colors_in[n] for every neighbour n and, with edge labels, also pairing(colors_in[n], label); colors_out[v] = the
 * fold c = pairing(c, entry) over the ascending entries, starting from colors_in[v].  group = lanes per node: 8 or 64 (lists of at
 * most that many entries, one per lane, sorted by a shuffle network) or 0 (one workgroup per node, lists of at most lds_entries
 * entries -- a power of two <= dn_wl_max_entries() -- sorted in LDS).  A node whose list is longer than its launch takes is left
 * unwritten: the caller classes the nodes (once per dataset) and sends longer lists through a device-wide segmented sort and
 * dn_wl_fold_u64.  colors_out must not alias colors_in. */
int32_t dn_wl_max_entries(void);
int dn_wl_refine_u64(int64_t num_nodes, int64_t num_list, const int32_t* nodes, int32_t group, int32_t lds_entries, const int32_t* ptr,
                     const int32_t* nbr, const int64_t* edge_label, const int64_t* colors_in, int64_t* colors_out, dn_stream_t stream);
/* The fold alone over lists the caller has sorted: list s = sorted_entries[seg_ptr[s] .. seg_ptr[s + 1]) ascending (unsigned),
 * colors_out[v] for v = nodes[s] (NULL: v = s).  One thread per list, any length. */
int dn_wl_fold_u64(int64_t num_nodes, int64_t num_list, const int32_t* nodes, const int64_t* seg_ptr, const int64_t* sorted_entries,
                   const int64_t* colors_in, int64_t* colors_out, dn_stream_t stream);
/* All num_steps = H + 1 gram matrices in one pass from the feature CSR: row g = feat_ptr[g] .. feat_ptr[g + 1] holds graph g's
 * distinct colours ascending (unsigned) with a count and a step (0 <= step < num_steps) each.  out [num_steps, B, B] (int64):
 * out[h, i, j] = sum over the colours common to i and j with max(step_i, step_j) <= h of count_i count_j (use_min = 0: WL) or
 * min(count_i, count_j) (use_min != 0: WLOA).  Every element is written (the upper triangle is computed, the lower mirrored).  A
 * workgroup takes dn_wl_gram_tile()^2 pairs, a thread one pair: a merge join of two rows of any length, read from global memory,
 * into num_steps <= dn_wl_max_steps() buckets in LDS.  Integer sums only: no atomics, two runs give the same bits. */
int32_t dn_wl_max_steps(void);
int32_t dn_wl_gram_tile(void);
int dn_wl_gram_i64(int64_t num_graphs, int32_t num_steps, int32_t use_min, const int32_t* feat_ptr, const int64_t* feat_color,
                   const int32_t* feat_count, const int32_t* feat_step, int64_t* out, dn_stream_t stream);

/* ---- shortest-path and graphlet graph kernels (graph_classification/graph_kernels: `gram --kernel SP | GR`): the feature extractors.
 * Both work on the dataset CSR of the dn_wl_* entry points and produce (graph, key, count) entries that the caller sorts into the
 * feature CSR of dn_wl_gram_i64 (one step, use_min = 0).
 *
 * dn_gk_sp_u64: one BFS per source node over bit sets, for the graphs graphs[0 .. num_list).  group = 64: a wavefront per graph, a
 * lane per source (graphs of at most 64 nodes); group = 0: a workgroup per graph with the adjacency bit matrix in LDS (graphs of at
 * most lds_nodes <= dn_gk_sp_lds_max_nodes() nodes).  A graph larger than its launch takes is left alone.  A source a emits, for every
 * label class c of its graph and every level d that reaches nodes of c, the entry key = ((src_base[a] + class_rank[class_ptr[g] + c])
 * << 32) | d with their number; likewise the nodes it cannot reach at d = INT_MAX, and itself with count 2 at d = 2 (INT_MAX without a
 * neighbour).  src_base[a] < 0: the source is filtered.  local_class[v] is v's class within its graph (0 .. class_ptr[g + 1] -
 * class_ptr[g]).  offsets == NULL: the counting pass, counts[a] = entries of source a (untouched for filtered sources and for graphs
 * left alone, so the caller zeroes it).  offsets != NULL: the fill, entries of a at out_key / out_count [offsets[a] ..), never at or
 * beyond out_entries. */
int32_t dn_gk_sp_lds_max_nodes(void);
int dn_gk_sp_u64(int64_t num_graphs, int64_t num_list, const int32_t* graphs, int32_t group, int32_t lds_nodes, const int32_t* node_ptr,
                 const int32_t* ptr, const int32_t* nbr, const int64_t* src_base, const int32_t* local_class, const int32_t* class_ptr,
                 const int32_t* class_rank, int32_t* counts, const int64_t* offsets, int64_t out_entries, int64_t* out_key,
                 int32_t* out_count, dn_stream_t stream);
/* dn_gk_gr_keys_u64: the 3-node graphlet keys.  Item k is the centre item_node[k] with the rows item_row0[k] .. item_row1[k] of its
 * ascending neighbour list; row i pairs neighbour i with every later neighbour j, and the item's pairs own the workspace slots
 * item_offset[k] .. in that order.  Adjacent pair: a triangle, keyed only where the centre is its smallest node (ws_graph = -1
 * elsewhere); else a wedge.  Keys: 2 / 3 without node labels; with them the reference's pairing folds (minimum over both directions
 * of a wedge, sorted labels or the six-way minimum of a triangle).  group = lanes per item: 8 or 64 (items of at most that many
 * pairs) or 0 (a workgroup per item, any length).  Nothing is written at or beyond workspace_keys. */
int dn_gk_gr_keys_u64(int64_t num_nodes, int64_t num_items, int32_t group, const int32_t* item_node, const int32_t* item_row0,
                      const int32_t* item_row1, const int64_t* item_offset, const int32_t* ptr, const int32_t* nbr, const int64_t* node_label,
                      const int64_t* edge_label, const int32_t* node_graph, int64_t workspace_keys, int64_t* ws_key, int32_t* ws_graph,
                      dn_stream_t stream);

/* ---- Weisfeiler-Lehman graph kernels at k = 2: WL, DWL, LWL and LWLC (dn_kwl.hip) ----
 * The items are the node pairs ("tuples") of every graph of the dataset CSR of the dn_wl_* entry points: tuple t = (tup_v[t],
 * tup_w[t]) (global node ids of one graph), graph after graph, rows in node order, a row's tuples by ascending second component.
 * WL, DWL and LWL have all n^2 pairs of a graph; LWLC ("connected") only (i, j) with i == j or j adjacent to i.  C[a, b] is the colour
 * of tuple (a, b) in colors_in.  A multiset is folded as: sort ascending (unsigned), start from the maximum, pairing(acc, x) over
 * the rest in ascending order.  Every neighbour colour enters its multiset TWICE.  The new colour is the tuple's own colour folded
 * over its local folds in ascending order, then over its global folds in ascending order; a tuple without any keeps its colour.
 *
 * dn_kwl_init_u64: colors_out[t] = pairing(pairing(ci, cj), c) with ci = pairing(node_label[v] + 1, 1) (1 without labels), cj =
 * pairing(node_label[w] + 1, 2) (2 without), c = 3 or pairing(3, edge_label[slot of w in v's list]) for adjacent v, w, 1 for v == w,
 * else 2. */
int dn_kwl_init_u64(int64_t num_nodes, int64_t num_tuples, const int32_t* tup_v, const int32_t* tup_w, const int32_t* ptr, const int32_t* nbr,
                    const int64_t* node_label, const int64_t* edge_label, int64_t* colors_out, dn_stream_t stream);
/* dn_kwl_local_u64: one LWL (connected = 0) or LWLC (connected != 0) step for the tuples tuples[0 .. num_list) (NULL: every tuple).
 * Local multiset 1 = C[x, w] for x adjacent to v, local multiset 2 = C[v, x] for x adjacent to w; LWLC keeps the x for which that
 * pair is a tuple.  row_ptr[a] = index of the first tuple of row a, node_first[a] = first node of a's graph.  group = lanes per tuple:
 * 8 or 64 (both degrees at most that) or 0 (one workgroup per tuple, both degrees at most lds_entries, a power of two <=
 * dn_kwl_max_entries()).  A tuple with a longer list than its launch takes is left unwritten. */
int32_t dn_kwl_max_entries(void);
int dn_kwl_local_u64(int64_t num_nodes, int64_t num_tuples, int64_t num_list, const int32_t* tuples, int32_t group, int32_t lds_entries,
                     int32_t connected, const int32_t* tup_v, const int32_t* tup_w, const int32_t* row_ptr, const int32_t* node_first,
                     const int32_t* ptr, const int32_t* nbr, const int64_t* colors_in, int64_t* colors_out, dn_stream_t stream);
/* dn_kwl_global_u64: one WL (malkin = 0) or DWL (malkin != 0) step for the graphs graphs[0 .. num_list), a workgroup per graph with
 * its colour matrix in LDS: graphs of at most lds_nodes nodes (a power of two <= dn_kwl_max_nodes()); a larger one is left unwritten.
 * Multiset 1 = C[x, w] for every x != v and the tuple's own colour FOUR times, multiset 2 = C[v, x] for every x != w.  WL: both are
 * local.  DWL: x goes to the local multiset where it is adjacent to the exchanged node (v for 1, w for 2), else to the global one, and
 * the four own copies to global 1.  tuple_ptr [num_graphs + 1]: first tuple of every graph (n^2 each).  work: scratch of num_tuples
 * values (2 num_tuples for DWL), aliasing neither colour array. */
int32_t dn_kwl_max_nodes(void);
int dn_kwl_global_u64(int64_t num_graphs, int64_t num_tuples, int64_t num_list, const int32_t* graphs, int32_t lds_nodes, int32_t malkin,
                      const int32_t* node_ptr, const int32_t* tuple_ptr, const int32_t* ptr, const int32_t* nbr, const int64_t* colors_in,
                      int64_t* colors_out, int64_t* work, dn_stream_t stream);

/* ---- Weisfeiler-Lehman graph kernels at k = 3: WL, DWL, LWL and LWLC (dn_k3wl.hip) ----
 * The items are node triples of every graph of the same dataset CSR: item t = (tup_v[t], tup_w[t], tup_u[t]) (global node ids of one
 * graph), graph after graph; tuple_ptr [num_graphs + 1]: first item of every graph.  WL, DWL and LWL have all n^3 triples of a graph,
 * row-major.  LWLC ("connected") has (i, i, i), then (i, i, j) for adjacent i, j, then pairwise distinct (i, j, k) with at least two
 * adjacent pairs; its items are found through item_key (per graph ascending keys (i n + j) n + k of local node numbers) and item_slot
 * (the item of every key).  C[a, b, c] is the colour of item (a, b, c) in colors_in.  Multisets, folds and the final combination are
 * those of k = 2: every neighbour colour enters TWICE, local folds ascending, then global folds ascending.
 *
 * dn_k3wl_init_u64: colors_out[t] = pairing(pairing(pairing(a, b), c), pairing(pairing(ci, cj), ck)); ci = pairing(node_label[v] + 1,
 * 1), cj = pairing(node_label[w] + 1, 2), ck = pairing(node_label[u] + 1, 3) (1, 2, 3 without labels); a, b, c code the pairs (v, w),
 * (v, u), (w, u): 1 adjacent, 2 not; connected: 3 adjacent, 1 the same node, 2 neither.  There are no edge labels at k = 3. */
int dn_k3wl_init_u64(int64_t num_nodes, int64_t num_items, int32_t connected, const int32_t* tup_v, const int32_t* tup_w,
                     const int32_t* tup_u, const int32_t* ptr, const int32_t* nbr, const int64_t* node_label, int64_t* colors_out,
                     dn_stream_t stream);
/* dn_k3wl_local_u64: one LWL (connected = 0) or LWLC (connected != 0) step for the items items[0 .. num_list) (NULL: every item).
 * LWL: three local multisets, C[x, w, u] for x adjacent to v, C[v, x, u] for x adjacent to w, C[v, w, x] for x adjacent to u.  LWLC:
 * the same entries where that triple is an item, the first two exchanges in ONE multiset, the third in another (item_key / item_slot
 * may be NULL for LWL).  node_graph[a] = graph of node a.  group = lanes per item: 8 or 64 (every list at most that long) or 0 (one
 * workgroup per item, every list at most lds_entries, a power of two <= 2 dn_k3wl_max_entries(): LWLC's merged list of a graph whose
 * largest degree is dn_k3wl_max_entries()).  An item with a longer list than its launch takes is left unwritten. */
int32_t dn_k3wl_max_entries(void);
int dn_k3wl_local_u64(int64_t num_nodes, int64_t num_items, int64_t num_list, const int32_t* items, int32_t group, int32_t lds_entries,
                      int32_t connected, const int32_t* tup_v, const int32_t* tup_w, const int32_t* tup_u, const int32_t* node_graph,
                      const int32_t* node_ptr, const int32_t* tuple_ptr, const int32_t* ptr, const int32_t* nbr, const int64_t* item_key,
                      const int32_t* item_slot, const int64_t* colors_in, int64_t* colors_out, dn_stream_t stream);
/* dn_k3wl_global_u64: the fibre pass of one WL (malkin = 0) or DWL (malkin != 0) step for the graphs graphs[0 .. num_list) of at most
 * `group` (8, 16, 32 or 64 <= dn_k3wl_max_nodes()) nodes, `group` lanes per fibre; fib_ptr [num_list + 1]: the first fibre of every
 * listed graph (3 n^2 each), num_fibres = fib_ptr[num_list].  Multiset 1 = C[x, w, u] for every x != v and the triple's own colour SIX
 * times, multiset 2 = C[v, x, u] for x != w, multiset 3 = C[v, w, x] for x != u.  WL: all local.  DWL: x is local where it is adjacent
 * to the exchanged node (bit x - first of adj_bits[that node], first = first node of the graph), else global; the own copies are
 * global.  work[(3 c + axis) num_items + t] receives the fold of class c (0 local, 1 global) of exchange axis + 1 of item t: 3
 * num_items values, 6 num_items for DWL.  dn_k3wl_close_u64 then writes colors_out for every item of a graph of at most
 * dn_k3wl_max_nodes() nodes from colors_in and work (which folds exist follows from the sizes and degrees). */
int32_t dn_k3wl_max_nodes(void);
int dn_k3wl_global_u64(int64_t num_graphs, int64_t num_items, int64_t num_list, const int32_t* graphs, const int32_t* fib_ptr,
                       int64_t num_fibres, int32_t group, int32_t malkin, const int32_t* node_ptr, const int32_t* tuple_ptr,
                       const int64_t* adj_bits, const int64_t* colors_in, int64_t* work, dn_stream_t stream);
int dn_k3wl_close_u64(int64_t num_nodes, int64_t num_items, int32_t malkin, const int32_t* tup_v, const int32_t* tup_w, const int32_t* tup_u,
                      const int32_t* node_graph, const int32_t* node_ptr, const int32_t* ptr, const int64_t* colors_in, const int64_t* work,
                      int64_t* colors_out, dn_stream_t stream);

/* ---- ragged sparsemax / softmax attention and DIAMNet's window pooling (dn_seg_attn.hip) ----------------------------------------
 * B pairs; pair b owns the query rows q_ptr[b] .. q_ptr[b + 1] of q [Nq, H] and the key rows k_ptr[b] .. k_ptr[b + 1] of k, v [Nk, H]
 * (fp32, already projected); head h owns the columns h dk .. (h + 1) dk, dk = H / heads.  heads in {1, 2, 4, 8}, H <= 256, dk a power
 * of two.  q_skip [Nq] / k_skip [Nk] (NULL: none): a key with a flag takes no weight, a query row with a flag (or of a pair without
 * a live key) yields a zero row.  max_q / max_k: the largest row counts of a pair (the caller's: the kernels clamp to them);
 * max_k <= dn_seg_attn_max_keys(), and the forward runs its one-wavefront-per-row form where max_k <= dn_seg_attn_wave_keys().
 *   fwd:    out [Nq, H] = sum_j p_j v_j per head, p = sparsemax or softmax of scale <q_i, k_j> over the live keys;
 *           stat [Nq, heads, 2] = {max, tau} (sparsemax: p_j = max(z_j - max - tau, 0)) or {max, sum exp(z - max)}.
 *   bwd_q:  dq [Nq, H] and rterm [Nq, heads] in fp64 (the mean of dP over the support, or sum p dP) from stat and dout [Nq, H].
 *   bwd_kv: dk, dv [Nk, H] from stat, rterm and dout; the query rows of a pair are walked in order.  No atomics anywhere. */
#define DN_SCORE_SPARSEMAX 0
#define DN_SCORE_SOFTMAX 1
int32_t dn_seg_attn_max_keys(void);
int32_t dn_seg_attn_wave_keys(void);
int dn_seg_attn_fwd_f32(int64_t B, int64_t Nq, int64_t Nk, int32_t H, int32_t heads, int32_t max_q, int32_t max_k, int32_t score,
                        const int32_t* q_ptr, const int32_t* k_ptr, const uint8_t* q_skip, const uint8_t* k_skip, const float* q,
                        const float* k, const float* v, float scale, float* out, float* stat, dn_stream_t stream);
int dn_seg_attn_bwd_q_f32(int64_t B, int64_t Nq, int64_t Nk, int32_t H, int32_t heads, int32_t max_q, int32_t max_k, int32_t score,
                          const int32_t* q_ptr, const int32_t* k_ptr, const uint8_t* q_skip, const uint8_t* k_skip, const float* q,
                          const float* k, const float* v, float scale, const float* stat, const float* dout, float* dq, double* rterm,
                          dn_stream_t stream);
int dn_seg_attn_bwd_kv_f32(int64_t B, int64_t Nq, int64_t Nk, int32_t H, int32_t heads, int32_t max_q, int32_t max_k, int32_t score,
                           const int32_t* q_ptr, const int32_t* k_ptr, const uint8_t* q_skip, const uint8_t* k_skip, const float* q,
                           const float* k, const float* v, float scale, const float* stat, const double* rterm, const float* dout,
                           float* dk, float* dv, dn_stream_t stream);
/* dn_seg_window_pool_*: per segment b of rows [N, D] (ptr [B + 1]) the span = the rows first .. last with skip == 0 (L of them; a
 * skipped row inside is a zero row) gives mem_len rows of mem [B mem_len, D]: L <= mem_len: the span's rows behind mem_len - L zero
 * rows; else window m = the kernel = L - (mem_len - 1) stride rows from m stride on, stride = L / mem_len, as their mean, sum or max.
 * mem_mask [B, mem_len] = the window holds a row with skip == 0; span [B, 2] = {first, L}; arg [B mem_len, D] (max only) = the row
 * that won, -1 where a zero row did.  bwd: drows [N, D], every row gathering from the windows that hold it. */
#define DN_POOL_MEAN 0
#define DN_POOL_SUM 1
#define DN_POOL_MAX 2
int dn_seg_window_pool_fwd_f32(int64_t B, int64_t N, int32_t D, int32_t mem_len, int32_t mode, const int32_t* ptr, const uint8_t* skip,
                               const float* rows, float* mem, uint8_t* mem_mask, int32_t* arg, int32_t* span, dn_stream_t stream);
int dn_seg_window_pool_bwd_f32(int64_t B, int64_t N, int32_t D, int32_t mem_len, int32_t mode, const int32_t* ptr, const uint8_t* skip,
                               const int32_t* span, const int32_t* arg, const float* dmem, float* drows, dn_stream_t stream);

/* ---- DiffPool on ragged rows (dn_diffpool.hip) -------------------------------------------------------------------------------
 * B graphs; graph g owns the rows graph_ptr[g] .. graph_ptr[g + 1] of every [N, .] operand (fp32).  No atomics: the same bits on
 * every run.  C <= dn_diffpool_max_clusters() (256) cluster columns, F <= dn_diffpool_max_features() (512) feature columns.
 *   dn_segment_gram_f32            out [B, CL, CR]: out[g] = L[rows_g]^T R[rows_g] (L [N, CL], CL <= 256; R [N, CR], CR <= 512) on the
 *                                  exact-f32 MFMA, the rows of a graph in order; a graph without rows yields zeros.  graphs (may be
 *                                  NULL, then num_list = 0): only the num_list graphs listed there are computed and written.
 *   dn_diffpool_softmax_fwd_f32    S [N, C] = softmax of the rows of logits [N, C].
 *   dn_diffpool_softmax_bwd_f32    dlogits = S (dS - rowsum(dS S)) with dS = d0 + d1 + d2 (d1, d2 may be NULL).
 *   dn_diffpool_assign_graphs_f32  for the num_list graphs listed in `graphs` (each of at most max_rows <= dn_diffpool_graph_rows(C)
 *                                  rows, so that S and A S fit in LDS), one workgroup per graph: S = softmax(logits) and
 *                                  AS[i] = sum of S[dst_by_src[e]] over out_ptr[i] <= e < out_ptr[i + 1] (the CSR by source of the E
 *                                  edges; an entry outside the graph's own rows is skipped) written to S, AS [N, C], and
 *                                  X[g] = S^T z ([C, F], z [N, F]), A[g] = S^T AS ([C, C]) written to X [B, C, F], A [B, C, C].
 *                                  Rows and graphs that are not listed are left untouched. */
int32_t dn_diffpool_max_clusters(void);
int32_t dn_diffpool_max_features(void);
int32_t dn_diffpool_graph_rows(int32_t C);
int dn_segment_gram_f32(int64_t B, int64_t N, int32_t CL, int32_t CR, const int32_t* graphs, int64_t num_list, const int32_t* graph_ptr,
                        const float* L, const float* R, float* out, dn_stream_t stream);
int dn_diffpool_softmax_fwd_f32(int64_t N, int32_t C, const float* logits, float* S, dn_stream_t stream);
int dn_diffpool_softmax_bwd_f32(int64_t N, int32_t C, const float* S, const float* d0, const float* d1, const float* d2, float* dlogits,
                                dn_stream_t stream);
int dn_diffpool_assign_graphs_f32(int64_t B, int64_t N, int64_t E, int64_t num_list, int32_t max_rows, int32_t C, int32_t F,
                                  const int32_t* graphs, const int32_t* graph_ptr, const int32_t* out_ptr, const int32_t* dst_by_src,
                                  const float* logits, const float* z, float* S, float* AS, float* X, float* A, dn_stream_t stream);

/* ---- HGP-SL pooling on ragged per-graph blocks (dn_hgpsl.hip) ----------------------------------------------------------------
 * B graphs; graph g owns the rows graph_ptr[g] .. graph_ptr[g + 1] of the batch and the kept rows pooled_ptr[g] .. pooled_ptr[g + 1]
 * (k_g of them, computed on the host) of the pooled batch of Np rows.  The per-pair storage is the ragged blocks: graph g's
 * k_g x k_g block, row-major, at blk_ptr[g] (int64) of a float array of T = sum k_g^2 entries.  Edges (row, col) with their CSR by
 * row (out_ptr, out_perm, dst_by_src) and by col (in_ptr, in_perm, src_by_dst); w [E] in edge order, NULL = ones.  fp32, no
 * atomics: the same bits on every run.  H <= dn_hgpsl_max_features() (512).
 *   dn_hgpsl_dinv_f32    dinv [N] = deg^-1/2 (0 where deg == 0), deg[v] = sum of w over the edges with row == v.
 *   dn_hgpsl_score_f32   score[i] = sum_f |x[i, f] - sum_{e: col = i} dinv[row_e] w_e dinv[i] x[row_e, f]|.
 *   dn_hgpsl_topk_f32    for the num_list graphs in `graphs` (each of at most max_nodes <= dn_hgpsl_topk_max_nodes() (4096) rows):
 *                        perm [Np] = the k_g rows of the highest scores, descending, ties to the lower row; pooled_batch [Np] = g;
 *                        inv [N] = the pooled row of a kept row, -1 of a dropped one.  Scores must be >= 0 and not NaN.
 *   dn_hgpsl_pq_f32      p[i] = <xp[i], att[:H]>, q[i] = <xp[i], att[H:]>  (xp [Np, H], att [2 H]).
 *   dn_hgpsl_structure_fwd_f32  for the num_rows pooled rows in `rows` (each of a graph with k_g <= max_keys <= dn_hgpsl_max_keys()
 *                        (1024); up to dn_hgpsl_wave_keys() (64): a wavefront per row, else a workgroup): the block row
 *                        softmax_j or sparsemax_j of leaky_relu(p_i + q_j, slope) + lamb A_ij, A_ij = the weight of the edge
 *                        (perm[i], perm[j]) or 0; score: DN_SCORE_SOFTMAX (max subtracted, 1e-16 added to the sum) or
 *                        DN_SCORE_SPARSEMAX.  Rows that are not listed are left untouched.
 *   dn_hgpsl_structure_bwd_rows_f32   dl [T] = the gradient of leaky_relu's argument, dp [Np] = its row sums, rterm [Np] = the row
 *                        term of the Jacobian (softmax: <o, g>; sparsemax: the mean of g over the support), for the listed rows.
 *   dn_hgpsl_structure_bwd_cols_f32   dq [Np] = the column sums of dl over the graph's rows in order, for the listed rows.
 *   dn_hgpsl_structure_bwd_edges_f32  dw [E] = lamb dz at the edge's pair; 0 for an edge with a dropped end or of a graph over
 *                        dn_hgpsl_max_keys().
 *   dn_hgpsl_att_grad_f32  datt [2 H] = [sum_i dp_i xp_i, sum_j dq_j xp_j]; ws: dn_hgpsl_att_slabs() x 2 H floats. */
int32_t dn_hgpsl_topk_max_nodes(void);
int32_t dn_hgpsl_wave_keys(void);
int32_t dn_hgpsl_max_keys(void);
int32_t dn_hgpsl_max_features(void);
int32_t dn_hgpsl_att_slabs(void);
int dn_hgpsl_dinv_f32(int64_t N, int64_t E, const int32_t* out_ptr, const int32_t* out_perm, const float* w, float* dinv,
                      dn_stream_t stream);
int dn_hgpsl_score_f32(int64_t N, int64_t E, int32_t H, const int32_t* in_ptr, const int32_t* in_perm, const int32_t* src_by_dst,
                       const float* w, const float* dinv, const float* x, float* score, dn_stream_t stream);
int dn_hgpsl_topk_f32(int64_t B, int64_t N, int64_t Np, int64_t num_list, int32_t max_nodes, const int32_t* graphs,
                      const int32_t* graph_ptr, const int32_t* pooled_ptr, const float* score, int32_t* perm, int32_t* pooled_batch,
                      int32_t* inv, dn_stream_t stream);
int dn_hgpsl_pq_f32(int64_t Np, int32_t H, const float* xp, const float* att, float* p, float* q, dn_stream_t stream);
int dn_hgpsl_structure_fwd_f32(int64_t B, int64_t N, int64_t E, int64_t Np, int64_t T, int64_t num_rows, int32_t max_keys, int32_t score,
                               const int32_t* rows, const int32_t* pooled_ptr, const int64_t* blk_ptr, const int32_t* pooled_batch,
                               const int32_t* perm, const int32_t* inv, const int32_t* out_ptr, const int32_t* out_perm,
                               const int32_t* dst_by_src, const float* w, const float* p, const float* q, float lamb, float slope,
                               float* blocks, dn_stream_t stream);
int dn_hgpsl_structure_bwd_rows_f32(int64_t B, int64_t Np, int64_t T, int64_t num_rows, int32_t score, const int32_t* rows,
                                    const int32_t* pooled_ptr, const int64_t* blk_ptr, const int32_t* pooled_batch, const float* p,
                                    const float* q, float slope, const float* blocks, const float* dblocks, float* dl, float* dp,
                                    float* rterm, dn_stream_t stream);
int dn_hgpsl_structure_bwd_cols_f32(int64_t B, int64_t Np, int64_t T, int64_t num_rows, const int32_t* rows, const int32_t* pooled_ptr,
                                    const int64_t* blk_ptr, const int32_t* pooled_batch, const float* dl, float* dq, dn_stream_t stream);
int dn_hgpsl_structure_bwd_edges_f32(int64_t B, int64_t N, int64_t E, int64_t Np, int64_t T, int32_t score, const int32_t* src,
                                     const int32_t* dst, const int32_t* inv, const int32_t* pooled_ptr, const int64_t* blk_ptr,
                                     const int32_t* pooled_batch, const float* blocks, const float* dblocks, const float* rterm, float lamb,
                                     float* dw, dn_stream_t stream);
int dn_hgpsl_att_grad_f32(int64_t Np, int32_t H, const float* xp, const float* dp, const float* dq, float* ws, float* datt,
                          dn_stream_t stream);

/* ---- The CNN count model's layer on edge sequences (csrc/dn_eseq.hip), rows layout x [B, L, C], fp32.
 *   C a multiple of 16 in 16 .. 128, 2 <= k <= 5, 0 <= padding <= k / 2, stride 1; L1 = L + 2 padding - k + 1 conv rows,
 *   L2 = L1 + 2 padding - k + 1 outputs (>= 1).  act: 0 none, 1 relu, 2 leaky_relu(slope).  Sequences are right-aligned: lo [B] is
 *   the first position of a sequence that may carry a non-zero gate_in; tiles left of a sequence's support are written as zeros
 *   without being computed.  Every entry point checks its arguments on the host before it launches anything.
 *   dn_eseq_conv_pool_fwd_f32   y [B, L2, C] = max-pool(act(conv(x * gate_in))) * gate_out (+ x * gate_in: residual, needs L2 == L),
 *                        gate_out [B, L2] = gate_in through the two max windows, arg [B, L2, C] = the winning window slot (bits
 *                        0-2, ties to the first) | 0x80 where the winning conv value is > 0 (undefined in the zero tiles).
 *                        wt [k][C][C] = weight[co][ci][j] stored as [j][ci][co].
 *   dn_eseq_dconv_f32    dconv [B, L1, C]: the gradient at the conv positions, gathered in slot order from dy, gate_out and arg.
 *   dn_eseq_dgrad_f32    dx [B, L, C] = (dconv * W (+ dy: residual)) * gate_in; wd [k][C][C] = weight[co][ci][k - 1 - j] stored as
 *                        [j][co][ci].
 *   dn_eseq_wgrad_f32    part [num_slices][k][C][C] ([j][ci][co]) and part_b [num_slices][C]: per slice of the batch's 32-row conv
 *                        tiles the sums of x0^T dconv and of dconv's columns.
 *   dn_eseq_wgrad_combine_f32   dW [C][C][k], db [C]: the partials added in slice order.
 *   dn_eseq_filter_gate_i64     out [B, Lg] (0 / 1) = g_ul in p_ul's row and g_el in p_el's and g_vl in p_vl's (the padded zeros of
 *                        the pattern rows count); labels in [0, dn_eseq_filter_max_labels()), others never match. */
int32_t dn_eseq_filter_max_labels(void);
int dn_eseq_conv_pool_fwd_f32(int64_t B, int32_t L, int32_t C, int32_t k, int32_t padding, int32_t act, float slope, int32_t residual,
                              const float* x, const float* gate_in, const float* wt, const float* bias, const int32_t* lo, float* y,
                              float* gate_out, uint8_t* arg, dn_stream_t stream);
int dn_eseq_dconv_f32(int64_t B, int32_t L, int32_t C, int32_t k, int32_t padding, int32_t act, float slope, const float* dy,
                      const float* gate_out, const uint8_t* arg, float* dconv, dn_stream_t stream);
int dn_eseq_dgrad_f32(int64_t B, int32_t L, int32_t C, int32_t k, int32_t padding, int32_t residual, const float* dconv, const float* dy,
                      const float* gate_in, const float* wd, const int32_t* lo, float* dx, dn_stream_t stream);
int dn_eseq_wgrad_f32(int64_t B, int32_t L, int32_t C, int32_t k, int32_t padding, const float* x, const float* gate_in,
                      const float* dconv, const int32_t* lo, int32_t num_slices, float* part, float* part_b, dn_stream_t stream);
int dn_eseq_wgrad_combine_f32(int32_t C, int32_t k, int32_t num_slices, const float* part, const float* part_b, float* dW, float* db,
                              dn_stream_t stream);
int dn_eseq_filter_gate_i64(int64_t B, int32_t Lp, int32_t Lg, const int64_t* p_ul, const int64_t* p_el, const int64_t* p_vl,
                            const int64_t* g_ul, const int64_t* g_el, const int64_t* g_vl, uint8_t* out, dn_stream_t stream);

/* ---- The RNN count model's recurrence on edge sequences (csrc/dn_eseq_rnn.hip), rows layout, fp32.
 *   cell: 0 LSTM (gates i f g o), 1 GRU (r z n), 2 tanh; G = 4 / 3 / 1 gates; Hd (hidden width per direction) in {16, 32, 48, 64};
 *   D = 1 or 2 directions (direction 1 walks the time axis backwards); 1 <= B <= 65535, L >= 1, B L D 5 Hd < 2^31.
 *   P [B, L, D G Hd]: the input side x0 W_ih^T + b, every bias folded in except the GRU's b_hn [D, Hd]; whh [D, G Hd, Hd]; gate [B, L]
 *   (0 / 1); lo [B]: the first position of a sequence that may carry a non-zero gate (only direction 1 uses it: it stops at the
 *   smallest lo of its 16 sequences and writes zeros to the left).  One workgroup per 16 sequences and direction walks all steps.
 *   dn_eseq_rnn_fwd_f32   y [B, L, D Hd] = h gate (+ x0 [B, L, D Hd] when residual), h [B, L, D Hd] the ungated state, saved
 *                         [B, L, D, S Hd] with S = dn_eseq_rnn_saved_per_unit(cell): LSTM i f g o c, GRU r z n (W_hn h + b_hn), tanh none.
 *   dn_eseq_rnn_bwd_f32   dP [B, L, D G Hd]: the gradient at the input-side pre-activations; dhn [B, L, D Hd] (GRU only): the gradient
 *                         at W_hn h + b_hn.  dy [B, L, D Hd] is the gradient at y (the gate is applied inside). */
int32_t dn_eseq_rnn_saved_per_unit(int32_t cell);
int dn_eseq_rnn_fwd_f32(int64_t B, int32_t L, int32_t Hd, int32_t D, int32_t cell, int32_t residual, const float* P, const float* whh,
                        const float* bhn, const float* x0, const float* gate, const int32_t* lo, float* y, float* h, float* saved,
                        dn_stream_t stream);
int dn_eseq_rnn_bwd_f32(int64_t B, int32_t L, int32_t Hd, int32_t D, int32_t cell, const float* dy, const float* gate, const int32_t* lo,
                        const float* whh, const float* h, const float* saved, float* dP, float* dhn, dn_stream_t stream);

/* ---- The TransformerXL count model's attention (csrc/dn_txl.hip): relative-position attention over a sliding memory as a banded
 *   attention over the whole padded sequence, rows layout, fp32.
 *   q, k, v, k_mem, v_mem, out, dout [B, Lp, n, D]; rk [P, n, D] indexed by relative position; r_w_bias, r_r_bias [n, D]; stats
 *   [B, Lp, n, 2] (row max, log of the sum).  D in {16, 32, 64}; seg in {16, 32, 48, 64}; mem a multiple of 16 with seg + mem <= 128;
 *   Lp a multiple of seg; P >= seg + mem; B Lp n D and B (Lp / seg) n P D below 2^31.  The queries of segment s attend the rows
 *   [s seg - mlen, (s + 1) seg), mlen = min(mem, s seg): the first mlen of them are read from k_mem / v_mem, the others from k / v
 *   (mem == 0: k_mem / v_mem may be NULL).  score = scale ((q + r_w_bias) K^T + rel_shift((q + r_r_bias) rk^T)) with the reference's
 *   pad-and-view shift; softmax over the whole window.
 *   dn_txl_attn_fwd_f32   out and stats, ONE launch.
 *   dn_txl_attn_bwd_f32   dq_ac / dq_bd [B, Lp, n, D]: the gradient at q through the AC and through the BD term (their sums over
 *                         (b, row) are the gradients at r_w_bias / r_r_bias); dk, dv: the gradient at the own rows; k_part, v_part
 *                         [B, S, n, mem, D]: at each window's memory rows; rk_part [B, S, n, P, D]: at rk's rows 0 .. klen - 1.
 *   dn_txl_fold_mem_f32   dk_mem, dv_mem [B, Lp, n, D] = k_part / v_part summed per row in segment order.
 *   dn_txl_reduce_rk_f32  drk [P, n, D] = rk_part summed over (sequence, segment) in a fixed order.  No atomics anywhere. */
int dn_txl_attn_fwd_f32(int64_t B, int32_t Lp, int32_t n, int32_t D, int32_t seg, int32_t mem, int32_t P, float scale, const float* q,
                        const float* k, const float* v, const float* k_mem, const float* v_mem, const float* rk, const float* r_w_bias,
                        const float* r_r_bias, float* out, float* stats, dn_stream_t stream);
int dn_txl_attn_bwd_f32(int64_t B, int32_t Lp, int32_t n, int32_t D, int32_t seg, int32_t mem, int32_t P, float scale, const float* dout,
                        const float* q, const float* k, const float* v, const float* k_mem, const float* v_mem, const float* rk,
                        const float* r_w_bias, const float* r_r_bias, const float* out, const float* stats, float* dq_ac, float* dq_bd,
                        float* dk, float* dv, float* k_part, float* v_part, float* rk_part, dn_stream_t stream);
int dn_txl_fold_mem_f32(int64_t B, int32_t Lp, int32_t n, int32_t D, int32_t seg, int32_t mem, const float* k_part, const float* v_part,
                        float* dk_mem, float* dv_mem, dn_stream_t stream);
int dn_txl_reduce_rk_f32(int64_t B, int32_t Lp, int32_t n, int32_t D, int32_t seg, int32_t mem, int32_t P, const float* rk_part, float* drk,
                         dn_stream_t stream);

/* ---- kernel-SVM evaluation of gram matrices: batched SMO for the C-SVC dual on precomputed kernels (dn_svm.hip) ----
 * The counterpart of scikit-learn's SVC(kernel="precomputed") inside graph_classification/graph_kernels/seed_svm.py, in fp64:
 * minimise 1/2 a^T Q a - sum(a), 0 <= a <= C, y^T a = 0, Q_tu = y_t y_u K_tu, with libsvm's second-order working-set selection
 * (ties to the lowest index, TAU = 1e-12), its update and clipping, its stopping rule m - M < eps and its rho; no shrinking.
 *   K      [num_matrices, n, n] doubles; the kernel rows of a solve are gathered out of it, nothing is copied per solve.
 *   table  [num_solves, 5] doubles {matrix, offset, length, positives, C}: the solve's training rows are rows[offset .. offset +
 *          length) (row indices into its matrix), the first `positives` of them the +1 class.
 *   list   the solves of this launch (NULL: all of them, num_list == num_solves); one workgroup each.
 *   alpha, grad [num_rows] doubles at the offsets of `rows`: the state, read at the start of a launch and stored at its end (a
 *          fresh solve starts from alpha = 0, grad = -1, iterations = 0); rho [num_solves]; iterations [num_solves] (int64).
 *   status [num_solves]: 0 converged, 1 still running after iters_per_launch more iterations, 2 libsvm's cap max(10^7, 100 length)
 *          reached, 3 the table row or a row index is out of range (nothing is computed for that solve).
 * max_len = the longest row list of the table (the launch's LDS: 28 bytes a row), at most dn_svm_max_rows(); a longer list in the
 * table gets status 3.  No atomics, fixed reduction order: the result does not depend on iters_per_launch, two runs give the same bits. */
int32_t dn_svm_max_rows(void);
int dn_svm_smo_f64(int64_t num_matrices, int64_t n, const double* K, int64_t num_solves, const double* table, int64_t num_list,
                   const int32_t* list, int64_t num_rows, const int32_t* rows, int32_t max_len, double eps, int32_t iters_per_launch,
                   double* alpha, double* grad, double* rho, int64_t* iterations, int32_t* status, dn_stream_t stream);

/* ---- the SI training objective and the epoch's per-sample errors (dn_objective.hip) ----
 * The objective of subgraph_isomorphism/train.py:776-821 and the per-sample errors of evaluate_epoch (train.py:1101-1173).  With
 * crit(d) = |d| (MAE), d^2 (MSE) or smooth-L1 at beta 1 (SMSE), s = neg_slp, m the mask and B the pairs:
 *   eval = 1/B sum_b crit_eval(relu(pred_c_b) - c_b)          bp = 1/B sum_b crit(lrelu(pred_c_b, s) - c_b)
 *   x_loss = 1/B sum_bj crit(lrelu(m p_bj, s) - m w_bj)       x_reg = 1/B sum_bj crit(relu(m p_bj - pred_c_b))     (x = v, e)
 *   rep_reg = sum_r (sum crit(rep_r)) / rep_denom[r]          (rep_denom = numel / size(1))
 *   loss = bp + rep_reg_w rep_reg + match_loss_w (v_loss + e_loss) + match_reg_w (v_reg + e_reg)
 * x_reg runs over ALL positions (a masked one enters as 0) and its gradient reaches pred_x there too.
 *   pred_c, counts [B]; pred_x, x_mask (bytes, non-zero = kept), x_target [B, L_x], a side is absent when all three are NULL and
 *   L_x == 0; reps / rep_numel / rep_denom / rep_dt: HOST arrays of num_reps <= DN_OBJECTIVE_MAX_REPS entries.  Every tensor is
 *   contiguous and fp32 or bf16, by its own *_dt code; gradients come back in the dtype of their input.
 *   dn_objective_fwd   terms [7] doubles = {eval, loss, v_loss, e_loss, v_reg, e_reg, rep_reg} (the order train.py:815-821 reads
 *                      them), loss a float; workspace of dn_objective_workspace_bytes bytes (the workgroups' partial sums, added
 *                      in index order by a closing launch).  fp64 accumulation, no atomics, the grid depends on the shapes only:
 *                      two runs give the same bits.
 *   dn_objective_bwd   ONE launch: grad_loss (device, a float) times the gradient of loss at pred_c, pred_v, pred_e and every
 *                      representation; an output that is NULL is not computed.
 *   dn_objective_eval  per pair, at [offset, offset + B) of buffers of `capacity` entries: ae = |relu(pred_c) - c|, se = ae^2,
 *                      ned / eed = sum_j |relu(p_bj) - w_bj| over all positions (no mask; 0 for an absent side),
 *                      cls = (c > 0) + 2 (relu(pred_c) > 0).
 * Arguments are checked on the host before any launch (-1 and a message); nothing reads device memory back. */
#define DN_OBJECTIVE_MAE 0
#define DN_OBJECTIVE_MSE 1
#define DN_OBJECTIVE_SMSE 2
#define DN_OBJECTIVE_F32 0
#define DN_OBJECTIVE_BF16 1
#define DN_OBJECTIVE_MAX_REPS 4
size_t dn_objective_workspace_bytes(int64_t B, int32_t num_reps, const int64_t* rep_numel);
int dn_objective_fwd(int64_t B, const void* pred_c, int32_t pred_c_dt, const void* counts, int32_t counts_dt, int64_t Lv, const void* pred_v,
                     int32_t pred_v_dt, const uint8_t* v_mask, const void* v_target, int32_t v_target_dt, int64_t Le, const void* pred_e,
                     int32_t pred_e_dt, const uint8_t* e_mask, const void* e_target, int32_t e_target_dt, int32_t num_reps,
                     const void* const* reps, const int64_t* rep_numel, const int64_t* rep_denom, const int32_t* rep_dt, int32_t bp_crit,
                     int32_t eval_crit, double neg_slp, double rep_reg_w, double match_loss_w, double match_reg_w, double* terms,
                     float* loss, void* workspace, size_t workspace_bytes, dn_stream_t stream);
int dn_objective_bwd(int64_t B, const float* grad_loss, const void* pred_c, int32_t pred_c_dt, const void* counts, int32_t counts_dt,
                     int64_t Lv, const void* pred_v, int32_t pred_v_dt, const uint8_t* v_mask, const void* v_target, int32_t v_target_dt,
                     int64_t Le, const void* pred_e, int32_t pred_e_dt, const uint8_t* e_mask, const void* e_target, int32_t e_target_dt,
                     int32_t num_reps, const void* const* reps, const int64_t* rep_numel, const int64_t* rep_denom, const int32_t* rep_dt,
                     int32_t bp_crit, double neg_slp, double rep_reg_w, double match_loss_w, double match_reg_w, void* d_pred_c,
                     void* d_pred_v, void* d_pred_e, void* const* d_reps, dn_stream_t stream);
int dn_objective_eval(int64_t B, const void* pred_c, int32_t pred_c_dt, const void* counts, int32_t counts_dt, int64_t Lv, const void* pred_v,
                      int32_t pred_v_dt, const void* v_target, int32_t v_target_dt, int64_t Le, const void* pred_e, int32_t pred_e_dt,
                      const void* e_target, int32_t e_target_dt, int64_t offset, int64_t capacity, float* ae, float* se, float* ned,
                      float* eed, int32_t* cls, dn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DN_HIP_H */
