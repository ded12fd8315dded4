// LRP (local relational pooling) of the SI count models: the ego-net permutation index and the fused pooling kernels.
//
// Reference: subgraph_isomorphism/dataset.py:1750-1886 (LRPDataset: the sequences of every node and the two COO matrices that
// scatter node / edge rows into [P L^2, in]) and models/lrp.py:65-75 (two sparse products, an einsum with weight [in, hid, L^2],
// a third sparse product that pools the P sequences per node).  Here the einsum is row-factorised (T_node = x @ diagonal slots,
// T_edge = edge_feat @ off-diagonal slots, both on the Linear kernels) and one workgroup per node enumerates the node's sequences
// itself: per sequence it sums <= L + L (L - 1) table rows, adds the bias, activates and accumulates.  Nothing of size P is stored.
// DMPLRP (models/dmplrp.py:180-185) pools the same contraction with no activation and no factor in between; its collapsed index
// (the distinct table rows of every ego with their occurrence counts over the sequences of dataset.py:1843-1886) is built below.
//
// Ego index (built once per batch): uptr / unbr / ueid = the duplicate-free, sorted out-neighbour lists over
// the edges that count (is_reversed == 0) with the LAST edge id of every (u, w); per node {kind, dummy neighbours}, the sequence
// count (int64) and upos = the positions of the non-dummy neighbours followed by those of the dummy neighbours.
//   kind 0: (v,) + every m-permutation of adj(v), m = min(L - 1, d), lexicographic in positions (itertools.permutations)
//   kind 1: v is a dummy node: (v,) + every m-combination of adj(v) (itertools.combinations)
//   kind 2: v has dummy neighbours: for every dummy neighbour z in adj order, (v,) + q + (z,), q over the min(L - 2, n')-
//           permutations of the n' non-dummy neighbours
#include "dn_common.h"
#include "dn_hip.h"

#include <limits.h>

namespace {

constexpr int kThreads = 256;
constexpr int kStageBytes = 56 * 1024;   // T_node rows of one ego kept in LDS (the backward keeps as many gradient rows next to them)
constexpr int kPairMax = 64;             // egos of up to this many nodes keep their (a, b) -> edge id table in LDS

struct LrpIndex {
    const int32_t *uptr, *unbr, *ueid, *upos, *ego;
    const int64_t* count;
};

__device__ __forceinline__ int64_t sat_mul(int64_t a, int64_t b, bool& over) {
    if (a > 0 && b > LLONG_MAX / a) {
        over = true;
        return LLONG_MAX;
    }
    return a * b;
}

// sequences of an ego: kind 0 / 1 over d neighbours, kind 2 over nd dummy and d - nd other neighbours
__device__ __forceinline__ int64_t lrp_count(int kind, int L, int64_t d, int64_t nd, bool& over) {
    if (kind == 2) {
        const int64_t nn = d - nd;
        const int mm = (int)(L - 2 < nn ? L - 2 : nn);
        int64_t r = nd;
        for (int i = 0; i < mm; ++i) r = sat_mul(r, nn - i, over);
        return r;
    }
    const int m = (int)(L - 1 < d ? L - 1 : d);
    if (kind == 0) {
        int64_t r = 1;
        for (int i = 0; i < m; ++i) r = sat_mul(r, d - i, over);
        return r;
    }
    if (m == 0) return 1;
    if (m == 1) return d;
    const int64_t c2 = d * (d - 1) / 2;          // d < 2^31
    if (m == 2) return c2;
    return c2 % 3 == 0 ? sat_mul(c2 / 3, d - 2, over) : sat_mul(c2, (d - 2) / 3, over);   // 3 | c2 (d - 2)
}

// the q-th m-permutation of {0 .. n-1} in lexicographic order (m <= 3)
template <typename T>
__device__ __forceinline__ void lrp_unrank_perm(int n, int m, T q, int (&idx)[3]) {
    if (m == 1) {
        idx[0] = (int)q;
    } else if (m == 2) {
        const T i0 = q / (T)(n - 1), r = q % (T)(n - 1);
        idx[0] = (int)i0;
        idx[1] = (int)(r + (r >= i0 ? 1 : 0));
    } else if (m == 3) {
        const T f = (T)(n - 1) * (T)(n - 2);
        const T i0 = q / f, r = q % f;
        const T a = r / (T)(n - 2), b = r % (T)(n - 2);
        const int j0 = (int)i0, j1 = (int)(a + (a >= i0 ? 1 : 0));
        const int lo = j0 < j1 ? j0 : j1, hi = j0 < j1 ? j1 : j0;
        int j2 = (int)b;
        if (j2 >= lo) ++j2;
        if (j2 >= hi) ++j2;
        idx[0] = j0; idx[1] = j1; idx[2] = j2;
    }
}

// Sequence q of an ego as local positions (0 = the node itself, i + 1 = its i-th sorted neighbour); returns the length.
template <int L>
__device__ __forceinline__ int lrp_decode(int kind, int d, int nd, int64_t q, const int32_t* __restrict__ upos_v, int (&lp)[L]) {
    lp[0] = 0;
    int idx[3] = {0, 0, 0};
    if (kind == 0) {
        const int m = L - 1 < d ? L - 1 : d;
        if (q <= 0x7fffffffLL && d <= 1024) lrp_unrank_perm<uint32_t>(d, m, (uint32_t)q, idx);
        else lrp_unrank_perm<int64_t>(d, m, q, idx);
#pragma unroll
        for (int k = 0; k < L - 1; ++k)
            if (k < m) lp[k + 1] = idx[k] + 1;
        return m + 1;
    }
    if (kind == 1) {
        const int m = L - 1 < d ? L - 1 : d;
        int c = 0;
#pragma unroll
        for (int pos = 0; pos < L - 1; ++pos) {
            if (pos >= m) break;
            const int rem = m - pos - 1;
            if (rem == 0) {
                c += (int)q;
                q = 0;
            } else {
                for (;;) {                                   // combinations whose next element is c: C(d - c - 1, rem)
                    const int64_t n = d - c - 1;
                    const int64_t w = rem == 1 ? n : n * (n - 1) / 2;
                    if (q < w) break;
                    q -= w;
                    ++c;
                }
            }
            lp[pos + 1] = c + 1;
            ++c;
        }
        return m + 1;
    }
    const int nn = d - nd;
    const int mm = L - 2 < nn ? L - 2 : nn;
    int64_t per = 1;
    for (int i = 0; i < mm; ++i) per *= nn - i;
    const int64_t j = q / per, r = q % per;
    lrp_unrank_perm<int64_t>(nn, mm, r, idx);
#pragma unroll
    for (int k = 0; k < L - 2; ++k)
        if (k < mm) lp[k + 1] = upos_v[idx[k]] + 1;
    lp[mm + 1] = upos_v[nn + (int)j] + 1;
    return mm + 2;
}

// The combination after lp[1 .. m] (positions 1 .. d, ascending) in lexicographic order; there is one (the caller stops at the count).
template <int L>
__device__ __forceinline__ void lrp_next_comb(int m, int d, int (&lp)[L]) {
    bool done = false;
#pragma unroll
    for (int i = L - 1; i >= 1; --i) {
        if (done || i > m || lp[i] >= d - (m - i)) continue;
        ++lp[i];
#pragma unroll
        for (int j = i + 1; j < L; ++j)
            if (j <= m) lp[j] = lp[j - 1] + 1;
        done = true;
    }
}

// eid(u, w): the last counted edge u -> w, -1 when there is none (binary search in u's sorted neighbour list)
__device__ __forceinline__ int32_t lrp_lookup(const LrpIndex& ix, int32_t u, int32_t w) {
    int32_t lo = ix.uptr[u], hi = ix.uptr[u + 1];
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (ix.unbr[mid] < w) lo = mid + 1;
        else hi = mid;
    }
    return (lo < ix.uptr[u + 1] && ix.unbr[lo] == w) ? ix.ueid[lo] : -1;
}

// compact index of the off-diagonal slot (a, b) of the L x L block, in slot order
template <int L>
__device__ __forceinline__ int lrp_off_slot(int a, int b) {
    return a * (L - 1) + (b > a ? b - 1 : b);
}

// ---------------------------------------------------------------------------------------------- index kernels
__global__ __launch_bounds__(kThreads) void lrp_ego_index_kernel(int64_t N, int32_t L, const int32_t* __restrict__ uptr,
                                                                  const int32_t* __restrict__ unbr, const uint8_t* __restrict__ dummy,
                                                                  int32_t* __restrict__ upos, int32_t* __restrict__ ego,
                                                                  int64_t* __restrict__ count, int32_t* __restrict__ err) {
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (v >= N) return;
    const int32_t base = uptr[v], d = uptr[v + 1] - base;
    int32_t nd = 0;
    bool loop = false;
    for (int32_t i = 0; i < d; ++i) {
        const int32_t w = unbr[base + i];
        loop = loop || w == (int32_t)v;
        if (dummy != nullptr && dummy[w]) ++nd;
    }
    if (loop) atomicMin(&err[0], (int32_t)v);
    const bool self_dummy = dummy != nullptr && dummy[v];
    const int kind = self_dummy ? 1 : (nd > 0 ? 2 : 0);
    int32_t a = 0, b = d - nd;
    for (int32_t i = 0; i < d; ++i) {
        const bool z = dummy != nullptr && dummy[unbr[base + i]];
        upos[base + (z ? b++ : a++)] = i;
    }
    bool over = false;
    count[v] = lrp_count(kind, L, d, nd, over);
    ego[2 * v] = kind;
    ego[2 * v + 1] = nd;
    if (over) atomicOr(&err[1], 1);
}

template <int L>
__global__ __launch_bounds__(kThreads) void lrp_perm_fill_kernel(int64_t N, int64_t P, LrpIndex ix, const int32_t* __restrict__ perm_ptr,
                                                                  int32_t* __restrict__ perm_nodes, int32_t* __restrict__ perm_edges) {
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= P) return;
    int64_t lo = 0, hi = N - 1;                                    // the node of sequence p: the last v with perm_ptr[v] <= p
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (perm_ptr[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    const int32_t v = (int32_t)lo, base = ix.uptr[v], d = ix.uptr[v + 1] - base;
    int lp[L];
    const int len = lrp_decode<L>(ix.ego[2 * v], d, ix.ego[2 * v + 1], p - perm_ptr[v], ix.upos + base, lp);
    int32_t node[L];
#pragma unroll
    for (int k = 0; k < L; ++k) {
        node[k] = k < len ? (lp[k] == 0 ? v : ix.unbr[base + lp[k] - 1]) : -1;
        perm_nodes[p * L + k] = node[k];
    }
#pragma unroll
    for (int a = 0; a < L; ++a)
#pragma unroll
        for (int b = 0; b < L; ++b)
            perm_edges[p * L * L + a * L + b] = (a != b && a < len && b < len) ? lrp_lookup(ix, node[a], node[b]) : -1;
}

// ---------------------------------------------------------------------------------------------- pooling kernels
struct LrpPoolArgs {
    LrpIndex ix;
    int32_t H;
    const float *t_node, *t_edge, *bias, *factor;
    int32_t pool_mean, act_on;
    float slope;
    float *pooled, *out;                               // forward outputs (pooled: the value in front of the factor, or NULL)
    const float* g;                                    // backward: d out [N, H]
    float *d_tnode, *d_tedge, *d_bias, *d_factor;      //   accumulated with fp32 atomics into zeroed tables (d_factor: stored)
};

// One workgroup per node, thread = (sequence group g, column h): G = 256 / H groups, each walks a contiguous share of the node's
// sequences (a dummy node's combinations by their successor rule: unranking one costs a walk over its neighbours).
template <int L, bool BWD>
__global__ __launch_bounds__(kThreads) void lrp_pool_kernel(LrpPoolArgs a) {
    __shared__ float s_rows[kStageBytes / 4];
    __shared__ float s_grad[BWD ? kStageBytes / 4 : 1];
    __shared__ int32_t s_pair[kPairMax * kPairMax];
    __shared__ float s_red[kThreads];
    const LrpIndex& ix = a.ix;
    const int32_t v = blockIdx.x, H = a.H, tid = threadIdx.x;
    const int32_t base = ix.uptr[v], d = ix.uptr[v + 1] - base;
    const int kind = ix.ego[2 * v], nd = ix.ego[2 * v + 1];
    const int64_t cnt = ix.count[v];
    const int G = kThreads / H, g = tid / H, h = tid - g * H;
    const bool active = g < G;
    const int LH = L * H;
    const bool staged = (int64_t)(d + 1) * LH * 4 <= kStageBytes, paired = d + 1 <= kPairMax;
    if (staged) {
        for (int i = tid; i < (d + 1) * LH; i += kThreads) {
            const int n = i / LH;
            const int32_t node = n == 0 ? v : ix.unbr[base + n - 1];
            s_rows[i] = a.t_node[(size_t)node * LH + (i - n * LH)];
            if (BWD) s_grad[i] = 0.f;
        }
    }
    if (paired) {
        for (int i = tid; i < (d + 1) * (d + 1); i += kThreads) {
            const int la = i / (d + 1), lb = i - la * (d + 1);
            const int32_t na = la == 0 ? v : ix.unbr[base + la - 1], nb = lb == 0 ? v : ix.unbr[base + lb - 1];
            s_pair[la * kPairMax + lb] = la == lb ? -1 : lrp_lookup(ix, na, nb);
        }
    }
    __syncthreads();

    const float bias = (a.bias != nullptr && active) ? a.bias[h] : 0.f;
    float gp = 0.f;                                                // backward: d (sum of the activated sequences)
    if (BWD && active) {
        gp = a.g[(size_t)v * H + h];
        if (a.factor != nullptr) {
            const float pl = a.pooled[(size_t)v * H + h], f = a.factor[(size_t)v * H + h];
            if (a.act_on && !(pl * f > 0.f)) gp *= a.slope;
            if (g == 0) a.d_factor[(size_t)v * H + h] = gp * pl;
            gp *= f;
        }
        if (a.pool_mean) gp /= (float)cnt;
    }
    float acc = 0.f;
    if (active) {
        const int64_t share = (cnt + G - 1) / G, q0 = g * share, q1 = q0 + share < cnt ? q0 + share : cnt;
        int lp[L];
        int len = 0;
        for (int64_t q = q0; q < q1; ++q) {
            if (kind == 1 && q > q0) lrp_next_comb<L>(len - 1, d, lp);
            else len = lrp_decode<L>(kind, d, nd, q, ix.upos + base, lp);
            int32_t node[L], eid[L * (L - 1)];
            float z = bias;
#pragma unroll
            for (int k = 0; k < L; ++k) {
                if (k >= len) continue;
                if (staged) {
                    z += s_rows[(lp[k] * L + k) * H + h];
                } else {
                    node[k] = lp[k] == 0 ? v : ix.unbr[base + lp[k] - 1];
                    z += a.t_node[((size_t)node[k] * L + k) * H + h];
                }
            }
#pragma unroll
            for (int s = 0; s < L * (L - 1); ++s) eid[s] = -1;
#pragma unroll
            for (int p = 0; p < L; ++p) {
#pragma unroll
                for (int r = 0; r < L; ++r) {
                    if (p == r || p >= len || r >= len) continue;
                    int32_t e;
                    if (paired) {
                        e = s_pair[lp[p] * kPairMax + lp[r]];
                    } else {
                        const int32_t np = lp[p] == 0 ? v : ix.unbr[base + lp[p] - 1], nr = lp[r] == 0 ? v : ix.unbr[base + lp[r] - 1];
                        e = lrp_lookup(ix, np, nr);
                    }
                    const int s = lrp_off_slot<L>(p, r);
                    eid[s] = e;
                    if (e >= 0) z += a.t_edge[((size_t)e * (L * (L - 1)) + s) * H + h];
                }
            }
            if (!BWD) {
                acc += a.act_on ? dn_act(z, a.slope) : z;
            } else {
                const float dz = (a.act_on && !(z > 0.f)) ? gp * a.slope : gp;
                acc += dz;
#pragma unroll
                for (int k = 0; k < L; ++k) {
                    if (k >= len) continue;
                    if (staged) atomicAdd(&s_grad[(lp[k] * L + k) * H + h], dz);
                    else atomicAdd(&a.d_tnode[((size_t)node[k] * L + k) * H + h], dz);
                }
#pragma unroll
                for (int s = 0; s < L * (L - 1); ++s)
                    if (eid[s] >= 0) atomicAdd(&a.d_tedge[((size_t)eid[s] * (L * (L - 1)) + s) * H + h], dz);
            }
        }
    }
    s_red[tid] = acc;
    __syncthreads();
    if (g == 0 && active) {
        float sum = 0.f;
        for (int j = 0; j < G; ++j) sum += s_red[j * H + h];
        if (!BWD) {
            if (a.pool_mean) sum /= (float)cnt;
            if (a.pooled != nullptr) a.pooled[(size_t)v * H + h] = sum;
            if (a.factor != nullptr) {
                sum *= a.factor[(size_t)v * H + h];
                if (a.act_on) sum = dn_act(sum, a.slope);
            }
            a.out[(size_t)v * H + h] = sum;
        } else if (a.d_bias != nullptr && sum != 0.f) {
            atomicAdd(&a.d_bias[h], sum);
        }
    }
    if (BWD && staged) {
        for (int i = tid; i < (d + 1) * LH; i += kThreads) {
            const float val = s_grad[i];
            if (val == 0.f) continue;
            const int n = i / LH;
            const int32_t node = n == 0 ? v : ix.unbr[base + n - 1];
            atomicAdd(&a.d_tnode[(size_t)node * LH + (i - n * LH)], val);
        }
    }
}

// ---------------------------------------------------------------------------------------------- collapsed index (DMPLRP)
// models/dmplrp.py:180-185 pools the contracted sequences of a node with nothing non-linear in between, so the pooled row is a
// weighted sum of table rows: out[v] = sum_rows (occurrences of the row in v's sequences) T[row].  The occurrence counts have
// closed forms in the ego's kind, its d neighbours (nd of them dummies) and the sorted positions of the nodes involved; nothing is
// enumerated and nothing is sized by the sequence count.  Rows are numbered as the composed path numbers them: node u at position
// k -> u L + k, edge eid in slot (a, b) -> N L + eid L (L - 1) + lrp_off_slot(a, b).
struct LrpForm {
    int kind, m;                 // positions 1 .. m hold (kind 2: non-dummy) neighbours; kind 2 puts a dummy neighbour at m + 1
    int64_t d, nd, nn, total;
};

__device__ __forceinline__ int64_t cl_perm(int64_t n, int k) {       // n (n - 1) .. (n - k + 1), 0 when there is none
    if (k < 0 || n < k) return 0;
    int64_t r = 1;
    for (int i = 0; i < k; ++i) r *= n - i;
    return r;
}

__device__ __forceinline__ int64_t cl_comb(int64_t n, int k) {       // C(n, k), k <= 3
    if (k < 0 || n < k) return 0;
    if (k == 0) return 1;
    if (k == 1) return n;
    const int64_t c2 = n * (n - 1) / 2;
    if (k == 2) return c2;
    return c2 % 3 == 0 ? c2 / 3 * (n - 2) : c2 * ((n - 2) / 3);
}

__device__ __forceinline__ LrpForm lrp_form(int kind, int L, int64_t d, int64_t nd, int64_t total) {
    LrpForm f;
    f.kind = kind; f.d = d; f.nd = nd; f.nn = d - nd; f.total = total;
    const int64_t room = kind == 2 ? L - 2 : L - 1, have = kind == 2 ? f.nn : d;
    f.m = (int)(room < have ? room : have);
    return f;
}

// sequences of the ego that hold its neighbour of sorted position t (t < 0: the ego's own node; z: the neighbour is a dummy) at k
__device__ __forceinline__ int64_t lrp_form_node(const LrpForm& f, int64_t t, bool z, int k) {
    if (t < 0) return k == 0 ? f.total : 0;
    if (k < 1) return 0;
    if (f.kind == 0) return k <= f.m ? cl_perm(f.d - 1, f.m - 1) : 0;
    if (f.kind == 1) return k <= f.m ? cl_comb(t, k - 1) * cl_comb(f.d - 1 - t, f.m - k) : 0;
    if (z) return k == f.m + 1 ? cl_perm(f.nn, f.m) : 0;
    return k <= f.m ? f.nd * cl_perm(f.nn - 1, f.m - 1) : 0;
}

// sequences that hold neighbour ta at position a AND neighbour tb at position b (a != b, ta != tb)
__device__ __forceinline__ int64_t lrp_form_joint(const LrpForm& f, int64_t ta, bool za, int a, int64_t tb, bool zb, int b) {
    if (ta < 0) return a == 0 ? lrp_form_node(f, tb, zb, b) : 0;
    if (tb < 0) return b == 0 ? lrp_form_node(f, ta, za, a) : 0;
    if (a < 1 || b < 1) return 0;
    const int m = f.m;
    if (f.kind == 0) return (a <= m && b <= m) ? cl_perm(f.d - 2, m - 2) : 0;
    if (f.kind == 1) {
        if (ta > tb) {
            const int64_t t = ta; ta = tb; tb = t;
            const int p = a; a = b; b = p;
        }
        if (!(a < b && b <= m)) return 0;
        return cl_comb(ta, a - 1) * cl_comb(tb - ta - 1, b - a - 1) * cl_comb(f.d - 1 - tb, m - b);
    }
    if (za && zb) return 0;
    if (!za && !zb) return (a <= m && b <= m) ? f.nd * cl_perm(f.nn - 2, m - 2) : 0;
    const int pn = za ? b : a, pz = za ? a : b;                    // the non-dummy's and the dummy's position
    return (pz == m + 1 && pn <= m) ? cl_perm(f.nn - 1, m - 1) : 0;
}

template <int L, typename F>
__device__ __forceinline__ void lrp_edge_rows(const LrpForm& f, int64_t NL, int32_t eid, int64_t ta, bool za, int64_t tb, bool zb, F&& emit) {
#pragma unroll
    for (int a = 0; a < L; ++a)
#pragma unroll
        for (int b = 0; b < L; ++b) {
            if (a == b) continue;
            const int64_t c = lrp_form_joint(f, ta, za, a, tb, zb, b);
            if (c > 0) emit(NL + (int64_t)eid * (L * (L - 1)) + lrp_off_slot<L>(a, b), c);
        }
}

// Candidate c of the ego of v (d neighbours), 3 d + 1 in all: c <= d the node rows of local node c (0 = v); d < c <= 2 d the
// edge v -> neighbour c - d - 1; 2 d < c <= 3 d the edges of neighbour c - 2 d - 1 into the ego (its own list walked and searched
// for in v's, or v's walked and looked up in its own, whichever list is shorter).
template <int L, typename F>
__device__ __forceinline__ void lrp_collapse_candidate(const LrpIndex& ix, const uint8_t* __restrict__ dummy, int64_t N, int32_t v,
                                                       int32_t base, int32_t d, const LrpForm& f, int64_t c, F&& emit) {
    const int64_t NL = N * L;
    if (c <= d) {
        const int64_t t = c - 1;
        const int32_t node = t < 0 ? v : ix.unbr[base + t];
        const bool z = t >= 0 && dummy != nullptr && dummy[node];
#pragma unroll
        for (int k = 0; k < L; ++k) {
            const int64_t cnt = lrp_form_node(f, t, z, k);
            if (cnt > 0) emit((int64_t)node * L + k, cnt);
        }
        return;
    }
    if (c <= 2 * (int64_t)d) {
        const int64_t t = c - d - 1;
        const bool z = dummy != nullptr && dummy[ix.unbr[base + t]];
        lrp_edge_rows<L>(f, NL, ix.ueid[base + t], -1, false, t, z, emit);
        return;
    }
    const int64_t t = c - 2 * (int64_t)d - 1;
    const int32_t u = ix.unbr[base + t];
    const bool zu = dummy != nullptr && dummy[u];
    const int32_t ub = ix.uptr[u], du = ix.uptr[u + 1] - ub;
    if (du <= d) {
        for (int32_t j = 0; j < du; ++j) {
            const int32_t w = ix.unbr[ub + j];
            int64_t tb = -1;
            if (w != v) {
                int32_t lo = base, hi = base + d;
                while (lo < hi) {
                    const int32_t mid = (lo + hi) >> 1;
                    if (ix.unbr[mid] < w) lo = mid + 1;
                    else hi = mid;
                }
                if (lo >= base + d || ix.unbr[lo] != w) continue;
                tb = lo - base;
            }
            lrp_edge_rows<L>(f, NL, ix.ueid[ub + j], t, zu, tb, tb >= 0 && dummy != nullptr && dummy[w], emit);
        }
    } else {
        const int32_t e0 = lrp_lookup(ix, u, v);
        if (e0 >= 0) lrp_edge_rows<L>(f, NL, e0, t, zu, -1, false, emit);
        for (int32_t tb = 0; tb < d; ++tb) {
            if (tb == t) continue;
            const int32_t w = ix.unbr[base + tb];
            const int32_t e = lrp_lookup(ix, u, w);
            if (e >= 0) lrp_edge_rows<L>(f, NL, e, t, zu, tb, dummy != nullptr && dummy[w], emit);
        }
    }
}

// exclusive scan of one value per thread over the workgroup; total = the sum
__device__ __forceinline__ int64_t lrp_block_scan(int64_t val, int64_t* s, int64_t& total) {
    const int tid = threadIdx.x;
    s[tid] = val;
    __syncthreads();
    for (int off = 1; off < kThreads; off <<= 1) {
        const int64_t add = tid >= off ? s[tid - off] : 0;
        __syncthreads();
        s[tid] += add;
        __syncthreads();
    }
    total = s[kThreads - 1];
    const int64_t excl = s[tid] - val;
    __syncthreads();
    return excl;
}

// One workgroup per node, one candidate per thread and round (a hub's 3 d + 1 candidates are spread over the 256 threads).  The
// count pass sums the entries of every candidate; the fill pass gives every candidate its slot from a workgroup scan -- no
// atomics, so two builds store the same lists -- and evaluates it again to store.  The rows of a node come out in candidate order;
// the caller sorts them.
template <int L, bool FILL>
__global__ __launch_bounds__(kThreads) void lrp_collapse_kernel(int64_t N, LrpIndex ix, const uint8_t* __restrict__ dummy,
                                                                 int64_t* __restrict__ col_count, const int32_t* __restrict__ col_ptr,
                                                                 int32_t* __restrict__ col_rows, int64_t* __restrict__ col_cnt) {
    __shared__ int64_t s_scan[kThreads];
    const int32_t v = blockIdx.x, tid = threadIdx.x;
    const int32_t base = ix.uptr[v], d = ix.uptr[v + 1] - base;
    const LrpForm f = lrp_form(ix.ego[2 * v], L, d, ix.ego[2 * v + 1], ix.count[v]);
    const int64_t C = 3 * (int64_t)d + 1;
    int64_t mine = 0, total = 0;
    int64_t run = FILL ? col_ptr[v] : 0;
    const int64_t end = FILL ? col_ptr[v + 1] : 0;
    for (int64_t c0 = 0; c0 < C; c0 += kThreads) {
        const int64_t c = c0 + tid;
        int64_t n = 0;
        if (c < C) lrp_collapse_candidate<L>(ix, dummy, N, v, base, d, f, c, [&](int64_t, int64_t) { ++n; });
        if (!FILL) {
            mine += n;
            continue;
        }
        int64_t pos = run + lrp_block_scan(n, s_scan, total);
        if (n > 0)
            lrp_collapse_candidate<L>(ix, dummy, N, v, base, d, f, c, [&](int64_t row, int64_t cnt) {
                if (pos < end) {
                    col_rows[pos] = (int32_t)row;
                    col_cnt[pos] = cnt;
                }
                ++pos;
            });
        run += total;
    }
    if (!FILL) {
        lrp_block_scan(mine, s_scan, total);
        if (tid == 0) col_count[v] = total;
    }
}

int check_index(int64_t N, int32_t L, const LrpIndex& ix) {
    DN_REQUIRE(N >= 0 && N < INT32_MAX, "dn_lrp: bad sizes (N = %lld)", (long long)N);
    DN_REQUIRE(L >= 2 && L <= 4, "dn_lrp: the sequence length must be 2, 3 or 4 (got %d)", L);
    if (N == 0) return DN_OK;
    DN_REQUIRE(ix.uptr && ix.ego && ix.count, "dn_lrp: NULL pointer");
    return DN_OK;
}

int check_collapse(int64_t N, int64_t E, int32_t L, const LrpIndex& ix) {
    if (int rc = check_index(N, L, ix)) return rc;
    DN_REQUIRE(E >= 0 && N * L + E * L * (L - 1) < INT32_MAX, "dn_lrp_collapse: %lld nodes and %lld edges: the table rows do not fit int32",
               (long long)N, (long long)E);
    if (N == 0) return DN_OK;
    DN_REQUIRE(E == 0 || (ix.unbr && ix.ueid), "dn_lrp_collapse: NULL pointer");
    return DN_OK;
}

template <bool BWD>
int launch_pool(int64_t N, int32_t L, const LrpPoolArgs& a, hipStream_t st) {
    const dim3 grid((unsigned)N), block(kThreads);
    if (L == 2) hipLaunchKernelGGL((lrp_pool_kernel<2, BWD>), grid, block, 0, st, a);
    else if (L == 3) hipLaunchKernelGGL((lrp_pool_kernel<3, BWD>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((lrp_pool_kernel<4, BWD>), grid, block, 0, st, a);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int check_pool(int64_t N, int64_t E, int32_t H, int32_t L, const LrpIndex& ix, const float* t_node, const float* t_edge) {
    if (int rc = check_index(N, L, ix)) return rc;
    DN_REQUIRE(H >= 16 && H <= 256 && H % 16 == 0, "dn_lrp_pool: unsupported width %d (a multiple of 16 up to 256)", H);
    DN_REQUIRE(E >= 0 && E < INT32_MAX, "dn_lrp_pool: bad sizes (E = %lld)", (long long)E);
    if (N == 0) return DN_OK;
    DN_REQUIRE(t_node != nullptr && (E == 0 || (t_edge && ix.unbr && ix.ueid && ix.upos)), "dn_lrp_pool: NULL pointer");
    return DN_OK;
}

}  // namespace

extern "C" {

int32_t dn_lrp_stage_bytes(void) { return kStageBytes; }
int32_t dn_lrp_pair_nodes(void) { return kPairMax; }

int dn_lrp_ego_index_i32(int64_t N, int32_t L, const int32_t* uptr, const int32_t* unbr, const uint8_t* dummy, int32_t* upos,
                         int32_t* ego, int64_t* count, int32_t* err, dn_stream_t stream) {
    LrpIndex ix{uptr, unbr, nullptr, upos, ego, count};
    if (int rc = check_index(N, L, ix)) return rc;
    if (N == 0) return DN_OK;
    DN_REQUIRE(err != nullptr, "dn_lrp_ego_index: NULL pointer");
    hipLaunchKernelGGL(lrp_ego_index_kernel, dim3((unsigned)dn_cdiv(N, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, N, L, uptr,
                       unbr, dummy, upos, ego, count, err);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_lrp_perm_fill_i32(int64_t N, int32_t L, const int32_t* uptr, const int32_t* unbr, const int32_t* ueid, const int32_t* upos,
                         const int32_t* ego, const int64_t* count, const int32_t* perm_ptr, int64_t P, int32_t* perm_nodes,
                         int32_t* perm_edges, dn_stream_t stream) {
    LrpIndex ix{uptr, unbr, ueid, upos, ego, count};
    if (int rc = check_index(N, L, ix)) return rc;
    DN_REQUIRE(P >= 0 && P * L * L < INT32_MAX, "dn_lrp_perm_fill: %lld sequences do not fit int32 tables", (long long)P);
    if (N == 0 || P == 0) return DN_OK;
    DN_REQUIRE(perm_ptr && perm_nodes && perm_edges, "dn_lrp_perm_fill: NULL pointer");
    const dim3 grid((unsigned)dn_cdiv(P, kThreads)), block(kThreads);
    hipStream_t st = (hipStream_t)stream;
    if (L == 2) hipLaunchKernelGGL(lrp_perm_fill_kernel<2>, grid, block, 0, st, N, P, ix, perm_ptr, perm_nodes, perm_edges);
    else if (L == 3) hipLaunchKernelGGL(lrp_perm_fill_kernel<3>, grid, block, 0, st, N, P, ix, perm_ptr, perm_nodes, perm_edges);
    else hipLaunchKernelGGL(lrp_perm_fill_kernel<4>, grid, block, 0, st, N, P, ix, perm_ptr, perm_nodes, perm_edges);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_lrp_collapse_count_i32(int64_t N, int64_t E, int32_t L, const int32_t* uptr, const int32_t* unbr, const int32_t* ueid,
                              const int32_t* upos, const int32_t* ego, const int64_t* count, const uint8_t* dummy, int64_t* col_count,
                              dn_stream_t stream) {
    LrpIndex ix{uptr, unbr, ueid, upos, ego, count};
    if (int rc = check_collapse(N, E, L, ix)) return rc;
    if (N == 0) return DN_OK;
    DN_REQUIRE(col_count != nullptr, "dn_lrp_collapse_count: NULL pointer");
    const dim3 grid((unsigned)N), block(kThreads);
    hipStream_t st = (hipStream_t)stream;
    if (L == 2) hipLaunchKernelGGL((lrp_collapse_kernel<2, false>), grid, block, 0, st, N, ix, dummy, col_count, nullptr, nullptr, nullptr);
    else if (L == 3) hipLaunchKernelGGL((lrp_collapse_kernel<3, false>), grid, block, 0, st, N, ix, dummy, col_count, nullptr, nullptr, nullptr);
    else hipLaunchKernelGGL((lrp_collapse_kernel<4, false>), grid, block, 0, st, N, ix, dummy, col_count, nullptr, nullptr, nullptr);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_lrp_collapse_fill_i32(int64_t N, int64_t E, int32_t L, const int32_t* uptr, const int32_t* unbr, const int32_t* ueid,
                             const int32_t* upos, const int32_t* ego, const int64_t* count, const uint8_t* dummy, const int32_t* col_ptr,
                             int64_t Q, int32_t* col_rows, int64_t* col_cnt, dn_stream_t stream) {
    LrpIndex ix{uptr, unbr, ueid, upos, ego, count};
    if (int rc = check_collapse(N, E, L, ix)) return rc;
    DN_REQUIRE(Q >= 0 && Q < INT32_MAX, "dn_lrp_collapse_fill: %lld rows do not fit an int32 index", (long long)Q);
    if (N == 0 || Q == 0) return DN_OK;
    DN_REQUIRE(col_ptr && col_rows && col_cnt, "dn_lrp_collapse_fill: NULL pointer");
    const dim3 grid((unsigned)N), block(kThreads);
    hipStream_t st = (hipStream_t)stream;
    if (L == 2) hipLaunchKernelGGL((lrp_collapse_kernel<2, true>), grid, block, 0, st, N, ix, dummy, nullptr, col_ptr, col_rows, col_cnt);
    else if (L == 3) hipLaunchKernelGGL((lrp_collapse_kernel<3, true>), grid, block, 0, st, N, ix, dummy, nullptr, col_ptr, col_rows, col_cnt);
    else hipLaunchKernelGGL((lrp_collapse_kernel<4, true>), grid, block, 0, st, N, ix, dummy, nullptr, col_ptr, col_rows, col_cnt);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_lrp_pool_fwd_f32(int64_t N, int64_t E, int32_t H, int32_t L, const int32_t* uptr, const int32_t* unbr, const int32_t* ueid,
                        const int32_t* upos, const int32_t* ego, const int64_t* count, const float* t_node, const float* t_edge,
                        const float* bias, const float* factor, int32_t pool_mean, int32_t act_on, float slope, float* pooled,
                        float* out, dn_stream_t stream) {
    LrpPoolArgs a{};
    a.ix = LrpIndex{uptr, unbr, ueid, upos, ego, count};
    if (int rc = check_pool(N, E, H, L, a.ix, t_node, t_edge)) return rc;
    if (N == 0) return DN_OK;
    DN_REQUIRE(out != nullptr, "dn_lrp_pool_fwd: NULL pointer");
    a.H = H; a.t_node = t_node; a.t_edge = t_edge; a.bias = bias; a.factor = factor;
    a.pool_mean = pool_mean; a.act_on = act_on; a.slope = slope; a.pooled = pooled; a.out = out;
    return launch_pool<false>(N, L, a, (hipStream_t)stream);
}

int dn_lrp_pool_bwd_f32(int64_t N, int64_t E, int32_t H, int32_t L, const int32_t* uptr, const int32_t* unbr, const int32_t* ueid,
                        const int32_t* upos, const int32_t* ego, const int64_t* count, const float* t_node, const float* t_edge,
                        const float* bias, const float* factor, int32_t pool_mean, int32_t act_on, float slope, const float* pooled,
                        const float* g, float* d_tnode, float* d_tedge, float* d_bias, float* d_factor, dn_stream_t stream) {
    LrpPoolArgs a{};
    a.ix = LrpIndex{uptr, unbr, ueid, upos, ego, count};
    if (int rc = check_pool(N, E, H, L, a.ix, t_node, t_edge)) return rc;
    if (N == 0) return DN_OK;
    DN_REQUIRE(g && d_tnode && (E == 0 || d_tedge), "dn_lrp_pool_bwd: NULL pointer");
    DN_REQUIRE(factor == nullptr || (pooled && d_factor), "dn_lrp_pool_bwd: factor needs pooled and d_factor");
    a.H = H; a.t_node = t_node; a.t_edge = t_edge; a.bias = bias; a.factor = factor;
    a.pool_mean = pool_mean; a.act_on = act_on; a.slope = slope; a.pooled = const_cast<float*>(pooled); a.g = g;
    a.d_tnode = d_tnode; a.d_tedge = d_tedge; a.d_bias = d_bias; a.d_factor = d_factor;
    return launch_pool<true>(N, L, a, (hipStream_t)stream);
}

}  // extern "C"
