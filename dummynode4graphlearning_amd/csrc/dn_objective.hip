// The SI training objective and the per-sample evaluation errors (subgraph_isomorphism/train.py:776-821 and :1101-1173) as three
// memory-bound kernels; docs/LAB_NOTES.md "SI training objective", DESIGN.md "SI training objective".
//
// The terms.  crit(d) = |d| (MAE), d^2 (MSE) or smooth-L1 with beta 1 (SMSE); s = the leaky slope; m = the mask; B = the pairs:
//   eval    = 1/B sum_b crit_eval(relu(pred_c_b) - c_b)
//   bp      = 1/B sum_b crit(lrelu(pred_c_b, s) - c_b)
//   x_loss  = 1/B sum_bj crit(lrelu(m p_bj, s) - m w_bj)                  x = v (nodes), e (edges); a masked entry is 0 against 0
//   x_reg   = 1/B sum_bj crit(relu(m p_bj - pred_c_b))                    over ALL positions: a masked one gives crit(relu(-pred_c_b))
//   rep_reg = sum_reps (sum crit(rep)) / denom                            denom = numel / size(1), given by the caller
//   loss    = bp + rep_reg_w rep_reg + match_loss_w (v_loss + e_loss) + match_reg_w (v_reg + e_reg)
// The gradient of x_reg reaches pred_x at masked positions too (the reference zeroes them in place outside autograd).
//
// The launches.  Workgroups [0, row_blocks) own four pairs each, a wavefront a pair: the wavefront walks the pair's L_v + L_e
// positions.  The workgroups behind them own 4096-element chunks of the representations, 16 bytes a lane and load where the
// tensor's base is 16-byte aligned (a partial last piece, and a tensor that is not aligned, go element by element: the same
// elements to the same lane either way, so the result does not depend on the alignment).  Everything is accumulated in fp64: a
// lane in index order, a wavefront by xor shuffles, the four wavefronts in order; a workgroup stores six partial sums and a
// closing launch of one workgroup adds them in index order.  No atomics; the grid depends on the shapes only; two runs give the
// same bits.  The backward is the same grid in one launch: the pair's wavefront also sums the regulariser's gradient at pred_c.
//
// The backward's arithmetic.  An element of d pred_x is the SUM of two products (the match loss's and the regulariser's), which may
// cancel; the reference's fp32 autograd rounds each product on the way, so an exact evaluation differs from it by more than a few
// ulps of the result there.  The backward therefore performs torch's own fp32 operations in torch's order (CritBack below: the
// criterion's backward kernel, then the activation's, then the one addition; no contraction into FMAs): on fp32 inputs an
// elementwise gradient has the reference's bits.  d pred_c adds those fp32 addends in fp64 and rounds once.
#include <hip/hip_runtime.h>

#include "dn_common.h"
#include "dn_hip.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kChunk = 4096;             // elements of a representation per workgroup
constexpr int kSlots = 6;                // partial sums a workgroup stores
constexpr int kMaxReps = DN_OBJECTIVE_MAX_REPS;

struct Side {                            // pred, mask, target [B, L]; dpred the backward's output (NULL: not wanted)
    const void* pred;
    const uint8_t* mask;
    const void* target;
    void* dpred;
    int64_t L;
    int32_t pred_dt, target_dt;
};

struct Rep {
    const void* x;
    void* dx;
    int64_t numel, first_block;
    double denom;
    int32_t dt, pad;
};

struct Params {
    int64_t B, row_blocks, num_blocks;
    const void* pred_c;
    const void* counts;
    void* dpred_c;
    int32_t pred_c_dt, counts_dt, bp_crit, eval_crit, num_reps, pad;
    double slope, rep_reg_w, match_loss_w, match_reg_w;
    float slope_f, rep_reg_w_f, match_loss_w_f, match_reg_w_f;                 // as torch multiplies by them in fp32
    Side v, e;
    Rep rep[kMaxReps];
};

__device__ __forceinline__ double ldd(const void* p, int32_t dt, int64_t i) {
    return dt == DN_OBJECTIVE_BF16 ? (double)(float)static_cast<const bf16_t*>(p)[i] : (double)static_cast<const float*>(p)[i];
}

__device__ __forceinline__ void std_(void* p, int32_t dt, int64_t i, double x) {
    if (dt == DN_OBJECTIVE_BF16) static_cast<bf16_t*>(p)[i] = (bf16_t)(float)x;
    else static_cast<float*>(p)[i] = (float)x;
}

__device__ __forceinline__ double crit(int32_t c, double d) {
    const double a = fabs(d);
    return c == DN_OBJECTIVE_MSE ? d * d : (c == DN_OBJECTIVE_MAE ? a : (a < 1.0 ? 0.5 * d * d : a - 0.5));
}

__device__ __forceinline__ double lrelu(double x, double s) { return x > 0.0 ? x : x * s; }

__device__ __forceinline__ float ldf(const void* p, int32_t dt, int64_t i) {
    return dt == DN_OBJECTIVE_BF16 ? (float)static_cast<const bf16_t*>(p)[i] : static_cast<const float*>(p)[i];
}

__device__ __forceinline__ void stf(void* p, int32_t dt, int64_t i, float x) {
    if (dt == DN_OBJECTIVE_BF16) static_cast<bf16_t*>(p)[i] = (bf16_t)x;
    else static_cast<float*>(p)[i] = x;
}

// torch's backward of a mean-reduced criterion over n elements, as its kernels compute it in fp32: upstream gv, d = input - target.
//   MSE  (norm d) gv, norm = 2 / n        MAE  (gv / n) sign(d)        SMSE  -norm gv | (norm d) gv | norm gv, norm = 1 / n
struct CritBack {
    float gv, norm, gv_n;
    int32_t c;
    __device__ __forceinline__ CritBack(int32_t crit, float upstream, double n)
        : gv(upstream), norm((float)((crit == DN_OBJECTIVE_MSE ? 2.0 : 1.0) / n)), gv_n(__fdiv_rn(upstream, (float)n)), c(crit) {}
    __device__ __forceinline__ float operator()(float d) const {
        if (c == DN_OBJECTIVE_MSE) return __fmul_rn(__fmul_rn(norm, d), gv);
        if (c == DN_OBJECTIVE_MAE) return __fmul_rn(gv_n, d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
        return d <= -1.f ? __fmul_rn(-norm, gv) : (d >= 1.f ? __fmul_rn(norm, gv) : __fmul_rn(__fmul_rn(norm, d), gv));
    }
};

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}

// the 8 (bf16) or 4 (fp32) elements of 16-byte piece q of a flat tensor, as doubles; count = how many of them exist
template <bool BF16>
__device__ __forceinline__ int load_piece(const void* x, int64_t numel, int64_t q, bool aligned, double (&v)[8]) {
    constexpr int V = BF16 ? 8 : 4;
    const int64_t e0 = q * V;
    if (e0 >= numel) return 0;
    const int n = numel - e0 >= V ? V : (int)(numel - e0);
    if (aligned && n == V) {
        if (BF16) {
            const uint4 w = *reinterpret_cast<const uint4*>(static_cast<const bf16_t*>(x) + e0);
            const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v[2 * i] = (double)__uint_as_float(u[i] << 16);
                v[2 * i + 1] = (double)__uint_as_float(u[i] & 0xffff0000u);
            }
        } else {
            const float4 w = *reinterpret_cast<const float4*>(static_cast<const float*>(x) + e0);
            v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < V; ++i)
            if (i < n) v[i] = ldd(x, BF16 ? DN_OBJECTIVE_BF16 : DN_OBJECTIVE_F32, e0 + i);
    }
    return n;
}

template <bool BF16>
__device__ __forceinline__ void store_piece(void* x, int64_t q, bool aligned, int n, const double (&v)[8]) {
    constexpr int V = BF16 ? 8 : 4;
    const int64_t e0 = q * V;
    if (aligned && n == V) {
        if (BF16) {
            uint4 w;
            w.x = pack_bf16x2((float)v[0], (float)v[1]);
            w.y = pack_bf16x2((float)v[2], (float)v[3]);
            w.z = pack_bf16x2((float)v[4], (float)v[5]);
            w.w = pack_bf16x2((float)v[6], (float)v[7]);
            *reinterpret_cast<uint4*>(static_cast<bf16_t*>(x) + e0) = w;
        } else {
            *reinterpret_cast<float4*>(static_cast<float*>(x) + e0) = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < V; ++i)
            if (i < n) std_(x, BF16 ? DN_OBJECTIVE_BF16 : DN_OBJECTIVE_F32, e0 + i, v[i]);
    }
}

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

__device__ __forceinline__ int rep_of_block(const Params& p, int64_t blk) {       // the last r with first_block <= blk
    int r = 0;
#pragma unroll
    for (int i = 1; i < kMaxReps; ++i)
        if (i < p.num_reps && p.rep[i].first_block <= blk) r = i;
    return r;
}

// sum crit(x) over this workgroup's chunk of a representation (forward), or dx = back(x) over it (backward)
template <bool BF16, bool BWD>
__device__ __forceinline__ double rep_chunk(const Rep& r, int32_t c, int64_t chunk, int tid, const CritBack& back) {
    constexpr int V = BF16 ? 8 : 4;
    constexpr int kPieces = kChunk / V;                                            // per workgroup: 2 or 4 per lane
    const bool al = aligned16(r.x) && (!BWD || aligned16(r.dx));
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < kPieces / kBlock; ++k) {
        const int64_t q = chunk * kPieces + k * kBlock + tid;
        double v[8];
        const int n = load_piece<BF16>(r.x, r.numel, q, al, v);
        if (BWD) {
            if (n > 0) {
#pragma unroll
                for (int i = 0; i < V; ++i) v[i] = i < n ? (double)back((float)v[i]) : 0.0;
                store_piece<BF16>(r.dx, q, al, n, v);
            }
        } else {
#pragma unroll
            for (int i = 0; i < V; ++i)
                if (i < n) acc += crit(c, v[i]);
        }
    }
    return acc;
}

// one side of one pair, a wavefront: the match loss and the regulariser summed over the pair's L positions
__device__ __forceinline__ void side_fwd(const Side& s, int64_t b, int lane, double pc, int32_t c, double slope, double& loss, double& reg) {
    if (s.pred == nullptr) return;
    for (int64_t j = lane; j < s.L; j += 64) {
        const int64_t i = b * s.L + j;
        const bool m = s.mask[i] != 0;
        const double pv = m ? ldd(s.pred, s.pred_dt, i) : 0.0, wt = m ? ldd(s.target, s.target_dt, i) : 0.0;
        loss += crit(c, lrelu(pv, slope) - wt);
        const double z = pv - pc;
        reg += crit(c, z > 0.0 ? z : 0.0);
    }
}

// ... its gradients: dpred stored (when wanted), the regulariser's part of d pred_c returned as a lane's partial sum
__device__ __forceinline__ double side_bwd(const Side& s, int64_t b, int64_t B, int lane, float pc, int32_t c, float slope, float g_loss,
                                           float g_reg) {
    double racc = 0.0;
    if (s.pred == nullptr) return racc;
    const float Lf = (float)s.L;                                               // x_loss = crit(..) * pred.size(1): the upstream is g w L
    const CritBack loss(c, __fmul_rn(g_loss, Lf), (double)B * (double)s.L), reg(c, __fmul_rn(g_reg, Lf), (double)B * (double)s.L);
    for (int64_t j = lane; j < s.L; j += 64) {
        const int64_t i = b * s.L + j;
        const bool m = s.mask[i] != 0;
        const float pv = m ? ldf(s.pred, s.pred_dt, i) : 0.f, wt = m ? ldf(s.target, s.target_dt, i) : 0.f;
        float a1 = loss(__fsub_rn(pv > 0.f ? pv : __fmul_rn(pv, slope), wt));
        if (!(pv > 0.f)) a1 = __fmul_rn(a1, slope);
        const float z = __fsub_rn(pv, pc), a2 = z > 0.f ? reg(z) : 0.f;
        if (s.dpred != nullptr) stf(s.dpred, s.pred_dt, i, __fadd_rn(a1, a2));
        racc += (double)a2;
    }
    return racc;
}

__global__ __launch_bounds__(kBlock) void objective_fwd_kernel(Params p, double* __restrict__ partials) {
    __shared__ double s_part[kWaves][kSlots];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t blk = blockIdx.x;
    double acc[kSlots] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (blk < p.row_blocks) {
        const int64_t b = blk * kWaves + wave;
        if (b < p.B) {                                                         // (uniform in the wavefront)
            const double pc = ldd(p.pred_c, p.pred_c_dt, b), c = ldd(p.counts, p.counts_dt, b);
            if (lane == 0) {
                acc[0] = crit(p.eval_crit, (pc > 0.0 ? pc : 0.0) - c);
                acc[1] = crit(p.bp_crit, lrelu(pc, p.slope) - c);
            }
            side_fwd(p.v, b, lane, pc, p.bp_crit, p.slope, acc[2], acc[4]);
            side_fwd(p.e, b, lane, pc, p.bp_crit, p.slope, acc[3], acc[5]);
        }
    } else {
        const int ri = rep_of_block(p, blk);
        const Rep& r = p.rep[ri];
        const CritBack none(p.bp_crit, 0.f, 1.0);
        acc[0] = r.dt == DN_OBJECTIVE_BF16 ? rep_chunk<true, false>(r, p.bp_crit, blk - r.first_block, tid, none)
                                           : rep_chunk<false, false>(r, p.bp_crit, blk - r.first_block, tid, none);
    }
#pragma unroll
    for (int k = 0; k < kSlots; ++k) {
        const double s = wave_sum(acc[k]);
        if (lane == 0) s_part[wave][k] = s;
    }
    __syncthreads();
    if (tid < kSlots) {
        double s = s_part[0][tid];
        for (int w = 1; w < kWaves; ++w) s += s_part[w][tid];
        partials[blk * kSlots + tid] = s;
    }
}

// slot `slot` of the workgroups [beg, end) added in index order: lane-strided in order, then the fixed tree (every thread returns it)
__device__ __forceinline__ double block_sum(const double* __restrict__ partials, int64_t beg, int64_t end, int slot, double* s_w) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double a = 0.0;
    for (int64_t i = beg + tid; i < end; i += kBlock) a += partials[i * kSlots + slot];
    a = wave_sum(a);
    __syncthreads();                                                           // (the previous call's reads of s_w are over)
    if (lane == 0) s_w[wave] = a;
    __syncthreads();
    double s = s_w[0];
    for (int w = 1; w < kWaves; ++w) s += s_w[w];
    return s;
}

__global__ __launch_bounds__(kBlock) void objective_close_kernel(Params p, const double* __restrict__ partials, double* __restrict__ terms,
                                                                 float* __restrict__ loss) {
    __shared__ double s_w[kWaves];
    double row[kSlots];
    for (int k = 0; k < kSlots; ++k) row[k] = block_sum(partials, 0, p.row_blocks, k, s_w) / (double)p.B;
    double rep = 0.0;
    for (int r = 0; r < p.num_reps; ++r) {
        const int64_t end = r + 1 < p.num_reps ? p.rep[r + 1].first_block : p.num_blocks;
        rep += block_sum(partials, p.rep[r].first_block, end, 0, s_w) / p.rep[r].denom;
    }
    if (threadIdx.x == 0) {
        const double total = row[1] + p.rep_reg_w * rep + p.match_loss_w * (row[2] + row[3]) + p.match_reg_w * (row[4] + row[5]);
        terms[0] = row[0];
        terms[1] = total;
        terms[2] = row[2];
        terms[3] = row[3];
        terms[4] = row[4];
        terms[5] = row[5];
        terms[6] = rep;
        *loss = (float)total;
    }
}

__global__ __launch_bounds__(kBlock) void objective_bwd_kernel(Params p, const float* __restrict__ gup) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t blk = blockIdx.x;
    const float g = *gup;
    if (blk < p.row_blocks) {
        const int64_t b = blk * kWaves + wave;
        if (b >= p.B) return;                                                  // (uniform in the wavefront)
        const float pc = ldf(p.pred_c, p.pred_c_dt, b), c = ldf(p.counts, p.counts_dt, b);
        const float g_loss = __fmul_rn(g, p.match_loss_w_f), g_reg = __fmul_rn(g, p.match_reg_w_f);
        double racc = side_bwd(p.v, b, p.B, lane, pc, p.bp_crit, p.slope_f, g_loss, g_reg);
        racc += side_bwd(p.e, b, p.B, lane, pc, p.bp_crit, p.slope_f, g_loss, g_reg);
        racc = wave_sum(racc);
        if (lane == 0 && p.dpred_c != nullptr) {
            const CritBack bp(p.bp_crit, g, (double)p.B);
            float a0 = bp(__fsub_rn(pc > 0.f ? pc : __fmul_rn(pc, p.slope_f), c));
            if (!(pc > 0.f)) a0 = __fmul_rn(a0, p.slope_f);
            std_(p.dpred_c, p.pred_c_dt, b, (double)a0 - racc);
        }
    } else {
        const int ri = rep_of_block(p, blk);
        const Rep& r = p.rep[ri];
        if (r.dx == nullptr) return;
        // rep_reg adds crit(rep) * rep.size(1): the upstream is g rep_reg_w size(1), size(1) = numel / denom
        const CritBack back(p.bp_crit, __fmul_rn(__fmul_rn(g, p.rep_reg_w_f), (float)((double)r.numel / r.denom)), (double)r.numel);
        if (r.dt == DN_OBJECTIVE_BF16) rep_chunk<true, true>(r, p.bp_crit, blk - r.first_block, tid, back);
        else rep_chunk<false, true>(r, p.bp_crit, blk - r.first_block, tid, back);
    }
}

// per pair: AE = |relu(pred_c) - c|, SE = AE^2 (both rounded as the reference's fp32 ops round them), NED / EED = sum_j |relu(p_bj) - w_bj|
// over all positions (no mask), cls = (c > 0) + 2 (relu(pred_c) > 0): the four counts of the epoch's AUC
__global__ __launch_bounds__(kBlock) void objective_eval_kernel(Params p, int64_t offset, float* __restrict__ ae, float* __restrict__ se,
                                                                float* __restrict__ ned, float* __restrict__ eed, int32_t* __restrict__ cls) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = (int64_t)blockIdx.x * kWaves + wave;
    if (b >= p.B) return;                                                      // (uniform in the wavefront)
    double sums[2] = {0.0, 0.0};
    const Side* sides[2] = {&p.v, &p.e};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const Side& s = *sides[k];
        if (s.pred == nullptr) continue;
        for (int64_t j = lane; j < s.L; j += 64) {
            const double pv = ldd(s.pred, s.pred_dt, b * s.L + j);
            sums[k] += fabs((pv > 0.0 ? pv : 0.0) - ldd(s.target, s.target_dt, b * s.L + j));
        }
    }
    sums[0] = wave_sum(sums[0]);
    sums[1] = wave_sum(sums[1]);
    if (lane == 0) {
        const float pc = (float)ldd(p.pred_c, p.pred_c_dt, b), c = (float)ldd(p.counts, p.counts_dt, b);
        const float r = pc > 0.f ? pc : 0.f, a = fabsf(r - c);
        ae[offset + b] = a;
        se[offset + b] = a * a;
        ned[offset + b] = (float)sums[0];
        eed[offset + b] = (float)sums[1];
        cls[offset + b] = (c > 0.f ? 1 : 0) + (r > 0.f ? 2 : 0);
    }
}

bool dt_ok(int32_t dt) { return dt == DN_OBJECTIVE_F32 || dt == DN_OBJECTIVE_BF16; }
bool crit_ok(int32_t c) { return c == DN_OBJECTIVE_MAE || c == DN_OBJECTIVE_MSE || c == DN_OBJECTIVE_SMSE; }

int check_side(const char* what, const char* name, int64_t L, const void* pred, int32_t pred_dt, const uint8_t* mask, const void* target,
               int32_t target_dt, bool need_mask, Side* out) {
    *out = Side{nullptr, nullptr, nullptr, nullptr, 0, 0, 0};
    if (pred == nullptr && mask == nullptr && target == nullptr && L == 0) return DN_OK;       // the side is absent
    DN_REQUIRE(L >= 1 && L <= 0x7fffffffLL, "%s: bad sizes (L_%s = %lld)", what, name, (long long)L);
    DN_REQUIRE(pred && target && (mask || !need_mask), "%s: NULL pointer (the %s side needs its prediction, %starget)", what, name,
               need_mask ? "mask and " : "");
    DN_REQUIRE(dt_ok(pred_dt) && dt_ok(target_dt), "%s: unknown dtype code on the %s side", what, name);
    *out = Side{pred, mask, target, nullptr, L, pred_dt, target_dt};
    return DN_OK;
}

// the grid: row_blocks workgroups of four pairs, then every representation's chunks
int plan(const char* what, int64_t B, int32_t num_reps, const int64_t* rep_numel, Params* p) {
    DN_REQUIRE(B >= 1 && B <= 0x7fffffffLL, "%s: bad sizes (B = %lld)", what, (long long)B);
    DN_REQUIRE(num_reps >= 0 && num_reps <= kMaxReps, "%s: at most %d representations (got %d)", what, kMaxReps, num_reps);
    DN_REQUIRE(num_reps == 0 || rep_numel, "%s: NULL pointer (rep_numel)", what);
    p->B = B;
    p->row_blocks = dn_cdiv(B, kWaves);
    p->num_reps = num_reps;
    int64_t blocks = p->row_blocks;
    for (int r = 0; r < num_reps; ++r) {
        DN_REQUIRE(rep_numel[r] >= 1 && rep_numel[r] <= (int64_t)1 << 40, "%s: bad sizes (representation %d has %lld elements)", what, r,
                   (long long)rep_numel[r]);
        p->rep[r].numel = rep_numel[r];
        p->rep[r].first_block = blocks;
        blocks += dn_cdiv(rep_numel[r], kChunk);
    }
    DN_REQUIRE(blocks <= 0x7fffffffLL, "%s: bad sizes (%lld workgroups)", what, (long long)blocks);
    p->num_blocks = blocks;
    return DN_OK;
}

int fill(const char* what, Params* p, int64_t B, const void* pred_c, int32_t pred_c_dt, const void* counts, int32_t counts_dt, int64_t Lv,
         const void* pred_v, int32_t pred_v_dt, const uint8_t* v_mask, const void* v_target, int32_t v_target_dt, int64_t Le,
         const void* pred_e, int32_t pred_e_dt, const uint8_t* e_mask, const void* e_target, int32_t e_target_dt, int32_t num_reps,
         const void* const* reps, const int64_t* rep_numel, const int64_t* rep_denom, const int32_t* rep_dt, int32_t bp_crit,
         int32_t eval_crit, double neg_slp, double rep_reg_w, double match_loss_w, double match_reg_w, bool need_mask) {
    *p = Params{};
    if (plan(what, B, num_reps, rep_numel, p) != DN_OK) return DN_ERR_ARG;
    DN_REQUIRE(pred_c && counts, "%s: NULL pointer (pred_c, counts)", what);
    DN_REQUIRE(dt_ok(pred_c_dt) && dt_ok(counts_dt), "%s: unknown dtype code (pred_c %d, counts %d)", what, pred_c_dt, counts_dt);
    DN_REQUIRE(crit_ok(bp_crit) && crit_ok(eval_crit), "%s: unknown criterion (bp_loss %d, eval_metric %d)", what, bp_crit, eval_crit);
    if (check_side(what, "v", Lv, pred_v, pred_v_dt, v_mask, v_target, v_target_dt, need_mask, &p->v) != DN_OK) return DN_ERR_ARG;
    if (check_side(what, "e", Le, pred_e, pred_e_dt, e_mask, e_target, e_target_dt, need_mask, &p->e) != DN_OK) return DN_ERR_ARG;
    DN_REQUIRE(num_reps == 0 || (reps && rep_denom && rep_dt), "%s: NULL pointer (reps, rep_denom, rep_dt)", what);
    for (int r = 0; r < num_reps; ++r) {
        DN_REQUIRE(reps[r], "%s: NULL pointer (representation %d)", what, r);
        DN_REQUIRE(dt_ok(rep_dt[r]), "%s: unknown dtype code (representation %d: %d)", what, r, rep_dt[r]);
        DN_REQUIRE(rep_denom[r] >= 1, "%s: bad sizes (representation %d: denominator %lld)", what, r, (long long)rep_denom[r]);
        p->rep[r].x = reps[r];
        p->rep[r].denom = (double)rep_denom[r];
        p->rep[r].dt = rep_dt[r];
    }
    p->pred_c = pred_c;
    p->counts = counts;
    p->pred_c_dt = pred_c_dt;
    p->counts_dt = counts_dt;
    p->bp_crit = bp_crit;
    p->eval_crit = eval_crit;
    p->slope = neg_slp;
    p->rep_reg_w = rep_reg_w;
    p->match_loss_w = match_loss_w;
    p->match_reg_w = match_reg_w;
    p->slope_f = (float)neg_slp;
    p->rep_reg_w_f = (float)rep_reg_w;
    p->match_loss_w_f = (float)match_loss_w;
    p->match_reg_w_f = (float)match_reg_w;
    return DN_OK;
}

}  // namespace

extern "C" {

size_t dn_objective_workspace_bytes(int64_t B, int32_t num_reps, const int64_t* rep_numel) {
    Params p{};
    if (plan("dn_objective_workspace_bytes", B, num_reps, rep_numel, &p) != DN_OK) return 0;
    return (size_t)p.num_blocks * kSlots * sizeof(double);
}

int dn_objective_fwd(int64_t B, const void* pred_c, int32_t pred_c_dt, const void* counts, int32_t counts_dt, int64_t Lv, const void* pred_v,
                     int32_t pred_v_dt, const uint8_t* v_mask, const void* v_target, int32_t v_target_dt, int64_t Le, const void* pred_e,
                     int32_t pred_e_dt, const uint8_t* e_mask, const void* e_target, int32_t e_target_dt, int32_t num_reps,
                     const void* const* reps, const int64_t* rep_numel, const int64_t* rep_denom, const int32_t* rep_dt, int32_t bp_crit,
                     int32_t eval_crit, double neg_slp, double rep_reg_w, double match_loss_w, double match_reg_w, double* terms,
                     float* loss, void* workspace, size_t workspace_bytes, dn_stream_t stream) {
    Params p;
    if (fill("dn_objective_fwd", &p, B, pred_c, pred_c_dt, counts, counts_dt, Lv, pred_v, pred_v_dt, v_mask, v_target, v_target_dt, Le, pred_e,
             pred_e_dt, e_mask, e_target, e_target_dt, num_reps, reps, rep_numel, rep_denom, rep_dt, bp_crit, eval_crit, neg_slp, rep_reg_w,
             match_loss_w, match_reg_w, true) != DN_OK)
        return DN_ERR_ARG;
    DN_REQUIRE(terms && loss && workspace, "dn_objective_fwd: NULL pointer (terms, loss, workspace)");
    DN_REQUIRE(workspace_bytes >= (size_t)p.num_blocks * kSlots * sizeof(double) && (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0,
               "dn_objective_fwd: workspace too small or not 8-byte aligned (%zu bytes)", workspace_bytes);
    double* partials = static_cast<double*>(workspace);
    hipLaunchKernelGGL(objective_fwd_kernel, dim3((unsigned)p.num_blocks), dim3(kBlock), 0, (hipStream_t)stream, p, partials);
    DN_CHECK_LAUNCH();
    hipLaunchKernelGGL(objective_close_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, p, partials, terms, loss);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_objective_bwd(int64_t B, const float* grad_loss, const void* pred_c, int32_t pred_c_dt, const void* counts, int32_t counts_dt,
                     int64_t Lv, const void* pred_v, int32_t pred_v_dt, const uint8_t* v_mask, const void* v_target, int32_t v_target_dt,
                     int64_t Le, const void* pred_e, int32_t pred_e_dt, const uint8_t* e_mask, const void* e_target, int32_t e_target_dt,
                     int32_t num_reps, const void* const* reps, const int64_t* rep_numel, const int64_t* rep_denom, const int32_t* rep_dt,
                     int32_t bp_crit, double neg_slp, double rep_reg_w, double match_loss_w, double match_reg_w, void* d_pred_c,
                     void* d_pred_v, void* d_pred_e, void* const* d_reps, dn_stream_t stream) {
    Params p;
    if (fill("dn_objective_bwd", &p, B, pred_c, pred_c_dt, counts, counts_dt, Lv, pred_v, pred_v_dt, v_mask, v_target, v_target_dt, Le, pred_e,
             pred_e_dt, e_mask, e_target, e_target_dt, num_reps, reps, rep_numel, rep_denom, rep_dt, bp_crit, bp_crit, neg_slp, rep_reg_w,
             match_loss_w, match_reg_w, true) != DN_OK)
        return DN_ERR_ARG;
    DN_REQUIRE(grad_loss, "dn_objective_bwd: NULL pointer (grad_loss)");
    DN_REQUIRE(num_reps == 0 || d_reps, "dn_objective_bwd: NULL pointer (d_reps)");
    DN_REQUIRE((d_pred_v == nullptr || p.v.pred) && (d_pred_e == nullptr || p.e.pred),
               "dn_objective_bwd: a gradient is asked for a side that is absent");
    p.dpred_c = d_pred_c;
    p.v.dpred = d_pred_v;
    p.e.dpred = d_pred_e;
    for (int r = 0; r < num_reps; ++r) p.rep[r].dx = d_reps[r];
    hipLaunchKernelGGL(objective_bwd_kernel, dim3((unsigned)p.num_blocks), dim3(kBlock), 0, (hipStream_t)stream, p, grad_loss);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_objective_eval(int64_t B, const void* pred_c, int32_t pred_c_dt, const void* counts, int32_t counts_dt, int64_t Lv, const void* pred_v,
                      int32_t pred_v_dt, const void* v_target, int32_t v_target_dt, int64_t Le, const void* pred_e, int32_t pred_e_dt,
                      const void* e_target, int32_t e_target_dt, int64_t offset, int64_t capacity, float* ae, float* se, float* ned,
                      float* eed, int32_t* cls, dn_stream_t stream) {
    Params p;
    if (fill("dn_objective_eval", &p, B, pred_c, pred_c_dt, counts, counts_dt, Lv, pred_v, pred_v_dt, nullptr, v_target, v_target_dt, Le, pred_e,
             pred_e_dt, nullptr, e_target, e_target_dt, 0, nullptr, nullptr, nullptr, nullptr, DN_OBJECTIVE_MAE, DN_OBJECTIVE_MAE, 0.0, 0.0,
             0.0, 0.0, false) != DN_OK)
        return DN_ERR_ARG;
    DN_REQUIRE(ae && se && ned && eed && cls, "dn_objective_eval: NULL pointer (ae, se, ned, eed, cls)");
    DN_REQUIRE(offset >= 0 && capacity >= 1 && offset <= capacity - B, "dn_objective_eval: bad sizes (%lld pairs at offset %lld of %lld)",
               (long long)B, (long long)offset, (long long)capacity);
    hipLaunchKernelGGL(objective_eval_kernel, dim3((unsigned)p.row_blocks), dim3(kBlock), 0, (hipStream_t)stream, p, offset, ae, se, ned, eed,
                       cls);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

}  // extern "C"
