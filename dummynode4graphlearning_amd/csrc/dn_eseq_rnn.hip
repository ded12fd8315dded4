// The RNN count model's recurrence on edge sequences in rows layout (DESIGN.md "SI count models: RNN"), fp32, gfx950.
//
// The input side P[b, t] = x0[b, t] @ W_ih^T + b is a batch product made before these kernels run (every bias folded in, except the
// GRU's b_hn).  With a = h[t'] @ W_hh^T, t' the step before t in the direction's order (h = c = 0 before the first step):
//
//   LSTM   i, f, o = sigmoid(P_i + a_i), ..., g = tanh(P_g + a_g);  c = f c' + i g;  h = o tanh(c)         saved: i f g o c
//   GRU    r = sigmoid(P_r + a_r), z = sigmoid(P_z + a_z), hn = a_n + b_hn, n = tanh(P_n + r hn);  h = (1 - z) n + z h'
//                                                                                                         saved: r z n hn
//   tanh   h = tanh(P + a)
//   y[b, t] = h gate[b, t] (+ x0[b, t] when residual);  h itself is kept for the backward pass and the W_hh gradient.
//
// One workgroup owns 16 sequences (the M of mfma_f32_16x16x4f32, exact f32) and one direction and walks the time axis itself.  Wave w
// owns hidden units 16 w .. 16 w + 15 with ALL their gates: its W_hh rows stay in registers for the whole launch, the cell update is
// wave-local, and only h crosses waves, through a double-buffered LDS image behind ONE workgroup barrier per step.  Every wave of a
// workgroup runs the same trip count (it depends on blockIdx and lo[] of the 16 sequences only).  P of step t + 1 is requested before
// the products of step t.
//
// Pad steps are NOT skipped in the forward direction: the input is zero there, but the biases drive h and c, and the first live step
// sees that state.  The reverse direction of a bidirectional layer stops at the first position that any of its 16 sequences may
// carry a gate at (lo[]): to the left every output is gated to zero and nothing reads the state; y, h and the gradients are written
// as zeros there.
//
// Backward: the same tiling, time walked the other way, dh (and dc) carried in registers in the layout the products leave them in;
// the pre-activation gradients cross waves through LDS (one barrier per step) for dh' = dpre @ W_hh.  It writes dP [B, L, D G Hd] and,
// for the GRU, the hidden-side n term dhn = dn_pre r.  The batch products (dx, dW_ih, dW_hh, the biases) are row kernels over B L
// rows.  No atomics anywhere: bit-identical from run to run.
#include "dn_common.h"

namespace {

constexpr int kSeq = 16;
constexpr int kLstm = 0, kGru = 1, kTanh = 2;

__host__ __device__ constexpr int rnn_gates(int cell) { return cell == kLstm ? 4 : (cell == kGru ? 3 : 1); }
__host__ __device__ constexpr int rnn_saved(int cell) { return cell == kLstm ? 5 : (cell == kGru ? 4 : 0); }

__device__ __forceinline__ float sigm(float v) { return 1.f / (1.f + expf(-v)); }

// the first position the reverse direction has to reach for the 16 sequences from b0 (0 for the forward direction)
__device__ __forceinline__ int first_step(int dir, int64_t b0, int64_t B, int L, const int32_t* __restrict__ lo) {
    if (dir == 0) return 0;
    int tmin = L;
    for (int s = 0; s < kSeq; ++s)
        if (b0 + s < B) tmin = min(tmin, max(0, min(L, lo[b0 + s])));
    return tmin;
}

// grid (tiles of 16 sequences, D), block 64 NT
template <int CELL, int NT>
__global__ __launch_bounds__(64 * NT) void rnn_fwd_kernel(int64_t B, int32_t L, int32_t D, int32_t residual, const float* __restrict__ P,
                                                         const float* __restrict__ whh, const float* __restrict__ bhn,
                                                         const float* __restrict__ x0, const float* __restrict__ gate,
                                                         const int32_t* __restrict__ lo, float* __restrict__ y, float* __restrict__ hbuf,
                                                         float* __restrict__ sv) {
    constexpr int G = rnn_gates(CELL), NS = rnn_saved(CELL), Hd = 16 * NT, ld = Hd + 4;
    __shared__ float hs[2][kSeq * ld];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, g = lane >> 4;
    const int dir = blockIdx.y, n0 = 16 * wave, u = n0 + i;
    const int64_t b0 = (int64_t)blockIdx.x * kSeq;
    const size_t PW = (size_t)D * G * Hd, YW = (size_t)D * Hd, SW = (size_t)D * (NS > 0 ? NS : 1) * Hd;

    float4 w[G][NT];                                              // B operand: W_hh[q Hd + u][16 kc + 4 g + e]
#pragma unroll
    for (int q = 0; q < G; ++q)
#pragma unroll
        for (int kc = 0; kc < NT; ++kc)
            w[q][kc] = *reinterpret_cast<const float4*>(whh + ((size_t)dir * G * Hd + q * Hd + u) * Hd + 16 * kc + 4 * g);
    const float bn = CELL == kGru ? bhn[dir * Hd + u] : 0.f;

    size_t row[4];                                                // this lane's sequences 4 g + r (clamped: a lane past B repeats the last)
    bool live[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t b = b0 + 4 * g + r;
        live[r] = b < B;
        row[r] = (size_t)(live[r] ? b : B - 1) * L;
    }
    const int tmin = first_step(dir, b0, B, L, lo), steps = L - tmin, dt = dir ? -1 : 1;
    for (int idx = tid; idx < kSeq * ld; idx += 64 * NT) hs[0][idx] = 0.f;
    __syncthreads();

    float c[4] = {0.f, 0.f, 0.f, 0.f}, hp[4] = {0.f, 0.f, 0.f, 0.f};
    float pn[G][4], gn[4], xn[4];
    int t = dir ? L - 1 : 0;
    if (steps > 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int q = 0; q < G; ++q) pn[q][r] = P[(row[r] + t) * PW + (size_t)dir * G * Hd + q * Hd + u];
            gn[r] = gate[row[r] + t];
            xn[r] = residual ? x0[(row[r] + t) * YW + dir * Hd + u] : 0.f;
        }
    }
    for (int s = 0; s < steps; ++s, t += dt) {
        float pc[G][4], gc[4], xc[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int q = 0; q < G; ++q) pc[q][r] = pn[q][r];
            gc[r] = gn[r];
            xc[r] = xn[r];
        }
        if (s + 1 < steps) {                                      // the next step's rows, under this step's products
            const int t1 = t + dt;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int q = 0; q < G; ++q) pn[q][r] = P[(row[r] + t1) * PW + (size_t)dir * G * Hd + q * Hd + u];
                gn[r] = gate[row[r] + t1];
                xn[r] = residual ? x0[(row[r] + t1) * YW + dir * Hd + u] : 0.f;
            }
        }
        const float* hcur = hs[s & 1];
        float* hnxt = hs[(s & 1) ^ 1];
        f32x4 acc[G];
#pragma unroll
        for (int q = 0; q < G; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < NT; ++kc) {
            const float4 av = *reinterpret_cast<const float4*>(hcur + i * ld + 16 * kc + 4 * g);
#pragma unroll
            for (int q = 0; q < G; ++q) {
                acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, w[q][kc].x, acc[q], 0, 0, 0);
                acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, w[q][kc].y, acc[q], 0, 0, 0);
                acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, w[q][kc].z, acc[q], 0, 0, 0);
                acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, w[q][kc].w, acc[q], 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {                             // sequence 4 g + r, hidden unit u
            float h;
            float* s_out = sv + (row[r] + t) * SW + (size_t)dir * NS * Hd + u;
            if (CELL == kLstm) {
                const float ig = sigm(pc[0][r] + acc[0][r]), fg = sigm(pc[1][r] + acc[1][r]);
                const float gg = tanhf(pc[2][r] + acc[2][r]), og = sigm(pc[3][r] + acc[3][r]);
                c[r] = fg * c[r] + ig * gg;
                h = og * tanhf(c[r]);
                if (live[r]) { s_out[0] = ig; s_out[Hd] = fg; s_out[2 * Hd] = gg; s_out[3 * Hd] = og; s_out[4 * Hd] = c[r]; }
            } else if (CELL == kGru) {
                const float rg = sigm(pc[0][r] + acc[0][r]), zg = sigm(pc[1][r] + acc[1][r]);
                const float hn = acc[2][r] + bn;
                const float ng = tanhf(pc[2][r] + rg * hn);
                h = (1.f - zg) * ng + zg * hp[r];
                if (live[r]) { s_out[0] = rg; s_out[Hd] = zg; s_out[2 * Hd] = ng; s_out[3 * Hd] = hn; }
            } else {
                h = tanhf(pc[0][r] + acc[0][r]);
            }
            hp[r] = h;
            hnxt[(4 * g + r) * ld + u] = h;
            if (live[r]) {
                const size_t o = (row[r] + t) * YW + dir * Hd + u;
                hbuf[o] = h;
                y[o] = (gc[r] != 0.f ? h * gc[r] : 0.f) + xc[r];
            }
        }
        __syncthreads();
    }
    // left of every support of the tile (reverse direction): zeros
    const int nseq = (int)min((int64_t)kSeq, B - b0);
    for (int idx = tid; idx < nseq * tmin * Hd; idx += 64 * NT) {
        const int sq = idx / (tmin * Hd), rem = idx - sq * (tmin * Hd), tt = rem / Hd, uu = rem - tt * Hd;
        const size_t o = ((size_t)(b0 + sq) * L + tt) * YW + dir * Hd + uu;
        y[o] = 0.f;
        hbuf[o] = 0.f;
    }
}

// grid (tiles of 16 sequences, D), block 64 NT
template <int CELL, int NT>
__global__ __launch_bounds__(64 * NT) void rnn_bwd_kernel(int64_t B, int32_t L, int32_t D, const float* __restrict__ dy,
                                                         const float* __restrict__ gate, const int32_t* __restrict__ lo,
                                                         const float* __restrict__ whh, const float* __restrict__ hbuf,
                                                         const float* __restrict__ sv, float* __restrict__ dP, float* __restrict__ dhn) {
    constexpr int G = rnn_gates(CELL), NS = rnn_saved(CELL), Hd = 16 * NT, GH = G * Hd, ld = GH + 4, MC = G * NT;
    __shared__ float ds[2][kSeq * ld];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, g = lane >> 4;
    const int dir = blockIdx.y, n0 = 16 * wave, u = n0 + i;
    const int64_t b0 = (int64_t)blockIdx.x * kSeq;
    const size_t PW = (size_t)D * GH, YW = (size_t)D * Hd, SW = (size_t)D * (NS > 0 ? NS : 1) * Hd;

    float wb[MC][4];                                              // B operand: W_hh[16 mc + 4 g + e][u]
#pragma unroll
    for (int mc = 0; mc < MC; ++mc)
#pragma unroll
        for (int e = 0; e < 4; ++e) wb[mc][e] = whh[((size_t)dir * GH + 16 * mc + 4 * g + e) * Hd + u];

    size_t row[4];
    bool live[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t b = b0 + 4 * g + r;
        live[r] = b < B;
        row[r] = (size_t)(live[r] ? b : B - 1) * L;
    }
    const int tmin = first_step(dir, b0, B, L, lo), steps = L - tmin;
    const int dt = dir ? 1 : -1;                                   // against the forward order
    const int t_first = dir ? L - 1 : 0;                           // the forward order's first step: no state before it
    float dh[4] = {0.f, 0.f, 0.f, 0.f}, dc[4] = {0.f, 0.f, 0.f, 0.f};

    struct Step { float d[4], s[NS > 0 ? NS : 1][4], prev[4]; };  // dy * gate, the saved values, c' (LSTM) / h' (GRU) / h (tanh)
    Step nx;
    auto load = [&](Step& st, int t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const size_t o = (row[r] + t) * YW + dir * Hd + u;
            const float gt = gate[row[r] + t];
            st.d[r] = gt != 0.f ? dy[o] * gt : 0.f;
#pragma unroll
            for (int q = 0; q < NS; ++q) st.s[q][r] = sv[(row[r] + t) * SW + (size_t)dir * NS * Hd + q * Hd + u];
            if (CELL == kLstm) st.prev[r] = t == t_first ? 0.f : sv[(row[r] + t + dt) * SW + (size_t)dir * NS * Hd + 4 * Hd + u];
            else if (CELL == kGru) st.prev[r] = t == t_first ? 0.f : hbuf[(row[r] + t + dt) * YW + dir * Hd + u];
            else st.prev[r] = hbuf[o];
        }
    };
    int t = dir ? tmin : L - 1;
    if (steps > 0) load(nx, t);
    for (int s = 0; s < steps; ++s, t += dt) {
        const Step cu = nx;
        if (s + 1 < steps) load(nx, t + dt);
        float* dcur = ds[s & 1];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float dht = dh[r] + cu.d[r];
            float* p_out = dP + (row[r] + t) * PW + (size_t)dir * GH + u;
            float* l_out = dcur + (4 * g + r) * ld + u;
            if (CELL == kLstm) {
                const float ig = cu.s[0][r], fg = cu.s[1][r], gg = cu.s[2][r], og = cu.s[3][r];
                const float tc = tanhf(cu.s[4][r]);
                const float dcc = dc[r] + dht * og * (1.f - tc * tc);
                const float di = dcc * gg * ig * (1.f - ig), df = dcc * cu.prev[r] * fg * (1.f - fg);
                const float dg = dcc * ig * (1.f - gg * gg), dO = dht * tc * og * (1.f - og);
                dc[r] = dcc * fg;
                dh[r] = 0.f;
                l_out[0] = di; l_out[Hd] = df; l_out[2 * Hd] = dg; l_out[3 * Hd] = dO;
                if (live[r]) { p_out[0] = di; p_out[Hd] = df; p_out[2 * Hd] = dg; p_out[3 * Hd] = dO; }
            } else if (CELL == kGru) {
                const float rg = cu.s[0][r], zg = cu.s[1][r], ng = cu.s[2][r], hn = cu.s[3][r];
                const float dn = dht * (1.f - zg) * (1.f - ng * ng);
                const float dz = dht * (cu.prev[r] - ng) * zg * (1.f - zg);
                const float dr = dn * hn * rg * (1.f - rg), dhid = dn * rg;
                dh[r] = dht * zg;
                l_out[0] = dr; l_out[Hd] = dz; l_out[2 * Hd] = dhid;
                if (live[r]) {
                    p_out[0] = dr; p_out[Hd] = dz; p_out[2 * Hd] = dn;
                    dhn[(row[r] + t) * YW + dir * Hd + u] = dhid;
                }
            } else {
                const float dp = dht * (1.f - cu.prev[r] * cu.prev[r]);
                dh[r] = 0.f;
                l_out[0] = dp;
                if (live[r]) p_out[0] = dp;
            }
        }
        __syncthreads();
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int mc = 0; mc < MC; ++mc) {
            const float4 av = *reinterpret_cast<const float4*>(dcur + i * ld + 16 * mc + 4 * g);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, wb[mc][0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, wb[mc][1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, wb[mc][2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, wb[mc][3], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) dh[r] += acc[r];
    }
    const int nseq = (int)min((int64_t)kSeq, B - b0);             // left of every support of the tile (reverse direction): zeros
    for (int idx = tid; idx < nseq * tmin * GH; idx += 64 * NT) {
        const int sq = idx / (tmin * GH), rem = idx - sq * (tmin * GH), tt = rem / GH, uu = rem - tt * GH;
        dP[((size_t)(b0 + sq) * L + tt) * PW + (size_t)dir * GH + uu] = 0.f;
    }
    if (CELL == kGru)
        for (int idx = tid; idx < nseq * tmin * Hd; idx += 64 * NT) {
            const int sq = idx / (tmin * Hd), rem = idx - sq * (tmin * Hd), tt = rem / Hd, uu = rem - tt * Hd;
            dhn[((size_t)(b0 + sq) * L + tt) * YW + dir * Hd + uu] = 0.f;
        }
}

int check_rnn(const char* what, int64_t B, int32_t L, int32_t Hd, int32_t D, int32_t cell) {
    DN_REQUIRE(B >= 1 && B <= 65535 && L >= 1, "%s: bad sizes (B = %lld, L = %d)", what, (long long)B, L);
    DN_REQUIRE(Hd == 16 || Hd == 32 || Hd == 48 || Hd == 64, "%s: the hidden width per direction must be 16, 32, 48 or 64 (got %d)", what, Hd);
    DN_REQUIRE(D == 1 || D == 2, "%s: 1 or 2 directions (got %d)", what, D);
    DN_REQUIRE(cell >= 0 && cell <= 2, "%s: cell must be 0 (LSTM), 1 (GRU) or 2 (tanh), got %d", what, cell);
    DN_REQUIRE(B * (int64_t)L * D * 5 * Hd < 0x7fffffffLL, "%s: B L D 5 Hd must stay below 2^31 (B = %lld, L = %d)", what, (long long)B, L);
    return DN_OK;
}

#define DN_RNN_DISPATCH(KERNEL, ...)                                                                                              \
    do {                                                                                                                          \
        const dim3 grid((unsigned)dn_cdiv(B, kSeq), (unsigned)D), block(64 * (Hd / 16));                                          \
        switch (cell * 4 + Hd / 16 - 1) {                                                                                         \
            case 0: hipLaunchKernelGGL((KERNEL<kLstm, 1>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__); break;              \
            case 1: hipLaunchKernelGGL((KERNEL<kLstm, 2>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__); break;              \
            case 2: hipLaunchKernelGGL((KERNEL<kLstm, 3>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__); break;              \
            case 3: hipLaunchKernelGGL((KERNEL<kLstm, 4>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__); break;              \
            case 4: hipLaunchKernelGGL((KERNEL<kGru, 1>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__); break;               \
            case 5: hipLaunchKernelGGL((KERNEL<kGru, 2>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__); break;               \
            case 6: hipLaunchKernelGGL((KERNEL<kGru, 3>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__); break;               \
            case 7: hipLaunchKernelGGL((KERNEL<kGru, 4>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__); break;               \
            case 8: hipLaunchKernelGGL((KERNEL<kTanh, 1>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__); break;              \
            case 9: hipLaunchKernelGGL((KERNEL<kTanh, 2>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__); break;              \
            case 10: hipLaunchKernelGGL((KERNEL<kTanh, 3>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__); break;             \
            default: hipLaunchKernelGGL((KERNEL<kTanh, 4>), grid, block, 0, (hipStream_t)stream, __VA_ARGS__); break;             \
        }                                                                                                                         \
    } while (0)

}  // namespace

extern "C" {

int32_t dn_eseq_rnn_saved_per_unit(int32_t cell) { return cell >= 0 && cell <= 2 ? rnn_saved(cell) : -1; }

int dn_eseq_rnn_fwd_f32(int64_t B, int32_t L, int32_t Hd, int32_t D, int32_t cell, int32_t residual, const float* P, const float* whh,
                        const float* bhn, const float* x0, const float* gate, const int32_t* lo, float* y, float* h, float* saved,
                        dn_stream_t stream) {
    if (int rc = check_rnn("dn_eseq_rnn_fwd", B, L, Hd, D, cell)) return rc;
    DN_REQUIRE(P && whh && gate && lo && y && h, "dn_eseq_rnn_fwd: NULL pointer");
    DN_REQUIRE(cell != kGru || bhn, "dn_eseq_rnn_fwd: the GRU needs b_hn");
    DN_REQUIRE(cell == kTanh || saved, "dn_eseq_rnn_fwd: the LSTM and the GRU need the saved buffer");
    DN_REQUIRE(!residual || x0, "dn_eseq_rnn_fwd: the residual needs x0 [B, L, D Hd]");
    DN_RNN_DISPATCH(rnn_fwd_kernel, B, L, D, residual, P, whh, bhn, x0, gate, lo, y, h, saved);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

int dn_eseq_rnn_bwd_f32(int64_t B, int32_t L, int32_t Hd, int32_t D, int32_t cell, const float* dy, const float* gate, const int32_t* lo,
                        const float* whh, const float* h, const float* saved, float* dP, float* dhn, dn_stream_t stream) {
    if (int rc = check_rnn("dn_eseq_rnn_bwd", B, L, Hd, D, cell)) return rc;
    DN_REQUIRE(dy && gate && lo && whh && h && dP, "dn_eseq_rnn_bwd: NULL pointer");
    DN_REQUIRE(cell == kTanh || saved, "dn_eseq_rnn_bwd: the LSTM and the GRU need the saved buffer");
    DN_REQUIRE(cell != kGru || dhn, "dn_eseq_rnn_bwd: the GRU needs dhn [B, L, D Hd]");
    DN_RNN_DISPATCH(rnn_bwd_kernel, B, L, D, dy, gate, lo, whh, h, saved, dP, dhn);
    DN_CHECK_LAUNCH();
    return DN_OK;
}

}  // extern "C"
