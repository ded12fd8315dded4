// dn_mlp_bwd_fused_bf16 (H = 256): one Linear's weight gradient, bias gradient and input gradient in ONE pass over its rows.
//
//   Gm   = mask_in ? keep_or_scale(G, mask_in) : G                       (the activation mask of the layer's output, as bits)
//   gW   = sum_p Gm[p, :]^T A[p, :]          gb = colsum(Gm)             (split-K over the row chunks + wgrad_reduce_kernel)
//   Gn   = mask_out ? keep_or_scale(Gm @ W, mask_out) : Gm @ W           (W [k][n]: nn.Linear.weight as the parameter stores it)
//
// The two-layer MLP's backward is this launch twice (layer 2: G = the incoming gradient, A = the hidden activation, both masks;
// layer 1: G = the Gn of layer 2, A = the MLP's input, no masks) instead of weight gradient 2, the input-gradient chain and weight
// gradient 1: the gradient rows are read once per layer instead of twice and the outer mask is applied once (docs/LAB_NOTES.md,
// round 7).  Arithmetic is the three launches': the same 32-row tiles in the same order, one v_mfma_f32_16x16x32_bf16 per tile and
// accumulator of the 256 x 256 product with the tile's row r in k-slot r, the column sums by the same (row slot, column chunk)
// partition, the input gradient's eight k-steps in order from a zero accumulator, the mask applied to the fp32 sums before the
// one rounding to bf16 -- all five results are bit-identical to rows_wgrad_dma_kernel / rows_wgrad_ls_kernel + rows_chain2_ring_kernel.
//
// One workgroup per chunk (and per CU: 136 KiB of LDS, + a 4 KiB table with masks), 8 self-loading waves at 2 per SIMD (256 registers a wave):
//   * a wave keeps its 128 x 64 part of the weight gradient (128 registers, as in the weight-gradient kernels) AND the weight's
//     32 output columns for the input gradient (64 registers, the ring transform's column order) + 8 for that product's sums,
//     taken one 16-row half of the tile at a time (with both halves' sums and fragments live the allocator spilled);
//   * a tile = 32 rows of G and A by LDS-DMA into a ring of 4 stages (+ the tile's 1 KiB of mask bits each), 3 tiles in flight;
//     the mask is applied to a landed G tile in place one tile AHEAD of its use and the column sums are taken from the registers
//     the masked pieces pass through (rows_wgrad_dma_kernel's scheme), so a tile costs one barrier;
//   * ONE image serves both products: LDS (row r, 16-byte position q) holds global piece q ^ s(r),
//         s(r) = r2 | r0 << 1 | r1 << 2 | (r3 ^ r2) << 3          (r0..r3: bits of r)
//     -- the transposed reads of the weight gradient (ds_read_b64_tr_b16: 32 lanes = rows {8g + q} of one 32-byte column slot)
//     see s(r) >> 1 distinct over the 8 rows of a half-wave, and the row-major reads of the input gradient (ds_read_b128: lane
//     groups {rows 0-3, 12-15 at k-group a; rows 4-11 at k-group a ^ 1}) see s(r) ^ (k-group) distinct over their 16 lanes;
//   * fragment reads are inline asm with hand-counted lgkmcnt waits (dn_rel_ring.hip): the weight gradient's G fragments run
//     two ahead of their MFMAs, the input gradient keeps four k-steps' fragments in flight;
//   * the input-gradient rows leave straight from the accumulators, 16 bytes per lane and row (rows past the chunk's end go to
//     a dump area so that every wave issues the same vector-memory operations per tile: the DMA waits are counted);
//   * the lanes do no 64-bit address arithmetic for a tile wholly inside the chunk: its row DMAs take a wave-uniform base from
//     scalar registers + a constant 32-bit lane offset (glds16_s), its result rows a uniform base + a constant lane offset; only
//     the chunk's last partial tile and the run-ahead tiles behind it take the per-lane path (a wave-uniform branch);
//   * a mask byte becomes the keep mask of its 8 bf16 by ONE ds_read_b128 from a 256-entry table built at kernel start (slope 0:
//     one AND per packed pair, in the input gradient after the rounding -- keep-or-zero commutes with it; slope != 0: the
//     bit-select on the mask pass, the fp32 blend from bit-field extracts on the input gradient).  docs/LAB_NOTES.md, round 9.
// No workgroup waits on another.
#include "dn_common.h"
#include "dn_internal.h"
#include "../../include/dn_hip.h"

namespace {

constexpr int kH = 256;
constexpr int kRowB = 2 * kH;                  // bytes per row
constexpr int kTR = 32;                        // rows per tile
constexpr int kMatB = kTR * kRowB;             // 16 KiB: one operand's tile
constexpr int kBitsB = kTR * (kH / 8);         // 1 KiB: one tile of mask bits
constexpr int kStB = 2 * kMatB + 2 * kBitsB;   // a stage: G rows, A rows, mask_in bits, mask_out bits
constexpr int kNST = 4;                        // ring stages (136 KiB)
constexpr int kTabB = 256 * 16;                // behind the ring: mask byte -> keep mask of its 8 bf16 (4 words), 4 KiB
constexpr int kThreads = 512;
constexpr int kDma = 4, kST = 2;               // per wave and tile: 4 row DMAs (+ a tile's bits on one wave), then 2 result stores
static_assert(kStB % 1024 == 0, "the fragment addressing XORs low bits of stage-relative offsets");

__device__ __attribute__((aligned(16))) uint4 g_mb_zero[64];        // 1 KiB of zeros: what rows past a chunk's end read
__device__ __attribute__((aligned(16))) uint4 g_mb_dump[64 * 8];    // where their results go (1 KiB per wave, never read)

__device__ __forceinline__ int swz(int r) {    // s(r) of the header
    return ((r >> 2) & 1) | ((r & 3) << 1) | ((((r >> 3) ^ (r >> 2)) & 1) << 3);
}

// "tile t has landed" (MASKED: and the G rows + bits of tile t + 1) at the top of iteration t.  Issue order of a wave: tiles 0..2
// (prologue), then per iteration k [tile k + 3][kST stores]; a tile = [2 G pieces][bits, on one wave][2 A pieces].  vmcnt counts all
// of them in issue order; the count below is what was issued BEHIND the awaited pieces (the bits only make a wave's wait stricter).
template <bool MASKED>
__device__ __forceinline__ void mb_wait(int t) {
    if constexpr (MASKED) {                    // behind the G pieces of tile t + 1: its A pieces, then stores and whole tiles
        if (t == 0) { wait_vmcnt<2 + kDma>(); return; }
        if (t == 1) { wait_vmcnt<2 + kDma + kST>(); return; }
        wait_vmcnt<2 + kDma + 2 * kST>();
    } else {                                   // behind tile t: two tiles, and the stores of the iterations since it was issued
        if (t == 0) { wait_vmcnt<2 * kDma>(); return; }
        if (t == 1) { wait_vmcnt<2 * kDma + kST>(); return; }
        if (t == 2) { wait_vmcnt<2 * kDma + 2 * kST>(); return; }
        wait_vmcnt<2 * kDma + 3 * kST>();
    }
}

struct Frag {
    short4v lo, hi;
};
__device__ __forceinline__ bf16x8 frag_val(const Frag& f) {
    const short8v v = {f.lo[0], f.lo[1], f.lo[2], f.lo[3], f.hi[0], f.hi[1], f.hi[2], f.hi[3]};
    return __builtin_bit_cast(bf16x8, v);
}
// rows 8 g + q (lo) and 8 g + 4 + q (hi: s(r + 4) = s(r) ^ 9, so its address is the first XOR 0x90, + 4 rows)
#define DN_MB_TR(fr, ad, ad2)                                                                                          \
    do {                                                                                                              \
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"((fr).lo) : "v"(ad));                                          \
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:2048" : "=v"((fr).hi) : "v"(ad2));                             \
    } while (0)
static_assert(4 * kRowB == 2048, "offset of a transposed fragment's second half");

template <bool MASKED>
__global__ __launch_bounds__(kThreads) void mlp_bwd_fused_kernel(const bf16_t* __restrict__ G, const bf16_t* __restrict__ A,
                                                                 const bf16_t* __restrict__ Wkn,
                                                                 const uint8_t* __restrict__ bits_in,
                                                                 const uint8_t* __restrict__ bits_out, int32_t N,
                                                                 const Chunk* __restrict__ chunks, float* __restrict__ partial,
                                                                 float* __restrict__ colsum_partial, bf16_t* __restrict__ Gn,
                                                                 float slope) {
    __shared__ __attribute__((aligned(1024))) char lds[kNST * kStB + (MASKED ? kTabB : 0)];
    const unsigned lds_base = lds_addr(lds);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const Chunk ch = chunks[blockIdx.x];
    const int32_t cbeg = max(ch.beg, 0), cend = min(ch.end, N);           // (a table never leaves [0, N): no row outside is touched anyway)
    const int ntiles = cend > cbeg ? (cend - cbeg + kTR - 1) / kTR : 0;
    if (ntiles <= 0) {                                                    // (chunk tables hold no empty chunks; guard anyway)
        for (int i = tid; i < kH * kH; i += kThreads) partial[(size_t)blockIdx.x * kH * kH + i] = 0.f;
        if (tid < kH) colsum_partial[(size_t)blockIdx.x * kH + tid] = 0.f;
        return;
    }

    // ---- the weight's 32 output columns of this wave for Gn = Gm @ W, in the ring transform's column order (A row i of MFMA tile
    //      n <-> column 32 wave + 8 (i >> 2) + 4 n + (i & 3)): a lane ends up with 8 consecutive columns of a row
    bf16x8 wf[8][2];
    dn_load_w_kn32<8>(Wkn, kH, 32 * wave, lane, lds + wave * 2048, wf);  // (wave-private scratch inside the idle ring)
    wait_vmcnt<0>();                                                      // no ordinary load may be pending once the DMAs start
    if constexpr (MASKED) {
        // the keep-mask table: word i of entry b = 0xffff where bit 2 i of b is set | 0xffff0000 where bit 2 i + 1 is (the two
        // bf16 of a packed pair); a mask byte costs one ds_read_b128 instead of eight bit-field extracts and twelve logic ops
        if (tid < 256) {
            u32x4 e;
#pragma unroll
            for (int i = 0; i < 4; ++i) e[i] = ((tid >> (2 * i)) & 1 ? 0xffffu : 0u) | ((tid >> (2 * i + 1)) & 1 ? 0xffff0000u : 0u);
            *reinterpret_cast<u32x4*>(lds + kNST * kStB + tid * 16) = e;
        }
    }
#pragma unroll
    for (int ks = 0; ks < 8; ++ks)
#pragma unroll
        for (int n = 0; n < 2; ++n) asm volatile("" : "+v"(wf[ks][n]));
    __syncthreads();                                                      // every wave is done with its scratch: the ring may fill

    // ---- DMA side: rows 4 w .. 4 w + 3 of both operands of a tile are this wave's (two wave-instructions of 2 rows each)
    // (The accumulators + weights leave 48 registers.  Four 32-bit lane constants live across the loop -- dma_off, mask_byte, off0,
    //  st_off, each pinned by an empty asm; the fragment addresses of the weight gradient and everything the partial-tile path
    //  needs are derived anew from `fresh()` in their phase: hoisted they would be ~40 more registers live across the loop.)
    auto fresh = [&]() __attribute__((always_inline)) {
        int l = lane;
        asm volatile("" : "+v"(l));
        return l;
    };
    const char* zero = reinterpret_cast<const char*>(g_mb_zero);
    // A tile wholly inside the chunk is 32 consecutive rows: its source is ONE wave-uniform 64-bit base (in SGPRs, from scalar
    // arithmetic) + a lane offset that never changes -- row-in-pair x 512 + the swizzled piece (the second pair of rows: s(r + 2) =
    // s(r) ^ 4, the same offset XOR 64); 16 x lane for a tile of bits.  One register lives across the loop instead of five 64-bit
    // addresses worked out per tile.  The chunk's last partial tile and the run-ahead tiles behind it take the per-lane path below
    // (a wave-uniform branch); both paths issue the same vector-memory operations in the same order -- mb_wait counts them.
    const int nfull = (cend - cbeg) / kTR;                                // tiles wholly inside the chunk (32-bit: a scalar compare)
    unsigned dma_off = (unsigned)((lane >> 5) * kRowB + (((lane & 31) ^ swz(4 * wave + (lane >> 5))) << 4));
    asm volatile("" : "+v"(dma_off));
    auto issue = [&](int T) __attribute__((always_inline)) {
        const unsigned st = lds_base + (unsigned)(T % kNST) * kStB;
        const int64_t r0 = (int64_t)cbeg + (int64_t)T * kTR;
        if (T < nfull) {
            const uint64_t rowoff = (uint64_t)(r0 + 4 * wave) * kRowB;
            const uint64_t gb = (uint64_t)(uintptr_t)G + rowoff, ab = (uint64_t)(uintptr_t)A + rowoff;
            const unsigned off1 = dma_off ^ 64u, sw = st + (unsigned)(4 * wave) * kRowB;
            glds16_s(gb, dma_off, sw);
            glds16_s(gb + 2 * kRowB, off1, sw + 2 * kRowB);
            if constexpr (MASKED) {
                const uint64_t boff = (uint64_t)r0 * (kH / 8);
                const unsigned lo = (unsigned)lane << 4;
                if (wave == (T & 7)) glds16_s((uint64_t)(uintptr_t)bits_in + boff, lo, st + 2 * kMatB);
                if (wave == ((T + 4) & 7)) glds16_s((uint64_t)(uintptr_t)bits_out + boff, lo, st + 2 * kMatB + kBitsB);
            }
            glds16_s(ab, dma_off, sw + (unsigned)kMatB);
            glds16_s(ab + 2 * kRowB, off1, sw + (unsigned)kMatB + 2 * kRowB);
            return;
        }
        const int ln = fresh(), rin = ln >> 5, cpos = ln & 31;
        uint64_t pas[2];
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int rl = 4 * wave + 2 * jj + rin;                       // row of the tile this lane fills
            const uint64_t gch = (uint64_t)((cpos ^ swz(rl)) << 4);       // source byte offset inside the row
            const int64_t p = r0 + rl;
            const bool ok = p < (int64_t)cend;                            // rows (and whole tiles) past the chunk's end read zeros
            const uint64_t off = (uint64_t)p * kRowB + gch, z = (uint64_t)(uintptr_t)zero + gch;
            const uint64_t pg = ok ? (uint64_t)(uintptr_t)G + off : z;
            pas[jj] = ok ? (uint64_t)(uintptr_t)A + off : z;
            glds16(reinterpret_cast<const char*>(pg), st + (unsigned)(4 * wave + 2 * jj) * kRowB);   // lane l lands at + 16 l
        }
        if constexpr (MASKED) {                                           // the tile's 1 KiB of mask_in / mask_out bits: one full-width DMA each
            const int64_t p = r0 + (ln >> 1);
            const size_t boff = (size_t)p * (kH / 8) + (size_t)(ln & 1) * 16;
            const bool ok = p < (int64_t)cend;
            if (wave == (T & 7)) glds16(ok ? reinterpret_cast<const char*>(bits_in) + boff : zero + ln * 16, st + 2 * kMatB);
            if (wave == ((T + 4) & 7))
                glds16(ok ? reinterpret_cast<const char*>(bits_out) + boff : zero + ln * 16, st + 2 * kMatB + kBitsB);
        }
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
            glds16(reinterpret_cast<const char*>(pas[jj]), st + (unsigned)kMatB + (unsigned)(4 * wave + 2 * jj) * kRowB);
    };

    // ---- mask pass / column sums: thread (mrow, mq) owns position mq of rows mrow and mrow + 16 of every G tile = column chunk
    //      mchunk (s(r + 16) = s(r)); per (row slot, chunk) the sum runs over the tiles in order, rows mrow then mrow + 16 -- the
    //      partition and order of the weight-gradient kernels
    float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    auto add_cs = [&](const uint4& v) __attribute__((always_inline)) {
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            cs[2 * i] += __uint_as_float(w[i] << 16);
            cs[2 * i + 1] += __uint_as_float(w[i] & 0xffff0000u);
        }
    };
    unsigned mask_byte = 0;                                               // my byte of a tile's mask_in bits (row mrow; + 512: row mrow + 16)
    if constexpr (MASKED) {
        mask_byte = (unsigned)((2 * wave + (lane >> 5)) * (kH / 8) + ((lane & 31) ^ swz(2 * wave + (lane >> 5))));
        asm volatile("" : "+v"(mask_byte));
    }
    auto mask_tile = [&](int T) __attribute__((always_inline)) {          // the G rows of tile T in place (+ their column sums)
        // (row mrow = 2 wave + (lane >> 5), position lane & 31: byte 1024 wave + 16 lane of the tile; mask_byte: its byte of bits)
        char* sT = lds + (T % kNST) * kStB;
        const uint8_t* sB = reinterpret_cast<const uint8_t*>(sT + 2 * kMatB) + mask_byte;
        const u32x4* tab = reinterpret_cast<const u32x4*>(lds + kNST * kStB);
        u32x4* pp[2];
        u32x4 v[2], mk[2];
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            pp[jj] = reinterpret_cast<u32x4*>(sT + wave * 1024 + 16 * jj * kRowB + (lane << 4));
            mk[jj] = tab[sB[16 * jj * (kH / 8)]];
            v[jj] = *pp[jj];
        }
        // keep where the bit is set, x slope (0: zero) elsewhere = dn_keep_or_scale_bits, branch-free: the byte's word masks
        // from the table and one AND (slope 0) or one bit-select
        if (slope == 0.f) {
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) v[jj] &= mk[jj];
        } else {
#pragma unroll
            for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const uint32_t alt =
                        pack_bf16x2(__uint_as_float(v[jj][i] << 16) * slope, __uint_as_float(v[jj][i] & 0xffff0000u) * slope);
                    v[jj][i] = (v[jj][i] & mk[jj][i]) | (alt & ~mk[jj][i]);
                }
        }
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            *pp[jj] = v[jj];
            add_cs(make_uint4(v[jj][0], v[jj][1], v[jj][2], v[jj][3]));
        }
    };
    auto colsum_tile = [&](int T) __attribute__((always_inline)) {        // (unmasked: the column sums of tile T as it lies)
        const int ln = fresh(), mrow = 2 * wave + (ln >> 5), mq = ln & 31;
        const char* sT = lds + (T % kNST) * kStB;
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) add_cs(*reinterpret_cast<const uint4*>(sT + (mrow + 16 * jj) * kRowB + mq * 16));
    };

    // ---- weight gradient: wave (wm, wn) owns rows 128 wm .. + 127 (columns of G), columns 64 wn .. + 63 (columns of A)
    const int wm = wave >> 2, wn = wave & 3;
    f32x4 acc[8][4];
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    // my 8 bytes of column slot S (16 columns = pieces 2 S, 2 S + 1) of row fR = 8 fg + fq: piece (2 S + (fp >> 1)) ^ s(fR), + 8 (fp & 1)
    // bytes; S = 8 wm + m / 4 wn + n: the address of slot S0 + m is the address of slot S0 XOR m << 5
    auto tr_lane = [&](int ln, int piece0) __attribute__((always_inline)) {
        const int fg = ln >> 4, fq = (ln & 15) >> 2, fp = ln & 3, fR = 8 * fg + fq;
        return lds_base + (unsigned)(fR * kRowB + (((piece0 + (fp >> 1)) ^ swz(fR)) << 4) + 8 * (fp & 1));
    };

    // ---- input gradient: rows j and 16 + j of a tile, my 32 columns; fragment of k-step ks = piece (4 ks + g) ^ s(j) of row j:
    //      (stage + off0) ^ (ks & 3) << 6, + 256 for ks >= 4
    f32x4 dacc[2];
    bf16x8 xf[4];
    // (lane constants of this phase kept across the loop: the fragment address inside a stage, and my 16 bytes of row j of Gn)
    unsigned off0 = lds_base + (unsigned)((lane & 15) * kRowB + (((lane >> 4) ^ swz(lane & 15)) << 4));
    unsigned st_off = (unsigned)((lane & 15) * kRowB + (32 * wave + 8 * (lane >> 4)) * 2);
    asm volatile("" : "+v"(off0), "+v"(st_off));

    // (HH: rows j of the tile's first or second 16 rows -- the sums of one half at a time: 8 registers, 4 per fragment)
#define DN_MB_FETCH(SLOT, KS, HH)                                                                                     \
    {                                                                                                                 \
        const unsigned a_ = (sg + off0) ^ (unsigned)(((KS) & 3) << 6);                                                \
        if ((HH) == 0) {                                                                                              \
            if ((KS) < 4) { DN_DS_READ128(xf[SLOT], a_, 0); } else { DN_DS_READ128(xf[SLOT], a_, 256); }              \
        } else {                                                                                                      \
            if ((KS) < 4) { DN_DS_READ128(xf[SLOT], a_, 8192); } else { DN_DS_READ128(xf[SLOT], a_, 8448); }          \
        }                                                                                                             \
    }
#define DN_MB_MFMA2(SLOT, KS)                                                                                         \
    _Pragma("unroll") for (int n = 0; n < 2; ++n)                                                                      \
        dacc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[KS][n], xf[SLOT], dacc[n], 0, 0, 0);                    \
    __builtin_amdgcn_sched_barrier(0);
#define DN_MB_KSTEP(SLOT, KS, CNT)                                                                                    \
    asm volatile("s_waitcnt lgkmcnt(" #CNT ")" : "+v"(xf[SLOT]));                                                     \
    DN_MB_MFMA2(SLOT, KS)
    // Gn's sums of one half: eight k-steps in order, four fragments in flight (reads in the queue behind the one a k-step waits
    // for: 3, ..., then 2, 1, 0); then the rows leave straight from the accumulators: mask_out on the fp32 sums (keep where the
    // bit is set, x slope -- 0: zero -- elsewhere, as rows_chain2_ring_kernel's), one rounding to bf16, one 16-byte store
    // MASKED: the half's byte of mask_out bits is requested AHEAD of the fragments (it has landed with the first of them) and its
    // table entry behind k-step 0 -- one more read in the queue behind the fragments of k-steps 1-3 (count 4), landed with the
    // fragment of k-step 4.  Slope 0: keep-or-zero commutes with the one rounding, so the packed pairs are ANDed with the entry.
#define DN_MB_KSTEP_M(SLOT, KS, CNT_MASKED, CNT_PLAIN)                                                                \
    if constexpr (MASKED) { DN_MB_KSTEP(SLOT, KS, CNT_MASKED) } else { DN_MB_KSTEP(SLOT, KS, CNT_PLAIN) }
#define DN_MB_DGRAD_HALF(HH)                                                                                          \
    {                                                                                                                 \
        uint32_t kb = 0;                                                                                              \
        u32x4 km = {0u, 0u, 0u, 0u};                                                                                  \
        if constexpr (MASKED) {                                                                                       \
            if ((HH) == 0) asm volatile("ds_read_u8 %0, %1" : "=v"(kb) : "v"(bitaddr));                               \
            else asm volatile("ds_read_u8 %0, %1 offset:512" : "=v"(kb) : "v"(bitaddr));                              \
        }                                                                                                             \
        DN_MB_FETCH(0, 0, HH) DN_MB_FETCH(1, 1, HH) DN_MB_FETCH(2, 2, HH) DN_MB_FETCH(3, 3, HH)                       \
        __builtin_amdgcn_sched_barrier(0);                                                                            \
        if constexpr (MASKED) asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(xf[0]), "+v"(kb));                           \
        else asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(xf[0]));                                                      \
        _Pragma("unroll") for (int n = 0; n < 2; ++n)                                                                  \
            dacc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[0][n], xf[0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);  \
        __builtin_amdgcn_sched_barrier(0);                                                                            \
        if constexpr (MASKED) {                                                                                       \
            const unsigned ta_ = lds_base + (unsigned)(kNST * kStB) + (kb << 4);                                      \
            DN_DS_READ128(km, ta_, 0);                                                                                \
        }                                                                                                             \
        DN_MB_FETCH(0, 4, HH) __builtin_amdgcn_sched_barrier(0);                                                      \
        DN_MB_KSTEP_M(1, 1, 4, 3) DN_MB_FETCH(1, 5, HH) __builtin_amdgcn_sched_barrier(0);                            \
        DN_MB_KSTEP_M(2, 2, 4, 3) DN_MB_FETCH(2, 6, HH) __builtin_amdgcn_sched_barrier(0);                            \
        DN_MB_KSTEP_M(3, 3, 4, 3) DN_MB_FETCH(3, 7, HH) __builtin_amdgcn_sched_barrier(0);                            \
        DN_MB_KSTEP(0, 4, 3)                                                                                          \
        DN_MB_KSTEP(1, 5, 2)                                                                                          \
        DN_MB_KSTEP(2, 6, 1)                                                                                          \
        DN_MB_KSTEP(3, 7, 0)                                                                                          \
        if constexpr (MASKED) asm volatile("" : "+v"(km));                                                            \
        float v[8];                                                                                                   \
        _Pragma("unroll") for (int n = 0; n < 2; ++n)                                                                  \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) v[4 * n + i] = dacc[n][i];                                       \
        u32x4 o;                                                                                                      \
        if (MASKED && slope != 0.f) {                                                                                 \
            _Pragma("unroll") for (int i = 0; i < 8; ++i) {                                                            \
                const uint32_t mk = (uint32_t)__builtin_amdgcn_sbfe((int32_t)kb, i, 1);                               \
                v[i] = __uint_as_float((__float_as_uint(v[i]) & mk) | (__float_as_uint(v[i] * slope) & ~mk));         \
            }                                                                                                         \
            _Pragma("unroll") for (int i = 0; i < 4; ++i) o[i] = pack_bf16x2(v[2 * i], v[2 * i + 1]);                  \
        } else {                                                                                                      \
            _Pragma("unroll") for (int i = 0; i < 4; ++i) o[i] = pack_bf16x2(v[2 * i], v[2 * i + 1]);                  \
            if constexpr (MASKED) o &= km;                                                                            \
        }                                                                                                             \
        /* (a store is always issued: the DMA waits count it) */                                                      \
        if (full_tile) {                                                                                              \
            char* dst = reinterpret_cast<char*>(Gn) + (uint64_t)(rt0 + 16 * (HH)) * kRowB + st_off;                   \
            __builtin_nontemporal_store(o, reinterpret_cast<u32x4*>(dst));                                            \
        } else {                                                                                                      \
            const int64_t p = rt0 + 16 * (HH) + j;                                                                    \
            char* dst = p < (int64_t)cend ? reinterpret_cast<char*>(Gn) + (uint64_t)p * kRowB + ycol : dump;          \
            __builtin_nontemporal_store(o, reinterpret_cast<u32x4*>(dst));                                            \
        }                                                                                                             \
        __builtin_amdgcn_sched_barrier(0);                                                                            \
    }

#pragma unroll 1
    for (int T = 0; T < kNST - 1; ++T) issue(T);
    if constexpr (MASKED) {
        wait_vmcnt<2 + 2 * kDma>();                                       // my G pieces (and the bits) of tile 0 have landed
        __builtin_amdgcn_s_barrier();
        mask_tile(0);
    }

#pragma unroll 1
    for (int t = 0; t < ntiles; ++t) {
        mb_wait<MASKED>(t);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                 // my LDS reads / mask writes of the last interval are done
        __builtin_amdgcn_s_barrier();                                      // everyone's are, and everyone's pieces have landed
        issue(t + kNST - 1);                                               // into the stage tile t - 1 used
        const unsigned sg = (unsigned)(t % kNST) * kStB;
        __builtin_amdgcn_sched_barrier(0);
        {
            // a tile's four A-operand fragments and the first two of G go out behind the barrier; row m of the MFMAs waits for
            // ITS fragment only (behind it in the queue: the next fragment = 2 reads) and requests the fragment two rows on
            const int ln = fresh();
            const unsigned va = tr_lane(ln, 16 * wm) + sg, vb = tr_lane(ln, 8 * wn) + (unsigned)kMatB + sg, va2 = va ^ 0x90u, vb2 = vb ^ 0x90u;
            Frag fb[4], fa[2];
#pragma unroll
            for (int n = 0; n < 4; ++n) DN_MB_TR(fb[n], vb ^ (unsigned)(n << 5), vb2 ^ (unsigned)(n << 5));
#pragma unroll
            for (int m = 0; m < 2; ++m) DN_MB_TR(fa[m], va ^ (unsigned)(m << 5), va2 ^ (unsigned)(m << 5));
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                Frag& f = fa[m & 1];
                if (m == 0)
                    asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(f.lo), "+v"(f.hi), "+v"(fb[0].lo), "+v"(fb[0].hi), "+v"(fb[1].lo), "+v"(fb[1].hi),
                                 "+v"(fb[2].lo), "+v"(fb[2].hi), "+v"(fb[3].lo), "+v"(fb[3].hi));
                else if (m < 7) asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(f.lo), "+v"(f.hi));
                else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f.lo), "+v"(f.hi));
                const bf16x8 av = frag_val(f);
#pragma unroll
                for (int n = 0; n < 4; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, frag_val(fb[n]), acc[m][n], 0, 0, 0);
                if (m + 2 < 8) DN_MB_TR(f, va ^ (unsigned)((m + 2) << 5), va2 ^ (unsigned)((m + 2) << 5));
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        {
            // a tile wholly inside the chunk stores to a uniform base + st_off; the last partial tile per lane, rows past the end
            // to the dump slot (a wave-uniform branch, one store either way)
            const int ln = fresh(), j = ln & 15, g = ln >> 4;
            char* dump = reinterpret_cast<char*>(g_mb_dump) + wave * 1024 + ln * 16;
            const unsigned ycol = (unsigned)(32 * wave + 8 * g) * 2;      // my 16 bytes of a row of Gn
            const int64_t rt0 = (int64_t)cbeg + (int64_t)t * kTR;
            const bool full_tile = t < nfull;
            // my byte of the tile's mask_out bits: row j (offset 512: row 16 + j), byte 4 wave + g = st_off / 16
            const unsigned bitaddr = lds_base + sg + (unsigned)(2 * kMatB + kBitsB) + (st_off >> 4);
            DN_MB_DGRAD_HALF(0)
            DN_MB_DGRAD_HALF(1)
        }
        if constexpr (MASKED) mask_tile(t + 1);                            // (a zero tile past the end stays zero)
        else colsum_tile(t);
    }
#undef DN_MB_DGRAD_HALF
#undef DN_MB_MFMA2
#undef DN_MB_KSTEP
#undef DN_MB_FETCH
    wait_vmcnt<0>();                                                       // the zero tiles still in flight: nothing may land later
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    // C layout of mfma 16x16: col = lane & 15, row = (lane >> 4) * 4 + i
    float* out = partial + (size_t)blockIdx.x * kH * kH;
    const int k0 = wm * (kH / 2), n0 = wn * (kH / 4);
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = k0 + m * 16 + (lane >> 4) * 4 + i, c = n0 + n * 16 + (lane & 15);
                out[(size_t)k * kH + c] = acc[m][n][i];
            }
    const int mrow = tid >> 5, mchunk = (tid & 31) ^ swz(mrow);
    float* red = reinterpret_cast<float*>(lds);                            // 16 row slots x 256 columns, folded in slot order
#pragma unroll
    for (int i = 0; i < 8; ++i) red[mrow * kH + mchunk * 8 + i] = cs[i];
    __syncthreads();
    if (tid < kH) {
        float sum = 0.f;
        for (int sl = 0; sl < kThreads / 32; ++sl) sum += red[sl * kH + tid];
        colsum_partial[(size_t)blockIdx.x * kH + tid] = sum;
    }
}
#undef DN_MB_TR

}  // namespace

extern "C" int dn_mlp_bwd_fused_bf16(const void* G, const void* A, const void* W_kn, const void* mask_in_bits,
                                     const void* mask_out_bits, int64_t N, int32_t H, const int32_t* chunks, int64_t num_chunks,
                                     const int32_t* chunk_ptr, void* out_w, int32_t out_is_f32, float* out_colsum,
                                     void* out_colsum_lp, void* g_next, float act_slope, void* workspace, size_t workspace_bytes,
                                     dn_stream_t stream) {
    DN_REQUIRE(H == 256, "dn_mlp_bwd_fused: unsupported width %d (256 only)", H);
    DN_REQUIRE(N >= 0 && N < 0x7fffffffLL && num_chunks >= 0, "dn_mlp_bwd_fused: bad sizes");
    DN_REQUIRE((mask_in_bits == nullptr) == (mask_out_bits == nullptr), "dn_mlp_bwd_fused: both masks or neither");
    DN_REQUIRE(out_w && chunk_ptr && out_colsum, "dn_mlp_bwd_fused: NULL pointer");
    DN_REQUIRE(num_chunks == 0 || (G && A && W_kn && chunks && workspace && g_next), "dn_mlp_bwd_fused: NULL pointer");
    DN_REQUIRE(workspace_bytes >= (size_t)num_chunks * ((size_t)H * H + H) * sizeof(float), "dn_mlp_bwd_fused: workspace too small");
    DN_REQUIRE((reinterpret_cast<uintptr_t>(G) | reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(W_kn) |
                reinterpret_cast<uintptr_t>(mask_in_bits) | reinterpret_cast<uintptr_t>(mask_out_bits) |
                reinterpret_cast<uintptr_t>(g_next) | reinterpret_cast<uintptr_t>(workspace) |
                reinterpret_cast<uintptr_t>(out_colsum)) % 16 == 0, "dn_mlp_bwd_fused: unaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    if (num_chunks > 0) {
        float* csp = ws + (size_t)num_chunks * H * H;
        const Chunk* ch = reinterpret_cast<const Chunk*>(chunks);
        if (mask_in_bits)
            hipLaunchKernelGGL((mlp_bwd_fused_kernel<true>), dim3((unsigned)num_chunks), dim3(kThreads), 0, st, (const bf16_t*)G,
                               (const bf16_t*)A, (const bf16_t*)W_kn, (const uint8_t*)mask_in_bits, (const uint8_t*)mask_out_bits,
                               (int32_t)N, ch, ws, csp, (bf16_t*)g_next, act_slope);
        else
            hipLaunchKernelGGL((mlp_bwd_fused_kernel<false>), dim3((unsigned)num_chunks), dim3(kThreads), 0, st, (const bf16_t*)G,
                               (const bf16_t*)A, (const bf16_t*)W_kn, (const uint8_t*)nullptr, (const uint8_t*)nullptr, (int32_t)N, ch,
                               ws, csp, (bf16_t*)g_next, act_slope);
        DN_CHECK_LAUNCH();
    }
    return dn_internal::launch_wgrad_reduce(ws, chunk_ptr, num_chunks, H, 1, out_w, out_is_f32, true, out_colsum, out_colsum_lp, st);
}
