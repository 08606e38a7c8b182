// gemm_skinny.hip -- the decode step's projections: one weight-streaming kernel, three weight streams (bf16, e4m3 codes with a row scale, and MXFP4:
// e2m1 codes with an E8M0 scale per 32-deep block).
#include "common.h"
#include "fp8_code.h"

#include <math.h>

#include <type_traits>

// ---------------------------------------------------------------------------------------
// Skinny GEMM for the decode step: out[M, N] = x[M, K] . w[N, K]^T with M <= 128 rows (one token per clip) -- the weight
// matrix is read exactly once, so the kernel is an HBM stream of W with the matrix cores idling behind it, and what bounds it
// is the number of weight bytes a CU keeps IN FLIGHT (rate = bytes in flight / memory latency).
//   work      one workgroup per (128-row weight tile, K split): K is split where N / 128 tiles alone would leave most of the 256
//             CUs without a stream (N = 4096: 32 tiles).  Unsplit tiles round and store straight to `out`; split tiles leave an
//             fp32 fragment each and a second small launch adds a tile's fragments in split order and rounds once (deterministic:
//             no atomics.  Adding them in the last-arriving workgroup of the same launch was built in round 3 and measured 2-5x
//             SLOWER: the device-scope release / acquire fences it needs write back and invalidate the L2 under the stream).
//   fragments THE LAYOUT CONTRACT of split calls: part[(tile b * S + split) * M + row][128] fp32, S = gridDim.y > 1.  Its readers are
//             gemm_skinny_reduce_kernel here and, under defer_reduce, parts_sum in llm.hip (vtgb_llm_rmsnorm_parts, vtgb_llm_rope_cache_parts*).
//   tile      128 (all of M) x 128 weight rows; 4 multiplying waves of 128 x 32 (acc[2][8] of v_mfma_f32_16x16x32_bf16) + 2
//             loader waves.
//   weights   straight from global memory into the multiplying waves' REGISTERS in MFMA fragment layout (a wave owns its 32
//             weight rows, nobody else reads them: no LDS): WS::D k-tiles of WS::LOADS 16-byte loads per lane ahead -- bf16: 8 x 4 KiB
//             per wave, fp8: 16 x 2 KiB, 128 KiB per workgroup either way (rounds 1-2 staged them through a 7-slot LDS ring: 96 KiB
//             in flight, and LDS had to hold the activations too).
//             k-tiles past the end of the split are requested OUT OF RANGE of the descriptor (zeros, no memory traffic), so the
//             counted wait is the same constant on every step.
//   x         L2-resident; the two loader waves stage it with buffer_load ... lds (LDS-DMA) into a 9-slot ring, 7 k-tiles ahead.
//             They have their own vmcnt: a wave that mixed this shallow stream with the deep weight stream would drain the
//             weights every k-tile (vmcnt completes in order per wave).  One barrier per k-tile.
//   x rows    XB = the 16-row x blocks the kernel stages, reads and multiplies (1, 2, 4 or 8; rows >= 16 XB must be >= M).
// x rows beyond M are clamped duplicates (never stored); weight rows beyond N read as zeros (descriptor range / packed zeros).
//
// The weight stream WS is what differs between the two entry points (SkinnyBf16, SkinnyFp8 below): how many loads make a k-tile and how
// many k-tiles are in flight, where the loads point, how a loaded register becomes an MFMA operand, and whether the epilogue scales.
//
// fp8 (opt-in: decode_weights="fp8").  A weight row n is stored as OCP e4m3 codes q[n, :] and one power-of-two scale 2^e[n] (e = the
// smallest integer with amax[n] 2^-e <= 448), so q * scale is exactly a bf16 number and "the fp8 model" is an ordinary bf16 model whose
// projection weights are dq = q * scale.  The codes are widened to bf16 in registers (v_cvt_pk_f32_fp8 is exact; the bf16 is the upper
// half of the fp32) and multiplied by the SAME v_mfma_f32_16x16x32_bf16 in the same k order; the scale is applied to the fp32 accumulators
// before a fragment leaves the registers (a power of two: exact), so fragments, the reduce launch and the deferred consumers see what the
// bf16 stream would have produced from dq -- bit for bit.
//
// mxfp4 (opt-in: decode_weights="mxfp4"; OCP Microscaling v1.0, the definition is ops.quantize_mxfp4_rows).  Every 32 consecutive weights of a row
// share one E8M0 scale 2^e (e = floor(log2(amax)) - 2, clamped to [-120, 125]) and are stored as e2m1 codes, two per byte.  code * 2^e is exactly
// a normal bf16 number, so here too "the mxfp4 model" is an ordinary bf16 model with the weights dq = code * 2^e.  A lane's 8-deep k chunk of a
// 32-deep MFMA half lies inside one block: v_cvt_scalef32_pk_bf16_fp4 widens a byte of two codes under the block's scale straight to the bf16
// pair (exact), the operands feed the SAME v_mfma_f32_16x16x32_bf16 in the same k order and nothing is left for the epilogue -- fragments and
// outputs are the bf16 stream's on dq, bit for bit.
// ---------------------------------------------------------------------------------------
constexpr int SK_BN = 128, SK_BK = 64, SK_TILE = 128 * 128;   // SK_TILE: bytes of one bf16 operand tile (128 rows x 64 bf16)
constexpr int SK8_TILE = 128 * 64;                             // bytes of one fp8 weight block (128 rows x 64 codes)
constexpr int SK4_CODES = 128 * 32, SK4_TILE = SK4_CODES + 256; // bytes of one mxfp4 weight block: 128 rows x 64 codes, then 128 rows x 2 scale bytes
constexpr int SK_XSLOTS = 9, SK_XD = 8;                        // x ring (LDS) and how far ahead the loaders run
constexpr int SK_THREADS = 384;
typedef __attribute__((address_space(3))) void* sk_lptr_t;
typedef __attribute__((ext_vector_type(4))) int sk_i32x4;

__device__ __forceinline__ int sk_swz(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }

// s_waitcnt vmcnt(P n), n = 0..6: a loader wave has P loads per k-tile in flight (P <= 8; vmcnt is 6 bits: [3:0] and [15:14]); the other
// counters are left alone
template <int P>
__device__ __forceinline__ void sk_wait_stages(int n) {
#define SK_VM(v) __builtin_amdgcn_s_waitcnt(0x0F70 | ((v) & 15) | (((v) >> 4) << 14))
    if (n >= 6) SK_VM(P * 6);
    else if (n == 5) SK_VM(P * 5);
    else if (n == 4) SK_VM(P * 4);
    else if (n == 3) SK_VM(P * 3);
    else if (n == 2) SK_VM(P * 2);
    else if (n == 1) SK_VM(P * 1);
    else SK_VM(0);
#undef SK_VM
}

// 8 e4m3 codes (two dwords) -> 8 bf16, exact
__device__ __forceinline__ bf16x8 sk8_widen(int lo, int hi) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((ext_vector_type(2))) float f32x2_;
    const f32x2_ a = __builtin_amdgcn_cvt_pk_f32_fp8(lo, false), b = __builtin_amdgcn_cvt_pk_f32_fp8(lo, true);
    const f32x2_ c = __builtin_amdgcn_cvt_pk_f32_fp8(hi, false), d = __builtin_amdgcn_cvt_pk_f32_fp8(hi, true);
    // (upper halves of two fp32: bytes 2, 3 of the second operand, then bytes 2, 3 of the first)
    const sk_i32x4 p = {(int)__builtin_amdgcn_perm(__float_as_uint(a[1]), __float_as_uint(a[0]), 0x07060302u),
                        (int)__builtin_amdgcn_perm(__float_as_uint(b[1]), __float_as_uint(b[0]), 0x07060302u),
                        (int)__builtin_amdgcn_perm(__float_as_uint(c[1]), __float_as_uint(c[0]), 0x07060302u),
                        (int)__builtin_amdgcn_perm(__float_as_uint(d[1]), __float_as_uint(d[0]), 0x07060302u)};
    return __builtin_bit_cast(bf16x8, p);
#else
    return bf16x8{};
#endif
}

// 8 e2m1 codes (one dword, the lower k in the low nibble) under the E8M0 scale byte of their block -> 8 bf16, exact.  The scale operand is the
// fp32 2^e: the byte in the exponent field (bytes 7 .. 252 in a packed stream; 0 -- an out-of-range load -- is 0.0 and meets zero codes)
__device__ __forceinline__ bf16x8 sk4_widen(int codes, unsigned e8m0) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_;
    const float scale = __uint_as_float(e8m0 << 23);
    const bf16x2_ a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4((unsigned)codes, scale, 0), b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4((unsigned)codes, scale, 1);
    const bf16x2_ c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4((unsigned)codes, scale, 2), d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4((unsigned)codes, scale, 3);
    const sk_i32x4 p = {__builtin_bit_cast(int, a), __builtin_bit_cast(int, b), __builtin_bit_cast(int, c), __builtin_bit_cast(int, d)};
    return __builtin_bit_cast(bf16x8, p);
#else
    return bf16x8{};
#endif
}

// ---- the weight streams.  D: k-tiles in flight per multiplying wave (registers); LOADS: 16-byte loads per lane per k-tile; SLOADS: 4-byte
// loads per lane per k-tile beside them (block scales; the counted wait covers LOADS + SLOADS instructions per k-tile); BY_XB: whether the entry
// launches the instantiation of the x row blocks that hold rows < M (else always all 8).  base / range /
// kstep: the tile's buffer descriptor and the k-tile step in bytes; offset(l, row, fg): the byte offset of load l for the lane whose fragment
// row is `row` of the tile's first 16 (wave * 32 + lane & 15) and whose 8-deep k chunk is fg; frag(r, i, half): the operand of 16-row fragment i,
// 32-deep half `half`, from the k-tile's LOADS registers.

// bf16 weights.  Row-major (nn.Linear.weight): range = the tile's rows inside the matrix (rows beyond N read as zeros).  Tiled
// (vtgb_pack_skinny_weight): the tile's nk blocks of 16 KiB, rows in the LDS swizzle of rounds 1-2 (chunk q of row r holds k-chunk
// q ^ ((r >> 1) & 7)).  Load 2 i + h: fragment i, half h.
struct SkinnyBf16 {
    static constexpr int D = 8, LOADS = 4, SLOADS = 0;
    static constexpr bool SCALED = false, BIASED = false, BY_XB = false;
    static constexpr const char* ENTRY = "gemm_skinny";
    const bf16_t* w;
    int ldw, tiled;
    __device__ uint64_t base(int b, int nk) const { return reinterpret_cast<uint64_t>(w + (tiled ? (int64_t)b * nk * (SK_TILE / 2) : (int64_t)b * SK_BN * ldw)); }
    __device__ unsigned range(int b, int N, int nk) const {
        const int rows_in = N - b * SK_BN < SK_BN ? N - b * SK_BN : SK_BN;
        return tiled ? (unsigned)nk * SK_TILE : (unsigned)(((int64_t)(rows_in - 1) * ldw + nk * SK_BK) * 2);
    }
    __device__ int kstep() const { return tiled ? SK_TILE : SK_BK * 2; }
    __device__ unsigned offset(int l, int row, int fg) const {
        const int r = row + (l >> 1) * 16, chunk = (l & 1) * 4 + fg;
        return tiled ? (unsigned)sk_swz(r, chunk) : (unsigned)(r * ldw + chunk * 8) * 2u;
    }
    static __device__ __forceinline__ bf16x8 frag(const sk_i32x4 (&r)[LOADS], int i, int half) { return __builtin_bit_cast(bf16x8, r[2 * i + half]); }
};

// e4m3 codes (vtgb_pack_skinny_weight_fp8) and their row scales.  8 KiB per (128-row tile, 64-deep k-tile): row r is 64 bytes, its 16-byte
// slot g = [8 codes of k 8g .. 8g+7 | 8 codes of k 32+8g ..], i.e. ONE 16-byte load per lane per 16-row fragment holds the lane's operands of
// both 32-deep MFMAs of the k-tile (a wave reads 1 KiB contiguous per fragment).  Load i: fragment i.
struct SkinnyFp8 {
    static constexpr int D = 16, LOADS = 2, SLOADS = 0;
    static constexpr bool SCALED = true, BIASED = false, BY_XB = true;
    static constexpr const char* ENTRY = "gemm_skinny_fp8";
    const uint8_t* w;
    const float* scale;
    __device__ uint64_t base(int b, int nk) const { return reinterpret_cast<uint64_t>(w + (int64_t)b * nk * SK8_TILE); }
    __device__ unsigned range(int, int, int nk) const { return (unsigned)nk * SK8_TILE; }
    __device__ int kstep() const { return SK8_TILE; }
    __device__ unsigned offset(int l, int row, int fg) const { return (unsigned)((row + l * 16) * 64 + fg * 16); }
    static __device__ __forceinline__ bf16x8 frag(const sk_i32x4 (&r)[LOADS], int i, int half) { return sk8_widen(r[i][2 * half], r[i][2 * half + 1]); }
};

// e2m1 codes and E8M0 block scales (vtgb_pack_skinny_weight_mxfp4).  4096 + 256 bytes per (128-row tile, 64-deep k-tile).  Codes: the 16 bytes
// at ((v * 16 + f) * 4 + g) * 16 belong to the lane of wave v with fragment row f and k chunk g -- dword 2 i + h = the 8 codes of row
// v * 32 + i * 16 + f at k 32 h + 8 g .., i.e. ONE 16-byte load per lane holds the lane's operands of both fragments and both 32-deep MFMAs of
// the k-tile (a wave reads 1 KiB contiguous).  Scales: the dword at 4096 + (v * 16 + f) * 4, byte 2 i + h = the scale byte of that row's block h
// (the four lanes g of a row read the same dword).  The scale is applied by the conversion: SCALED = false, the bf16 epilogue.
// D = 16: 16 KiB of codes + 1 KiB of scales in flight per wave, 64 + 4 KiB per workgroup, in 16 x 5 ring registers; the counted wait is
// vmcnt(30).  Registers and the 6-bit vmcnt would allow D = 24 (96 + 6 KiB, vmcnt(46); D = 32 -- 128 KiB -- needs 160 ring registers and no
// longer fits beside the XB = 8 accumulators at two waves per SIMD), and D = 24 was built and MEASURED SLOWER: the multiplying waves run whole
// groups of D straight-line steps, so a split of 16 or 25 k-tiles (o and down at Vicuna-7B) pays 24 and 48 steps instead of 16 and 32
// ("MXFP4 weight stream").
struct SkinnyMxfp4 {
    static constexpr int D = 16, LOADS = 1, SLOADS = 1;
    static constexpr bool SCALED = false, BIASED = false, BY_XB = true;
    static constexpr const char* ENTRY = "gemm_skinny_mxfp4";
    const uint8_t* w;
    __device__ uint64_t base(int b, int nk) const { return reinterpret_cast<uint64_t>(w + (int64_t)b * nk * SK4_TILE); }
    __device__ unsigned range(int, int, int nk) const { return (unsigned)nk * SK4_TILE; }
    __device__ int kstep() const { return SK4_TILE; }
    __device__ unsigned offset(int, int row, int fg) const { return (unsigned)((((row >> 5) * 16 + (row & 15)) * 4 + fg) * 16); }
    __device__ unsigned scale_offset(int row) const { return (unsigned)(SK4_CODES + ((row >> 5) * 16 + (row & 15)) * 4); }
    static __device__ __forceinline__ bf16x8 frag(const sk_i32x4 (&r)[LOADS], int sc, int i, int half) {
        return sk4_widen(r[0][2 * i + half], ((unsigned)sc >> (8 * (2 * i + half))) & 0xFFu);
    }
};

// Either stream with a projection bias (vtgb_gemm_skinny_bias): bias[n] fp32 is added to the fp32 accumulators of split 0 alone, behind the row
// scale and before the fragment leaves the registers, so whoever adds the fragments in split order -- the reduce launch, the deferred
// consumers -- rounds acc + bias once and needs no change.  A stream type of its own: the kernels of the plain streams keep their
// parameters and their code.
template <typename Base>
struct SkinnyBiased : Base {
    static constexpr bool BIASED = true;
    static constexpr const char* ENTRY = "gemm_skinny_bias";
    const float* bias;
};

template <typename WS, int XB>
__global__ __launch_bounds__(SK_THREADS) void gemm_skinny_kernel(const bf16_t* __restrict__ x, int M, int ldx, const WS ws, int N, int nk, float* __restrict__ part,
                                                                 void* __restrict__ out, int64_t ldo, int out_f32) {
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ __attribute__((aligned(16))) char sk_smem[];      // the x ring: SK_XSLOTS tiles (rows < 16 XB of each are used)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x, S = gridDim.y, sp = blockIdx.y;
    const int k0 = (int)((int64_t)nk * sp / S), k1 = (int)((int64_t)nk * (sp + 1) / S), ns = k1 - k0;   // this split's k-tiles
    if (ns <= 0) return;
    if (wave >= 4) {
        // ---------------- loader waves: each stages 8 XB of the 16 XB x rows of every k-tile (XB pieces of 8 rows x 128 bytes)
        const int lw = wave - 4;
        const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(x), 0, 0x7FFFFF00, 0x00020000);
        unsigned voff[XB];
#pragma unroll
        for (int i = 0; i < XB; i++) {
            const int row = (lw * XB + i) * 8 + (lane >> 3), slot = lane & 7, c = slot ^ ((row >> 1) & 7);
            voff[i] = (unsigned)((row < M ? row : M - 1) * ldx + c * 8) * 2u;
        }
#define SK_ISSUE_X(slot, kt)                                                                                 \
        _Pragma("unroll") for (int i = 0; i < XB; i++)                                                       \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (sk_lptr_t)(sk_smem + (slot) * SK_TILE + (lw * XB + i) * 8 * 128), 16, voff[i], (kt) * (SK_BK * 2), 0, 0);
        for (int t = 0; t < SK_XD && t < ns; t++) { SK_ISSUE_X(t, k0 + t) }
        int slot_in = SK_XD % SK_XSLOTS;
        const int nsp = (ns + WS::D - 1) / WS::D * WS::D;     // the multiplying waves run whole groups of WS::D steps: same barrier count here
        for (int t = 0; t < nsp; t++) {
            // my pieces of k-tiles t AND t + 1 (the multiplying waves read one fragment group ahead, across the barrier) have landed
            // when only the k-tiles younger than t + 1 (XB pieces each) are outstanding
            const int younger = t >= ns - 2 ? 0 : ns - 2 - t < SK_XD - 2 ? ns - 2 - t : SK_XD - 2;
            sk_wait_stages<XB>(younger);
            __builtin_amdgcn_s_barrier();                      // x of k-tiles t, t + 1 is in LDS; everyone is done with k-tile t - 1
            if (t + SK_XD < ns) { SK_ISSUE_X(slot_in, k0 + t + SK_XD) }      // (slot of k-tile t + XD - XSLOTS = t - 1: free)
            slot_in = slot_in + 1 == SK_XSLOTS ? 0 : slot_in + 1;
        }
#undef SK_ISSUE_X
        return;
    }
    // ---------------- multiplying waves: 32 weight rows each, fragments straight from memory
    const int fr = lane & 15, fg = lane >> 4;
    // one descriptor for the tile (its words by hand: the loads below are inline asm -- see SK_ISSUE_W); per-lane byte offsets of the k-tile's
    // loads; k-tile step in bytes
    const uint64_t wptr = ws.base(b, nk);
    const sk_i32x4 wrsrc = {__builtin_amdgcn_readfirstlane((int)(unsigned)wptr), __builtin_amdgcn_readfirstlane((int)((wptr >> 32) & 0xFFFFu)),
                            __builtin_amdgcn_readfirstlane((int)ws.range(b, N, nk)), 0x00020000};
    const int kstep = ws.kstep();
    unsigned wv[WS::LOADS];
#pragma unroll
    for (int l = 0; l < WS::LOADS; l++) wv[l] = ws.offset(l, wave * 32 + fr, fg);
    sk_i32x4 wreg[WS::D][WS::LOADS];
    unsigned wsv = 0;                  // a stream with block scales (WS::SLOADS = 1): their per-lane byte offset and their ring, one dword per k-tile
    int wsc[WS::D];
    if constexpr (WS::SLOADS != 0) wsv = ws.scale_offset(wave * 32 + fr);
    // The ring's loads are inline asm and its waits are written by hand: with the builtin, hipcc's own vmcnt bookkeeping drained
    // the whole ring (vmcnt(0)) at the top of every group of WS::D steps -- it cannot see that a register loaded in one trip of the
    // loop is consumed in the next -- which halves the bytes in flight.  SK_WAIT_W(u): everything but the WS::D - 1 younger k-tiles
    // (WS::LOADS loads each) has landed, i.e. ring entry u; the empty asm ties the registers' next use to that point.
#define SK_ISSUE_W(u, t)                                                                                     \
    {                                                                                                        \
        const int so_ = __builtin_amdgcn_readfirstlane((t) < ns ? (k0 + (t)) * kstep : 0x7FFFFF00);   /* past the split: out of range, no traffic */ \
        _Pragma("unroll") for (int l = 0; l < WS::LOADS; l++)                                                \
            asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=&v"(wreg[u][l]) : "v"(wv[l]), "s"(wrsrc), "s"(so_) : "memory"); \
        if constexpr (WS::SLOADS != 0)                                                                       \
            asm volatile("buffer_load_dword %0, %1, %2, %3 offen" : "=&v"(wsc[u]) : "v"(wsv), "s"(wrsrc), "s"(so_) : "memory"); \
    }
#define SK_WAIT_W(u)                                                                                         \
    {                                                                                                        \
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((WS::LOADS + WS::SLOADS) * (WS::D - 1)) : "memory");        \
        _Pragma("unroll") for (int l = 0; l < WS::LOADS; l++) asm volatile("" : "+v"(wreg[u][l]));           \
        if constexpr (WS::SLOADS != 0) asm volatile("" : "+v"(wsc[u]));                                      \
    }
    f32x4 acc[2][XB];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < XB; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < WS::D; u++) { SK_ISSUE_W(u, u) }
    // x fragments in groups of G (group g of a k-tile: 32-deep half g / NH, x row blocks G (g % NH) ...; XB = 8: four quads), double
    // buffered -- the next group's LDS reads are issued before the current group's 2 G MFMAs (one wave per SIMD: nobody else hides the LDS
    // latency), and group 0 of the NEXT k-tile before the last group of this one (the loaders guarantee k-tile t + 1 at barrier t).  Every
    // accumulator gets half 0 then half 1 of every k-tile.
    constexpr int G = XB < 4 ? XB : 4, NG = 2 * XB / G, NH = NG / 2;
    static_assert(NH == 1 || NH == 2, "SK_READ_X takes g % NH and g / NH as g & (NH - 1) and g >> (NH - 1): with % and / hipcc keeps the LDS read address in two parts and adds them every step");
    bf16x8 xf[2][G];
#define SK_READ_X(buf, xs_, g)                                                                               \
    _Pragma("unroll") for (int j = 0; j < G; j++)                                                            \
        xf[buf][j] = *reinterpret_cast<const bf16x8*>((xs_) + sk_swz((((g) & (NH - 1)) * G + j) * 16 + fr, ((g) >> (NH - 1)) * 4 + fg));
    int slot_x = 0;
    const char* xs = sk_smem;
    bool primed = false;
    for (int t0 = 0; t0 < ns; t0 += WS::D) {
#pragma unroll
        for (int u = 0; u < WS::D; u++) {
            // Straight-line steps (a branch per step made hipcc drain the weight ring with vmcnt(0..3) at every join): the steps of
            // the last group past the split multiply ZERO weight fragments (out-of-range loads) with the last real x tile.
            const int t = t0 + u;
            __builtin_amdgcn_s_barrier();                      // x of k-tiles t, t + 1 is in LDS
            if (!primed) { SK_READ_X(0, xs, 0) primed = true; }
            if (t < ns - 1) slot_x = slot_x + 1 == SK_XSLOTS ? 0 : slot_x + 1;
            const char* const xs_next = sk_smem + slot_x * SK_TILE;
            SK_WAIT_W(u)
            bf16x8 wf[2][2];                                   // [fragment][32-deep half]
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    if constexpr (WS::SLOADS != 0) wf[i][h] = WS::frag(wreg[u], wsc[u], i, h);
                    else wf[i][h] = WS::frag(wreg[u], i, h);
                }
#pragma unroll
            for (int g = 0; g < NG; g++) {
                if (g < NG - 1) { SK_READ_X((g + 1) & 1, xs, g + 1) } else { SK_READ_X(0, xs_next, 0) }
                __builtin_amdgcn_sched_barrier(0);             // (left alone, hipcc sinks the reads to just before their MFMAs)
#pragma unroll
                for (int j = 0; j < G; j++) {
                    acc[0][(g % NH) * G + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[0][g / NH], xf[g & 1][j], acc[0][(g % NH) * G + j], 0, 0, 0);
                    acc[1][(g % NH) * G + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[1][g / NH], xf[g & 1][j], acc[1][(g % NH) * G + j], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            xs = xs_next;
            SK_ISSUE_W(u, t + WS::D)
        }
    }
    // The last group's re-issues (out of range: zeros, no traffic) may still be in flight, and hipcc, which does not know of them, hands their
    // registers to the epilogue.  The streams above have run that way since they were written and keep their code; a stream added since drains.
    if constexpr (WS::SLOADS != 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#undef SK_READ_X
#undef SK_ISSUE_W
#undef SK_WAIT_W
    // D layout: column (lane & 15) <- x row (m), rows (lane >> 4) * 4 + reg <- w row (n); a scaled stream's row scales first (rows beyond N: 1),
    // then split 0's bias (rows beyond N: 0, never read)
    f32x4 sc[2] = {};
    f32x4 bi[2] = {};
    if constexpr (WS::BIASED) {
        if (sp == 0) {
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int n = b * SK_BN + wave * 32 + i * 16 + fg * 4 + e;
                    bi[i][e] = n < N ? ws.bias[n] : 0.f;
                }
        }
    }
    if constexpr (WS::SCALED) {
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int n = b * SK_BN + wave * 32 + i * 16 + fg * 4 + e;
                sc[i][e] = n < N ? ws.scale[n] : 1.f;
            }
    }
#pragma unroll
    for (int j = 0; j < XB; j++) {
        const int m = j * 16 + fr;
        if (m >= M) continue;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int c = wave * 32 + i * 16 + fg * 4, n = b * SK_BN + c;
            f32x4 v = acc[i][j];
            if constexpr (WS::SCALED) v *= sc[i];
            if constexpr (WS::BIASED) v += bi[i];
            if (S > 1) {
                *reinterpret_cast<f32x4*>(part + ((int64_t)(b * S + sp) * M + m) * SK_BN + c) = v;
            } else if (n < N) {                                // no K split: round once and store straight to `out`
                if (out_f32) {
                    float* o = reinterpret_cast<float*>(out) + m * ldo + n;
                    if (n + 3 < N) *reinterpret_cast<f32x4*>(o) = v;
                    else for (int e = 0; e < 4 && n + e < N; e++) o[e] = v[e];
                } else {
                    bf16_t* o = reinterpret_cast<bf16_t*>(out) + m * ldo + n;
                    if (n + 3 < N) *reinterpret_cast<bf16x4*>(o) = bf16x4{(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
                    else for (int e = 0; e < 4 && n + e < N; e++) o[e] = (bf16_t)v[e];
                }
            }
        }
    }
#endif
}

// out[m][b * 128 + c] = sum over the splits, in split order, of tile b's fragments
template <typename T>
__global__ __launch_bounds__(256) void gemm_skinny_reduce_kernel(const float* __restrict__ part, int M, int N, int S, T* __restrict__ out, int64_t ldo) {
    const int b = blockIdx.x, c4 = (threadIdx.x & 31) * 4, n = b * SK_BN + c4;
    if (n >= N) return;
    for (int m = blockIdx.y * 8 + (threadIdx.x >> 5); m < M; m += gridDim.y * 8) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        for (int sp = 0; sp < S; sp++) v += *reinterpret_cast<const f32x4*>(part + ((int64_t)(b * S + sp) * M + m) * SK_BN + c4);
        T* o = out + m * ldo + n;
        if (n + 3 < N) {
            if constexpr (sizeof(T) == 2) *reinterpret_cast<bf16x4*>(o) = bf16x4{(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
            else *reinterpret_cast<f32x4*>(o) = v;
        } else {
            for (int e = 0; e < 4 && n + e < N; e++) o[e] = (T)v[e];
        }
    }
}

// ---- one-time weight preparation

// The tiled bf16 layout: dst[tile b][k-tile kt][row r][16-byte slot q] = src[b * 128 + r][kt * 64 + 8 (q ^ ((r >> 1) & 7)) ...],
// rows beyond N zero.  One thread per 16-byte chunk.
__global__ __launch_bounds__(256) void skinny_pack_kernel(const bf16_t* __restrict__ src, int64_t ld, int N, int nk, bf16_t* __restrict__ dst, int64_t chunks) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= chunks) return;
    const int q = (int)(i & 7), r = (int)((i >> 3) & 127);
    const int64_t blk = i >> 10, b = blk / nk, kt = blk - b * nk;
    const int64_t n = b * 128 + r;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (n < N) v = *reinterpret_cast<const uint4*>(src + n * ld + kt * 64 + 8 * (q ^ ((r >> 1) & 7)));
    *reinterpret_cast<uint4*>(dst + i * 8) = v;
}

extern "C" size_t vtgb_pack_skinny_weight_bytes(int32_t N, int32_t K) {
    if (N <= 0 || K <= 0 || (K % SK_BK) != 0) return 0;
    return (size_t)((N + SK_BN - 1) / SK_BN) * (K / SK_BK) * SK_TILE;
}

extern "C" int vtgb_pack_skinny_weight(const void* w, int64_t ldw, int32_t N, int32_t K, void* dst, vtgb_stream_t s) {
    VTGB_REQUIRE(w && dst && N > 0 && K > 0 && (K % SK_BK) == 0 && (ldw % 8) == 0 && ldw >= K, VTGB_EINVAL, "pack_skinny_weight: N=%d K=%d ldw=%lld", N, K,
                 (long long)ldw);
    const int64_t chunks = (int64_t)vtgb_pack_skinny_weight_bytes(N, K) / 16;
    hipLaunchKernelGGL(skinny_pack_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, s, (const bf16_t*)w, ldw, N, K / SK_BK, (bf16_t*)dst, chunks);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

// scale[n] = 2^e[n]: one wave per weight row
__global__ __launch_bounds__(256) void skinny_fp8_scale_kernel(const bf16_t* __restrict__ src, int64_t ld, int N, int K, float* __restrict__ scale) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (n >= N) return;
    float amax = 0.f;
    for (int k = lane * 8; k < K; k += 512) {
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(src + n * ld + k);
#pragma unroll
        for (int e = 0; e < 8; e++) amax = fmaxf(amax, fabsf((float)v[e]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    if (lane == 0) scale[n] = ldexpf(1.f, sk8_row_exp(amax));
}

// dst[tile b][k-tile kt][row r][slot g] = codes of src[b * 128 + r][kt * 64 + 8 g ...] | codes of src[..][kt * 64 + 32 + 8 g ...], rows beyond N
// zero.  One thread per 16-byte slot.
__global__ __launch_bounds__(256) void skinny_fp8_pack_kernel(const bf16_t* __restrict__ src, int64_t ld, int N, int nk, const float* __restrict__ scale,
                                                              uint8_t* __restrict__ dst, int64_t chunks) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= chunks) return;
    const int g = (int)(i & 3), r = (int)((i >> 2) & 127);
    const int64_t blk = i >> 9, b = blk / nk, kt = blk - b * nk;
    const int64_t n = b * 128 + r;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (n < N) {
        int ex;
        (void)frexpf(scale[n], &ex);                           // scale = 2^(ex - 1)
        const bf16_t* s = src + n * ld + kt * 64 + 8 * g;
        const bf16x8 h0 = *reinterpret_cast<const bf16x8*>(s), h1 = *reinterpret_cast<const bf16x8*>(s + 32);
        uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
        for (int e = 0; e < 8; e++) {
            o[e >> 2] |= (uint32_t)sk8_code(ldexpf((float)h0[e], 1 - ex)) << (8 * (e & 3));
            o[2 + (e >> 2)] |= (uint32_t)sk8_code(ldexpf((float)h1[e], 1 - ex)) << (8 * (e & 3));
        }
        v = make_uint4(o[0], o[1], o[2], o[3]);
    }
    *reinterpret_cast<uint4*>(dst + i * 16) = v;
}

extern "C" size_t vtgb_pack_skinny_weight_fp8_bytes(int32_t N, int32_t K) {
    if (N <= 0 || K <= 0 || (K % SK_BK) != 0) return 0;
    return (size_t)((N + SK_BN - 1) / SK_BN) * (K / SK_BK) * SK8_TILE;
}

extern "C" int vtgb_pack_skinny_weight_fp8(const void* w, int64_t ldw, int32_t N, int32_t K, void* dst, float* scale_out, vtgb_stream_t s) {
    VTGB_REQUIRE(w && dst && scale_out && N > 0 && K > 0 && (K % SK_BK) == 0 && (ldw % 8) == 0 && ldw >= K, VTGB_EINVAL,
                 "pack_skinny_weight_fp8: N=%d K=%d ldw=%lld", N, K, (long long)ldw);
    const int64_t chunks = (int64_t)vtgb_pack_skinny_weight_fp8_bytes(N, K) / 16;
    hipLaunchKernelGGL(skinny_fp8_scale_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, (const bf16_t*)w, ldw, N, K, scale_out);
    hipLaunchKernelGGL(skinny_fp8_pack_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, s, (const bf16_t*)w, ldw, N, K / SK_BK,
                       (const float*)scale_out, (uint8_t*)dst, chunks);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

// One workgroup per (128-row tile, k-tile) block of the stream, one thread per 16-byte code slot (wave v, fragment row f, k chunk g): the four
// lanes g of a row hold its two 32-blocks of the k-tile between them (amax by two shuffles); lane g = 0 writes the row pair's four scale bytes.
// ops.quantize_mxfp4_rows in integer and exact fp32 arithmetic: e from the exponent field of the block's largest |w|, the element times 2^-e
// (a power of two: exact, or below 2^-126 where the code is 0 either way) against the grid's midpoints, which go to the even code.
__global__ __launch_bounds__(256) void skinny_mxfp4_pack_kernel(const bf16_t* __restrict__ src, int64_t ld, int N, int nk, uint8_t* __restrict__ dst) {
    const int tid = threadIdx.x, g = tid & 3, f = (tid >> 2) & 15, v = tid >> 6;
    const int64_t blk = blockIdx.x, b = blk / nk, kt = blk - b * nk;
    uint32_t o[4] = {0, 0, 0, 0}, sc = 0;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int64_t n = b * 128 + v * 32 + i * 16 + f;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            uint4 raw = make_uint4(0, 0, 0, 0);                // (rows beyond N: zero codes under e = 0)
            if (n < N) raw = *reinterpret_cast<const uint4*>(src + n * ld + kt * 64 + h * 32 + g * 8);
            const uint32_t rw[4] = {raw.x, raw.y, raw.z, raw.w};
            uint32_t bits[8], amax = 0;
#pragma unroll
            for (int e = 0; e < 8; e++) {
                bits[e] = (rw[e >> 1] >> (16 * (e & 1))) & 0xFFFFu;
                amax = max(amax, bits[e] & 0x7FFFu);           // (|bf16| compares as its bits)
            }
            amax = max(amax, (uint32_t)__shfl_xor((int)amax, 1));
            amax = max(amax, (uint32_t)__shfl_xor((int)amax, 2));
            int ex = (int)(amax >> 7) - 127 - 2;               // floor(log2(amax)) - 2; a subnormal amax lands below the clamp
            ex = amax == 0 ? 0 : ex < -120 ? -120 : ex > 125 ? 125 : ex;
            const float down = __uint_as_float((uint32_t)(127 - ex) << 23);      // 2^-e
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const float a = __uint_as_float((bits[e] & 0x7FFFu) << 16) * down;
                const uint32_t code = (uint32_t)(a > 0.25f) + (uint32_t)(a >= 0.75f) + (uint32_t)(a > 1.25f) + (uint32_t)(a >= 1.75f) + (uint32_t)(a > 2.5f) +
                                      (uint32_t)(a >= 3.5f) + (uint32_t)(a > 5.f);
                o[2 * i + h] |= (code | ((bits[e] >> 15) << 3)) << (4 * e);
            }
            sc |= (uint32_t)(ex + 127) << (8 * (2 * i + h));
        }
    }
    uint8_t* const out = dst + blk * SK4_TILE;
    *reinterpret_cast<uint4*>(out + tid * 16) = make_uint4(o[0], o[1], o[2], o[3]);
    if (g == 0) *reinterpret_cast<uint32_t*>(out + SK4_CODES + (v * 16 + f) * 4) = sc;
}

extern "C" size_t vtgb_pack_skinny_weight_mxfp4_bytes(int32_t N, int32_t K) {
    if (N <= 0 || K <= 0 || (K % SK_BK) != 0) return 0;
    return (size_t)((N + SK_BN - 1) / SK_BN) * (K / SK_BK) * SK4_TILE;
}

extern "C" int vtgb_pack_skinny_weight_mxfp4(const void* w, int64_t ldw, int32_t N, int32_t K, void* dst, vtgb_stream_t s) {
    VTGB_REQUIRE(w && dst && N > 0 && K > 0 && (K % SK_BK) == 0 && (ldw % 8) == 0 && ldw >= K, VTGB_EINVAL, "pack_skinny_weight_mxfp4: N=%d K=%d ldw=%lld", N, K,
                 (long long)ldw);
    const int64_t blocks = (int64_t)((N + SK_BN - 1) / SK_BN) * (K / SK_BK);
    hipLaunchKernelGGL(skinny_mxfp4_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const bf16_t*)w, ldw, N, K / SK_BK, (uint8_t*)dst);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

// ---- host side

// splits.  Measured (tools/exp/skinny_bench.py, hipGraph replay, M = 124; profiles/r03_skinny_experiments.md): a workgroup streams
// ~16 KiB of weights per 0.45 us whatever is in flight (ablations: without the x stream 0.47 us per k-tile, without the weight stream
// 0.43 us -- both go through the CU's one L1/TA path, and x is re-read by every tile), so the stream count decides: >= 160 tiles run
// unsplit (gate|up, lm_head); fewer tiles are split until ~128 workgroups stream, long K a little further (one split per 24
// k-tiles), never more than 8 splits (each costs an M x 128 fp32 fragment written and read back) or fewer than 8 k-tiles per split.
static int skinny_splits(const vtgb_gemm_skinny_args* a) {
    const int nk = a->K / SK_BK, n_tiles = (a->N + SK_BN - 1) / SK_BN;
    if (a->n_splits > 0) return a->n_splits < nk ? a->n_splits : nk;
    if (n_tiles >= 160) return 1;
    int S = (128 + n_tiles - 1) / n_tiles;
    if (S < nk / 24) S = nk / 24;
    if (S > 8) S = 8;
    while (S > 1 && nk / S < 8) S--;
    return S;
}

// bytes of the fragments S splits leave (the layout contract above)
static size_t skinny_part_bytes(const vtgb_gemm_skinny_args* a, int S) {
    return S == 1 ? 0 : (size_t)((a->N + SK_BN - 1) / SK_BN) * S * a->M * SK_BN * sizeof(float);
}

static int skinny_check(const vtgb_gemm_skinny_args* a) {
    VTGB_REQUIRE(a, VTGB_EINVAL, "gemm_skinny: NULL args");
    VTGB_REQUIRE(a->M > 0 && a->M <= 128 && a->N > 0 && a->K > 0 && (a->K % SK_BK) == 0, VTGB_EUNSUPPORTED,
                 "gemm_skinny: M=%d (<= 128), N=%d, K=%d (multiple of 64)", a->M, a->N, a->K);
    VTGB_REQUIRE((a->ldx % 8) == 0 && a->ldx >= a->K && a->ldo >= a->N && (int64_t)128 * a->ldx * 2 < 0x7FFFFF00ll &&
                     (a->w_tiled ? (int64_t)((a->N + 127) / 128) * 128 * a->K * 2 < 0x7FFFFF00ll
                                 : ((a->ldw % 8) == 0 && a->ldw >= a->K && (int64_t)((a->N + 127) / 128) * 128 * a->ldw * 2 < 0x7FFFFF00ll)),
                 VTGB_EINVAL, "gemm_skinny: row pitches ldx=%lld ldw=%lld ldo=%lld (operands must stay below 2 GiB)", (long long)a->ldx, (long long)a->ldw,
                 (long long)a->ldo);
    VTGB_REQUIRE(a->out_dtype == VTGB_BF16 || a->out_dtype == VTGB_F32, VTGB_EINVAL, "gemm_skinny: bad out_dtype %d", a->out_dtype);
    VTGB_REQUIRE(a->n_splits >= 0 && a->n_splits <= 64, VTGB_EINVAL, "gemm_skinny: n_splits=%d", a->n_splits);
    return VTGB_OK;
}

extern "C" int32_t vtgb_gemm_skinny_splits(const vtgb_gemm_skinny_args* a) {
    if (skinny_check(a) != VTGB_OK) return 0;
    return skinny_splits(a);
}

extern "C" size_t vtgb_gemm_skinny_workspace_bytes(const vtgb_gemm_skinny_args* a) {
    if (skinny_check(a) != VTGB_OK) return 0;
    return skinny_part_bytes(a, skinny_splits(a));
}

template <typename WS, int XB>
static int skinny_launch(const vtgb_gemm_skinny_args* a, const WS& ws, int S, vtgb_stream_t s) {
    constexpr int LDS = SK_XSLOTS * SK_TILE;
    const auto kernel = gemm_skinny_kernel<WS, XB>;
    static DeviceOnce attr;
    VTGB_FUNC_LDS_ONCE(attr, kernel, LDS);
    ProfScope prof(VTGB_PROF_GEMM, 2.0 * a->M * a->N * a->K, s);
    hipLaunchKernelGGL(kernel, dim3((a->N + SK_BN - 1) / SK_BN, S), dim3(SK_THREADS), LDS, s, (const bf16_t*)a->x, a->M, (int)a->ldx, ws, a->N, a->K / SK_BK,
                       (float*)a->workspace, a->out, a->ldo, a->out_dtype == VTGB_F32 ? 1 : 0);
    return VTGB_OK;
}

// Both entry points, after skinny_check and their own operand checks (in that order: a bad shape is reported before a NULL operand); the
// caller names its weight stream by the type of `ws`.
template <typename WS>
static int skinny_run(const vtgb_gemm_skinny_args* a, const WS& ws, vtgb_stream_t s) {
    const int S = skinny_splits(a);
    const size_t need = skinny_part_bytes(a, S);
    VTGB_REQUIRE(need == 0 || (a->workspace && a->workspace_bytes >= need), VTGB_EWORKSPACE, "%s: workspace %zu < %zu bytes", WS::ENTRY, a->workspace_bytes, need);
    if constexpr (!WS::BY_XB) {
        // bf16 always runs all 8 x row blocks: specialising it on XB as fp8 does would change what the default mode launches at small batch
        VTGB_TRY((skinny_launch<WS, 8>(a, ws, S, s)));
    } else {
        // the x row blocks that hold rows < M
        if (a->M <= 16) VTGB_TRY((skinny_launch<WS, 1>(a, ws, S, s)));
        else if (a->M <= 32) VTGB_TRY((skinny_launch<WS, 2>(a, ws, S, s)));
        else if (a->M <= 64) VTGB_TRY((skinny_launch<WS, 4>(a, ws, S, s)));
        else VTGB_TRY((skinny_launch<WS, 8>(a, ws, S, s)));
    }
    if (S > 1 && !a->defer_reduce) {      // (defer_reduce: the consumer adds the fragments -- vtgb_llm_rmsnorm_parts / vtgb_llm_rope_cache_parts)
        const dim3 rgrid((a->N + SK_BN - 1) / SK_BN, (a->M + 7) / 8 < 4 ? (a->M + 7) / 8 : 4);
        if (a->out_dtype == VTGB_BF16)
            hipLaunchKernelGGL(gemm_skinny_reduce_kernel<bf16_t>, rgrid, dim3(256), 0, s, (const float*)a->workspace, a->M, a->N, S, (bf16_t*)a->out, a->ldo);
        else
            hipLaunchKernelGGL(gemm_skinny_reduce_kernel<float>, rgrid, dim3(256), 0, s, (const float*)a->workspace, a->M, a->N, S, (float*)a->out, a->ldo);
    }
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

extern "C" int vtgb_gemm_skinny(const vtgb_gemm_skinny_args* a, vtgb_stream_t s) {
    VTGB_TRY(skinny_check(a));
    VTGB_REQUIRE(a->x && a->w && a->out, VTGB_EINVAL, "gemm_skinny: NULL operand");
    return skinny_run(a, SkinnyBf16{(const bf16_t*)a->w, (int)a->ldw, a->w_tiled}, s);
}

extern "C" int vtgb_gemm_skinny_fp8(const vtgb_gemm_skinny_args* a, const float* w_scale, vtgb_stream_t s) {
    VTGB_TRY(skinny_check(a));
    VTGB_REQUIRE(a->x && a->w && a->out && w_scale, VTGB_EINVAL, "gemm_skinny_fp8: NULL operand");
    VTGB_REQUIRE(a->w_tiled == 1, VTGB_EINVAL, "gemm_skinny_fp8: the weights are a vtgb_pack_skinny_weight_fp8 stream (w_tiled = 1)");
    return skinny_run(a, SkinnyFp8{(const uint8_t*)a->w, w_scale}, s);
}

extern "C" int vtgb_gemm_skinny_bias(const vtgb_gemm_skinny_args* a, const float* w_scale, const float* bias, vtgb_stream_t s) {
    VTGB_TRY(skinny_check(a));
    VTGB_REQUIRE(a->x && a->w && a->out && bias, VTGB_EINVAL, "gemm_skinny_bias: NULL operand");
    VTGB_REQUIRE((reinterpret_cast<uintptr_t>(bias) & 3) == 0, VTGB_EUNSUPPORTED, "gemm_skinny_bias: bias %p is not 4-byte aligned", (const void*)bias);
    if (!w_scale) return skinny_run(a, SkinnyBiased<SkinnyBf16>{{(const bf16_t*)a->w, (int)a->ldw, a->w_tiled}, bias}, s);
    VTGB_REQUIRE(a->w_tiled == 1, VTGB_EINVAL, "gemm_skinny_bias: fp8 weights are a vtgb_pack_skinny_weight_fp8 stream (w_tiled = 1)");
    return skinny_run(a, SkinnyBiased<SkinnyFp8>{{(const uint8_t*)a->w, w_scale}, bias}, s);
}

extern "C" int vtgb_gemm_skinny_mxfp4(const vtgb_gemm_skinny_args* a, const float* bias, vtgb_stream_t s) {
    VTGB_TRY(skinny_check(a));
    VTGB_REQUIRE(a->x && a->w && a->out, VTGB_EINVAL, "gemm_skinny_mxfp4: NULL operand");
    VTGB_REQUIRE(a->w_tiled == 1, VTGB_EINVAL, "gemm_skinny_mxfp4: the weights are a vtgb_pack_skinny_weight_mxfp4 stream (w_tiled = 1)");
    if (!bias) return skinny_run(a, SkinnyMxfp4{(const uint8_t*)a->w}, s);
    VTGB_REQUIRE((reinterpret_cast<uintptr_t>(bias) & 3) == 0, VTGB_EUNSUPPORTED, "gemm_skinny_mxfp4: bias %p is not 4-byte aligned", (const void*)bias);
    return skinny_run(a, SkinnyBiased<SkinnyMxfp4>{{(const uint8_t*)a->w}, bias}, s);
}
