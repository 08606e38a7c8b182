// conv64.hip -- 3x3, stride 1, 64 -> 64 channel convolution with the input rows RESIDENT in LDS (gfx950).
//
// RAFT's feature / context encoders spend their first residual stage (112 x 112 x 64 at 224 x 224 input; extractor.py:136-143,
// layer1) in four of these per image.  As an implicit GEMM on the general kernel (gemm.hip, 64-wide tile) every k-tile re-stages a
// 256-pixel x 64-channel operand block for each of the nine taps: 64 FLOP per operand byte, and the launches ran at 460 TFLOP/s
// with the L2 -> LDS path, not the matrix cores, setting the pace (a plain [M, 576] x [64, 576]^T GEMM on the same tile: 274 TFLOP/s
// at 4.3 TB/s of operand stream; profiles/r03_conv64.md).  Here an input pixel is staged ONCE and read from LDS by all nine taps:
//   * a persistent workgroup (8 waves) walks runs of image rows two output rows per step (tile = 2 rows x 128 pixel slots x 64
//     channels; W <= 126); an image is cut into as many runs as balance the grid;
//   * LDS holds a ring of 8 input rows x 128 pixel slots x 128 bytes (slot 0 and W + 1 = the zero padding, written by the LDS-DMA's
//     out-of-range reads; rows -1 and H likewise), filled two rows ahead with buffer_load ... lds; 16-byte chunks XOR-swizzled by
//     (slot >> 1) & 7 like every other operand image of this library;
//   * the WEIGHTS live in registers: waves form a 4 (pixels) x 2 (channels) grid, a wave keeps its 32 output channels' 9 x 64
//     weights as 36 MFMA fragments (144 VGPRs) for the whole launch -- LDS bandwidth goes to the pixels only (2 fragment reads per 4
//     MFMAs: 128 B/clk per CU at full MFMA rate, i.e. LDS and matrix cores are balanced);
//   * the four resident input rows of a step feed both output rows: 48 fragment reads for 144 MFMAs;
//   * one barrier per step; the step's 8 stores are ALWAYS issued (invalid pixels store out of the descriptor's range), so the
//     counted wait in front of the next barrier (`vmcnt(8)`: the rows requested one step ago have landed) is exact.
// Epilogues: fp32 output + per-(image, channel) sum / sum of squares for InstanceNorm (fnet: reduced in registers / LDS per run, one
// atomic per channel and run -- stored without atomics when a workgroup owns the image), or bf16 output with ReLU / skip + ReLU
// (cnet, BatchNorm folded into the weights).
#include <type_traits>
#include <utility>
#include "common.h"
#include "pair_h8.h"

namespace {

constexpr int C64_R = 8, C64_RS = 128;                 // ring rows, pixel slots per row
constexpr int C64_ROW_BYTES = C64_RS * 128;            // 16 KiB
constexpr int C64_LDS = C64_R * C64_ROW_BYTES + 8 * 32 * 2 * 4 + 64 * 4;   // + the moments exchange (8 waves x 32 channels x 2) + the bias
typedef __attribute__((address_space(3))) void* c64_lptr_t;

struct Conv64Params {
    const bf16_t* in;      // [n_img, H, W, 64]
    const bf16_t* w;       // [64, 9 * 64]: k = tap * 64 + channel
    const float* bias;     // [64]
    float* out_f32;        // MODE 0: [n_img * H * W, 64]
    float* stats;          // MODE 0: [n_img, 64, 2] (sum, sum of squares)
    float* stats_part;     // parts > 1: [n_img * parts, 64, 2] per-run partial moments
    bf16_t* out_bf16;      // MODE 1
    const bf16_t* resid;   // MODE 1, nullable
    int n_img, H, W, relu, post_relu;
    int parts, rows_per_part;   // an image is cut into `parts` runs of `rows_per_part` (even) output rows: one workgroup walks a run
};

template <int MODE>
__global__ __launch_bounds__(512) void conv3x3_c64_kernel(const Conv64Params p) {
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ __attribute__((aligned(16))) char ring[];
    float* const xch = reinterpret_cast<float*>(ring + C64_R * C64_ROW_BYTES);
    const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, fg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave & 3, wn = wave >> 2;
    const int H = p.H, W = p.W;

    // ---- this wave's weights: fragments [tap][32-deep half][16-channel block] and bias
    bf16x8 wf[9][2][2];
#pragma unroll
    for (int t = 0; t < 9; t++)
#pragma unroll
        for (int ks = 0; ks < 2; ks++)
#pragma unroll
            for (int i = 0; i < 2; i++)
                wf[t][ks][i] = *reinterpret_cast<const bf16x8*>(p.w + (wn * 32 + i * 16 + fr) * 576 + t * 64 + ks * 32 + fg * 8);
    float* const bias_s = xch + 8 * 32 * 2;                // the bias, read back from LDS in every epilogue (8 registers the weight fragments need)
    if (tid < 64) bias_s[tid] = p.bias[tid];

    // ---- staging: wave w issues pieces 2 w, 2 w + 1 of a row (8 pixel slots x 128 bytes each).  Lane l of a piece: slot 8 piece + (l >> 3),
    // LDS chunk position l & 7 <- global chunk (l & 7) ^ ((slot >> 1) & 7) of pixel slot - 1; slots outside [1, W] read out of range (zeros)
    unsigned dma_off[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int slot = (wave * 2 + q) * 8 + (lane >> 3), x = slot - 1, c = (lane & 7) ^ ((slot >> 1) & 7);
        dma_off[q] = (x >= 0 && x < W) ? (unsigned)(x * 64 + c * 8) * 2u : 0x80000000u;
    }
    // ---- fragment reads: pixel px = 32 wm + 16 j + fr of the output row reads slot px + kx (kx = 0..2) of ring row y + ky - 1
    // (fragment j = 1 sits 16 slots = 2048 bytes further with the same swizzle term; the second 32-deep half is chunk ^ 4 = byte ^ 64:
    // three registers instead of twelve.  Pixels beyond the row read whatever slot that lands on: their results are never stored.)
    unsigned x_off[3];
    int px[2];
#pragma unroll
    for (int j = 0; j < 2; j++) px[j] = wm * 32 + j * 16 + fr;
#pragma unroll
    for (int kx = 0; kx < 3; kx++) x_off[kx] = (unsigned)((px[0] + kx) * 128 + ((fg ^ (((px[0] + kx) >> 1) & 7)) << 4));

    typedef __attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned u32x4_t;
    typedef __attribute__((__vector_size__(2 * sizeof(unsigned)))) unsigned u32x2_t;
    constexpr unsigned OOB = 0x80000000u;
    constexpr int ES = MODE == 0 ? 4 : 2;
    // output lane offsets inside an image row (channel block i, pixel fragment j); pixels beyond the row store out of range
    unsigned o_off[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) o_off[i][j] = px[j] < W ? (unsigned)(px[j] * 64 + wn * 32 + i * 16 + fg * 4) * ES : OOB;

    const int n_units = p.n_img * p.parts;
    for (int unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        const int img = unit / p.parts, y0 = (unit - img * p.parts) * p.rows_per_part;
        if (y0 >= H) continue;
        const int y1 = y0 + p.rows_per_part < H ? y0 + p.rows_per_part : H;
        const bf16_t* const ibase = p.in + (int64_t)img * H * W * 64;
        const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(ibase), 0, H * W * 128, 0x00020000);
        const auto orsrc = __builtin_amdgcn_make_buffer_rsrc(MODE == 0 ? (void*)(p.out_f32 + (int64_t)img * H * W * 64) : (void*)(p.out_bf16 + (int64_t)img * H * W * 64), 0,
                                                             H * W * 64 * ES, 0x00020000);
        const auto rrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(p.resid ? p.resid + (int64_t)img * H * W * 64 : ibase), 0, H * W * 128, 0x00020000);
#define C64_ISSUE(yy)                                                                                                          \
        {                                                                                                                      \
            const int so_ = ((yy) >= 0 && (yy) < H) ? (yy) * W * 128 : 0x7FFFFF00;      /* rows -1 and H: out of range, zeros */  \
            char* const dst_ = ring + ((yy) & (C64_R - 1)) * C64_ROW_BYTES + (wave * 2) * 1024;                                \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (c64_lptr_t)dst_, 16, dma_off[0], so_, 0, 0);                       \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (c64_lptr_t)(dst_ + 1024), 16, dma_off[1], so_, 0, 0);              \
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);               // (my rows of the previous unit have landed / been stored: their ring rows are reused)
        __builtin_amdgcn_s_barrier();                     // the previous unit's last rows have been consumed by every wave
        C64_ISSUE(y0 - 1)
        C64_ISSUE(y0)
        C64_ISSUE(y0 + 1)
        C64_ISSUE(y0 + 2)
        f32x4 s1[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}}, s2[2] = {s1[0], s1[0]};
        // Two output rows per step: input rows y - 1 .. y + 2 are resident, each x fragment feeds the taps of both output rows that touch it
        // (48 fragment reads for 144 MFMAs: the matrix cores, not LDS, bound the step).
        for (int y = y0; y < y1; y += 2) {
            // rows y + 1, y + 2 (4 pieces, issued one step ago) have landed when only what was issued behind them is outstanding: the 8
            // stores of the previous step (always issued: invalid pixels / rows store out of range).  First step: everything.
            if (y == y0) __builtin_amdgcn_s_waitcnt(0x0F70);
            else __builtin_amdgcn_s_waitcnt(0x0F78);
            __builtin_amdgcn_s_barrier();                 // everybody's pieces are in LDS; everybody is done with the previous step's rows
            bf16x4 rres[2][2][2];
            if constexpr (MODE == 1) {
                if (p.resid) {                            // (requested BEFORE this step's DMA: vmcnt completes in order)
#pragma unroll
                    for (int o = 0; o < 2; o++)
#pragma unroll
                        for (int i = 0; i < 2; i++)
#pragma unroll
                            for (int j = 0; j < 2; j++) {
                                const unsigned off = (y + o < y1 && o_off[i][j] != OOB) ? o_off[i][j] + (unsigned)((y + o) * W * 64 * 2) : OOB;
                                rres[o][i][j] = __builtin_bit_cast(bf16x4, __builtin_amdgcn_raw_buffer_load_b64(rrsrc, off, 0, 0));
                            }
                }
            }
            C64_ISSUE(y + 3)
            C64_ISSUE(y + 4)
            f32x4 acc[2][2][2];
#pragma unroll
            for (int o = 0; o < 2; o++)
#pragma unroll
                for (int i = 0; i < 2; i++)
#pragma unroll
                    for (int j = 0; j < 2; j++) acc[o][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int rr = 0; rr < 4; rr++) {
                const char* const rowp = ring + ((y + rr - 1) & (C64_R - 1)) * C64_ROW_BYTES;
#pragma unroll
                for (int kx = 0; kx < 3; kx++)
#pragma unroll
                    for (int ks = 0; ks < 2; ks++) {
                        const bf16x8 x0 = *reinterpret_cast<const bf16x8*>(rowp + (x_off[kx] ^ (ks * 64)));
                        const bf16x8 x1 = *reinterpret_cast<const bf16x8*>(rowp + (x_off[kx] ^ (ks * 64)) + 2048);
#pragma unroll
                        for (int o = 0; o < 2; o++) {
                            const int ky = rr - o;
                            if (ky < 0 || ky > 2) continue;
#pragma unroll
                            for (int i = 0; i < 2; i++) {
                                acc[o][i][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ky * 3 + kx][ks][i], x0, acc[o][i][0], 0, 0, 0);
                                acc[o][i][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ky * 3 + kx][ks][i], x1, acc[o][i][1], 0, 0, 0);
                            }
                        }
                    }
            }
            // ---- epilogue: 8 stores, always issued
            f32x4 b4[2];
#pragma unroll
            for (int i = 0; i < 2; i++) b4[i] = *reinterpret_cast<const f32x4*>(bias_s + wn * 32 + i * 16 + fg * 4);
#pragma unroll
            for (int o = 0; o < 2; o++) {
                const bool row_ok = y + o < y1;
#pragma unroll
                for (int i = 0; i < 2; i++)
#pragma unroll
                    for (int j = 0; j < 2; j++) {
                        const bool ok = row_ok && o_off[i][j] != OOB;
                        const unsigned off = ok ? o_off[i][j] + (unsigned)((y + o) * W * 64 * ES) : OOB;
                        f32x4 v = acc[o][i][j] + b4[i];
                        if constexpr (MODE == 0) {
                            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v), orsrc, off, 0, 0);
                            // (selects, not a branch -- a branch here makes hipcc duplicate the store into both arms -- and not a multiply
                            // by 0 / 1: pixel slots beyond the row multiply whatever LDS holds there, possibly NaN)
                            const f32x4 vz = {ok ? v[0] : 0.f, ok ? v[1] : 0.f, ok ? v[2] : 0.f, ok ? v[3] : 0.f};
                            s1[i] += vz;
                            s2[i] += vz * vz;
                        } else {
                            if (p.relu) v = f32x4{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
                            if (p.resid) {
                                const bf16x4 r = rres[o][i][j];
                                v += f32x4{(float)r[0], (float)r[1], (float)r[2], (float)r[3]};
                            }
                            if (p.post_relu) v = f32x4{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
                            const bf16x4 pk = {(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
                            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2_t, pk), orsrc, off, 0, 0);
                        }
                    }
            }
        }
#undef C64_ISSUE
        if constexpr (MODE == 0) {
            // moments of this unit's rows: over the 16 pixel lanes of a fragment, then over the four pixel waves (LDS), added to the image's
            // (sum, sum of squares) -- stored per unit, added in unit order by a second pass (r5: was one atomic per channel and unit)
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    float a_ = s1[i][e], b_ = s2[i][e];
#pragma unroll
                    for (int off = 1; off < 16; off <<= 1) { a_ += __shfl_xor(a_, off); b_ += __shfl_xor(b_, off); }
                    s1[i][e] = a_; s2[i][e] = b_;
                }
            __builtin_amdgcn_s_waitcnt(0xC07F);
            __builtin_amdgcn_s_barrier();                 // (the exchange area is free: the previous unit's reads are done)
            if (fr == 0) {
#pragma unroll
                for (int i = 0; i < 2; i++)
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        xch[(wave * 32 + i * 16 + fg * 4 + e) * 2] = s1[i][e];
                        xch[(wave * 32 + i * 16 + fg * 4 + e) * 2 + 1] = s2[i][e];
                    }
            }
            __syncthreads();
            if (tid < 128) {                              // 64 channels x (sum, sum of squares)
                const int ch = tid >> 1, which = tid & 1, wn_ = ch >> 5, c32 = ch & 31;
                float t = 0.f;
#pragma unroll
                for (int m_ = 0; m_ < 4; m_++) t += xch[((wn_ * 4 + m_) * 32 + c32) * 2 + which];
                // the workgroup owns the image: stored; else stored to this run's slot, added in run order by launch_stats_finish_parts (r5: no atomics)
                if (p.parts == 1) p.stats[((int64_t)img * 64 + ch) * 2 + which] = t;
                else p.stats_part[((int64_t)unit * 64 + ch) * 2 + which] = t;      // (unit = img * parts + run)
            }
        }
    }
#endif
}


// ---------------------------------------------------------------------------------------
// The stem (7x7, stride 2, 3 -> 64 channels; extractor.py:128-130 with the input scaling of xraft.py:105-106) without its HBM
// round trip.  Rounds 1-3a ran it as raft_stem_pack_kernel (a 128-channel "space to depth" image per half-resolution pixel: bf16
// hi | lo pairs of x - 127.5 for a 4 x 2 input-column window, 3.2 MB per frame written) + a 4 x 1 implicit-GEMM convolution that read
// that image back four times: 8.5 + 8.7 ms per 31-clip RAFT batch.  Here a persistent workgroup walks runs of output rows and builds
// the SAME packed rows (same K order, same packed weights: vtgb.h) straight into an LDS ring of 5 rows x W/2 pixels x 256 bytes, one
// row ahead of the row whose 4 vertical taps it multiplies; the wave's 32 x 512 weights live in registers (128 VGPRs) as in
// conv3x3_c64_kernel.  16-byte chunks of a pixel's 256 bytes are XOR-swizzled by (X & 15): the 16 pixels of a fragment read hit 16
// different chunk positions.
// X3 (VTGB_BF16X3 / VTGB_F16C8 encoders): the same rows against the table's split weights [Wh | Wh | Wl] (K = 3 chunks x 4 tY x 64), i.e. the
// contraction [hi | lo | hi] x [Wh | Wh | Wl] of the pack + implicit-GEMM route it replaces, with THAT route's arithmetic per output element:
// the accumulator starts at the bias and takes one in-order MFMA chain in the GEMM's K order (gemm.hip: 64-channel chunk major, tap minor --
// hi.Wh over tY = 0..3, then lo.Wh, then hi.Wl, each k-tile as its two 32-deep halves), so the fp32 output has the GEMM's bits.  The wave
// keeps Wh and Wl of its 32 channels (2 x 8 k-steps x 2 blocks: the 128 VGPRs of the bf16 form's hi | lo table) and reads the hi fragments
// twice (96 MFMAs per row step on 48 fragment reads: the bf16 form's ratio).  MODE 2 (cnet: BatchNorm folded, no moments) applies ReLU and
// stores the pair row [hi(64) | lo(64)] -- bf16 pair or f16c8 (pair_h8.h) -- straight from the accumulators: what x3_pair_pass_kernel wrote
// from the fp32 rows, without the fp32 rows.
// ---------------------------------------------------------------------------------------
constexpr int ST_R = 5;
struct StemParams {
    const float* img;      // [n_img, 3, H, W] raw 0..255 (or CLIP-normalised floats: see raft_enc.hip)
    const bf16_t* w;       // [64, 512]: k = chunk (hi | lo) * 256 + tY * 64 + (dX * 12 + py * 6 + px * 3 + c); X3: [64, 768], chunks Wh | Wh | Wl
    const float* bias;
    float* out_f32;        // MODE 0: [n_img * H2 * W2, 64] + moments
    float* stats;
    float* stats_part;
    bf16_t* out_bf16;      // MODE 1: relu -> bf16; MODE 2: relu -> pair rows [n_img * H2 * W2, 128 16-bit units]
    int n_img, H, W, relu;
    int parts, rows_per_part;
    int h8;                // MODE 2: f16c8 pair instead of a bf16 pair
};

template <int MODE, bool X3>
__global__ __launch_bounds__(512) void stem7x7_kernel(const StemParams p) {
    static_assert(X3 ? (MODE == 0 || MODE == 2) : (MODE == 0 || MODE == 1), "stem7x7: bf16 stores fp32 / bf16 rows, the split form fp32 / pair rows");
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ __attribute__((aligned(16))) char ring[];
    const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, fg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave & 3, wn = wave >> 2;
    const int H = p.H, W = p.W, H2 = H >> 1, W2 = W >> 1;
    const int row_bytes = W2 * 256;
    float* const xch = reinterpret_cast<float*>(ring + ST_R * row_bytes);
    float* const bias_s = xch + 8 * 32 * 2;
    if (tid < 64) bias_s[tid] = p.bias[tid];
    // the 16 zero columns of every 64 (48 real values per tap): chunks 6, 7 (hi) and 14, 15 (lo) of every pixel, written once
    for (int i = tid; i < ST_R * W2 * 4; i += 512) {
        const int pxl = i >> 2, X = pxl % W2, c = 6 + (i & 1) + ((i & 2) << 2);      // 6, 7, 14, 15
        *reinterpret_cast<uint4*>(ring + pxl * 256 + ((c ^ (X & 15)) << 4)) = make_uint4(0, 0, 0, 0);
    }
    // ---- weights: 16 k-steps of 32 (s = chunk * 8 + tY * 2 + half) x two 16-channel blocks; X3: chunk = Wh (table chunk 0) | Wl (table chunk 2)
    constexpr int W_LD = X3 ? 768 : 512;
    bf16x8 wf[16][2];
#pragma unroll
    for (int s_ = 0; s_ < 16; s_++)
#pragma unroll
        for (int i = 0; i < 2; i++)
            wf[s_][i] = *reinterpret_cast<const bf16x8*>(p.w + (wn * 32 + i * 16 + fr) * W_LD + (X3 ? (s_ >> 3) * 512 + (s_ & 7) * 32 : s_ * 32) + fg * 8);
    // ---- building a packed row: thread = (pixel X, column pair dX): 12 values (2 rows x 2 columns x 3 channels) as hi / lo bf16
    const bool builder = tid < W2 * 4;
    const int bX = tid >> 2, bdX = tid & 3, bcol = 2 * (bX + bdX - 2);        // first of the two input columns
    const bool bcol_ok = builder && bcol >= 0 && bcol + 1 < W;                // (W even, bcol even: the pair is inside or outside together)
    const int bcol_c = bcol < 0 ? 0 : bcol + 1 < W ? bcol : W - 2;            // clamped: the loads are unconditional, ST_WRITE zeroes what is outside
    unsigned b_off[3];                                                         // LDS byte offsets of the three 8-byte pieces (hi; lo = chunk + 8)
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const int off = bdX * 24 + q * 8;
        b_off[q] = (unsigned)(bX * 256 + (((off >> 4) ^ (bX & 15)) << 4) + (off & 8));
    }
    // ---- fragment reads: pixel X = 32 wm + 16 j + fr, chunk (hl * 8 + half * 4 + fg) ^ (X & 15)
    int px[2];
    unsigned x_off[2];
#pragma unroll
    for (int j = 0; j < 2; j++) {
        px[j] = wm * 32 + j * 16 + fr;
        const int pc = px[j] < W2 ? px[j] : 0;
        x_off[j] = (unsigned)(pc * 256 + ((fg ^ (pc & 15)) << 4));
    }
    typedef __attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned u32x4_t;
    typedef __attribute__((__vector_size__(2 * sizeof(unsigned)))) unsigned u32x2_t;
    constexpr unsigned OOB = 0x80000000u;
    constexpr int ES = MODE == 0 ? 4 : 2;
    constexpr int PXU = MODE == 2 ? 128 : 64;             // output elements per pixel (pair rows: hi | lo)
    unsigned o_off[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) o_off[i][j] = px[j] < W2 ? (unsigned)(px[j] * PXU + wn * 32 + i * 16 + fg * 4) * ES : OOB;

    const int n_units = p.n_img * p.parts;
    for (int unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        const int img = unit / p.parts, y0 = (unit - img * p.parts) * p.rows_per_part;
        if (y0 >= H2) continue;
        const int y1 = y0 + p.rows_per_part < H2 ? y0 + p.rows_per_part : H2;
        const float* const ibase = p.img + (int64_t)img * 3 * H * W;
        const auto orsrc = __builtin_amdgcn_make_buffer_rsrc(MODE == 0 ? (void*)(p.out_f32 + (int64_t)img * H2 * W2 * 64) : (void*)(p.out_bf16 + (int64_t)img * H2 * W2 * PXU),
                                                             0, H2 * W2 * PXU * ES, 0x00020000);
        float2 ld[6];
        // packed row Yp <- input rows 2 Yp, 2 Yp + 1 (zeros outside the image)
#define ST_LOAD(Yp)      /* unconditional loads from clamped addresses (conditional ones are serialised by hipcc: one vmcnt(0) each) */ \
        {                                                                                                    \
            const int yc_ = (Yp) < 0 ? 0 : (Yp) >= H2 ? H2 - 1 : (Yp);                                       \
            _Pragma("unroll") for (int py = 0; py < 2; py++)                                                 \
                _Pragma("unroll") for (int c = 0; c < 3; c++)                                                \
                    ld[py * 3 + c] = *reinterpret_cast<const float2*>(ibase + ((int64_t)c * H + 2 * yc_ + py) * W + bcol_c); \
        }
#define ST_WRITE(Yp)                                                                                         \
        if (builder) {                                                                                       \
            const bool in_ = bcol_ok && (Yp) >= 0 && (Yp) < H2;                                              \
            bf16_t hi[12], lo[12];                                                                           \
            _Pragma("unroll") for (int py = 0; py < 2; py++)                                                 \
                _Pragma("unroll") for (int c = 0; c < 3; c++) {                                              \
                    const float d0 = in_ ? ld[py * 3 + c].x - 127.5f : 0.f, d1 = in_ ? ld[py * 3 + c].y - 127.5f : 0.f; \
                    const float h0_ = bf16_round(d0), h1_ = bf16_round(d1);                                  \
                    hi[py * 6 + c] = (bf16_t)h0_; lo[py * 6 + c] = (bf16_t)(d0 - h0_);                       \
                    hi[py * 6 + 3 + c] = (bf16_t)h1_; lo[py * 6 + 3 + c] = (bf16_t)(d1 - h1_);               \
                }                                                                                            \
            char* const rb_ = ring + ((((Yp) % ST_R) + ST_R) % ST_R) * row_bytes;                            \
            _Pragma("unroll") for (int q = 0; q < 3; q++) {                                                  \
                *reinterpret_cast<bf16x4*>(rb_ + b_off[q]) = bf16x4{hi[q * 4], hi[q * 4 + 1], hi[q * 4 + 2], hi[q * 4 + 3]}; \
                *reinterpret_cast<bf16x4*>(rb_ + (b_off[q] ^ 128)) = bf16x4{lo[q * 4], lo[q * 4 + 1], lo[q * 4 + 2], lo[q * 4 + 3]}; \
            }                                                                                                \
        }
        __syncthreads();                                       // the previous unit's rows have been consumed (and the one-time zero / bias writes are done)
        for (int yy = y0 - 2; yy <= y0 + 1; yy++) {            // the four rows of the first step (one load latency each: once per unit)
            ST_LOAD(yy)
            ST_WRITE(yy)
        }
        f32x4 s1[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}}, s2[2] = {s1[0], s1[0]};
        for (int y = y0; y < y1; y++) {
            // rows y - 2 .. y + 1 are complete (LDS writes only: __syncthreads would also wait for the previous row's output stores,
            // a memory round trip per row); everybody is done with row y - 3's slot
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_waitcnt(0xC07F);
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
            ST_LOAD(y + 2)                                     // in flight under this row's MFMAs
            f32x4 acc[2][2], b4[2];
            // one 32-deep k-step: the hi (hl = 0) or lo (hl = 1) half-chunk `half` of packed row y + tY - 2 against weight k-step s_
#define ST_STEP(tY, hl, half, s_)                                                                            \
            {                                                                                                \
                const char* const rowp = ring + ((y + (tY) - 2 + ST_R) % ST_R) * row_bytes;                  \
                const unsigned cx = (unsigned)(((hl) * 8 + (half) * 4) << 4);      /* chunk index bits above fg: XORed in (16-byte units) */ \
                const bf16x8 x0 = *reinterpret_cast<const bf16x8*>(rowp + (x_off[0] ^ cx));                  \
                const bf16x8 x1 = *reinterpret_cast<const bf16x8*>(rowp + (x_off[1] ^ cx));                  \
                _Pragma("unroll") for (int i = 0; i < 2; i++) {                                              \
                    acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s_][i], x0, acc[i][0], 0, 0, 0);  \
                    acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s_][i], x1, acc[i][1], 0, 0, 0);  \
                }                                                                                            \
            }
            if constexpr (X3) {
                // the GEMM's chain: bias first (+ its zero start value), then K in table order -- chunk (hi.Wh, lo.Wh, hi.Wl) major, tY minor
#pragma unroll
                for (int i = 0; i < 2; i++) b4[i] = *reinterpret_cast<const f32x4*>(bias_s + wn * 32 + i * 16 + fg * 4);
#pragma unroll
                for (int i = 0; i < 2; i++)
#pragma unroll
                    for (int j = 0; j < 2; j++) acc[i][j] = b4[i] + f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < 3; c++) {
#pragma unroll
                    for (int tY = 0; tY < 4; tY++)
#pragma unroll
                        for (int half = 0; half < 2; half++) ST_STEP(tY, c == 1 ? 1 : 0, half, (c == 2 ? 8 : 0) + tY * 2 + half)
                    // (fragment reads stay inside their chunk: hoisted across all 24 k-steps they cost 9 spilled registers next to the 128 of the weights)
                    if (c < 2) __builtin_amdgcn_sched_barrier(0);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 2; i++)
#pragma unroll
                    for (int j = 0; j < 2; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int tY = 0; tY < 4; tY++)
#pragma unroll
                    for (int hl = 0; hl < 2; hl++)
#pragma unroll
                        for (int half = 0; half < 2; half++) ST_STEP(tY, hl, half, hl * 8 + tY * 2 + half)
#pragma unroll
                for (int i = 0; i < 2; i++) b4[i] = *reinterpret_cast<const f32x4*>(bias_s + wn * 32 + i * 16 + fg * 4);
            }
#undef ST_STEP
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const bool ok = o_off[i][j] != OOB;
                    const unsigned off = ok ? o_off[i][j] + (unsigned)(y * W2 * PXU * ES) : OOB;
                    f32x4 v = X3 ? acc[i][j] : acc[i][j] + b4[i];
                    if constexpr (MODE == 0) {
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v), orsrc, off, 0, 0);
                        const f32x4 vz = {ok ? v[0] : 0.f, ok ? v[1] : 0.f, ok ? v[2] : 0.f, ok ? v[3] : 0.f};
                        s1[i] += vz;
                        s2[i] += vz * vz;
                    } else if constexpr (MODE == 2) {
                        if (p.relu) v = f32x4{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
                        u32x2_t hu, lu;                   // (x3_pair_pass_kernel's split: the pair row it wrote from the fp32 rows)
                        if (p.h8) {
                            h8_split4(v, hu, lu);
                        } else {
                            bf16x4 hi, lo;
                            pair_split4(v, hi, lo);
                            hu = __builtin_bit_cast(u32x2_t, hi); lu = __builtin_bit_cast(u32x2_t, lo);
                        }
                        __builtin_amdgcn_raw_buffer_store_b64(hu, orsrc, off, 0, 0);
                        __builtin_amdgcn_raw_buffer_store_b64(lu, orsrc, ok ? off + 128u : OOB, 0, 0);      // lo half: 64 units further
                    } else {
                        if (p.relu) v = f32x4{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
                        const bf16x4 pk = {(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
                        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2_t, pk), orsrc, off, 0, 0);
                    }
                }
            ST_WRITE(y + 2)                                    // slot of row y - 3
        }
#undef ST_LOAD
#undef ST_WRITE
        if constexpr (X3) {
            if (!p.stats) continue;                            // rows only: the caller adds the moments in an association of its own (raft_enc.hip)
        }
        if constexpr (MODE == 0) {
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    float a_ = s1[i][e], b_ = s2[i][e];
#pragma unroll
                    for (int off = 1; off < 16; off <<= 1) { a_ += __shfl_xor(a_, off); b_ += __shfl_xor(b_, off); }
                    s1[i][e] = a_; s2[i][e] = b_;
                }
            __syncthreads();
            if (fr == 0) {
#pragma unroll
                for (int i = 0; i < 2; i++)
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        xch[(wave * 32 + i * 16 + fg * 4 + e) * 2] = s1[i][e];
                        xch[(wave * 32 + i * 16 + fg * 4 + e) * 2 + 1] = s2[i][e];
                    }
            }
            __syncthreads();
            if (tid < 128) {
                const int ch = tid >> 1, which = tid & 1, wn_ = ch >> 5, c32 = ch & 31;
                float t = 0.f;
#pragma unroll
                for (int m_ = 0; m_ < 4; m_++) t += xch[((wn_ * 4 + m_) * 32 + c32) * 2 + which];
                if (p.parts == 1) p.stats[((int64_t)img * 64 + ch) * 2 + which] = t;
                else p.stats_part[((int64_t)unit * 64 + ch) * 2 + which] = t;      // (unit = img * parts + run)
            }
        }
    }
#endif
}

// ---------------------------------------------------------------------------------------
// layer1 at VTGB_F16C8: the same 3x3 / stride 1 / 64 -> 64 convolution over f16c8 pair rows [M, 128 16-bit units] (pair_h8.h: 128 bytes of fp16 values +
// 128 correction bytes per pixel), with the rows resident.  On gemm_h8.hip's 256 x 64 tile every pixel's 256 bytes were staged nine times (once per tap, 40
// LDS-DMA pieces per 512 matrix-pipe cycles) and the 8 KiB weight tile once per k-tile of every m-tile: 27-30 % matrix-pipe busy.  Here
//   * a persistent workgroup (8 waves) walks runs of image rows ONE output row per step; LDS holds a ring of 4 input rows x (W + 2, rounded up to 4) pixel slots
//     x 256 bytes, sized from W (112 pixels: 29 696 B per row), filled one row ahead by LDS-DMA -- slot 0 and W + 1 are the zero columns, rows -1 and H the
//     DMA's out-of-range reads; the 16-byte chunks of a slot are XOR-swizzled by (slot & 15);
//   * waves form a 4 (16-channel blocks) x 2 (halves of the row: 4 pixel fragments each) grid; a wave keeps the nine taps' fp16 AND correction weight fragments
//     of its 16 channels in registers (9 x 16 = 144 VGPRs) for the whole launch: nothing but the pixels passes through LDS;
//   * taps are shifted fragment reads (slot px + kx of ring row y + ky - 1), 36 groups per row step, each requested one group ahead of the MFMAs that consume it
//     into three register sets (the order pinned by sched_group_barrier: hipcc otherwise puts every read in front of its MFMA).  ds_read_b128 moves 256 B/clk
//     per CU, so the four channel-block waves' reads of a row equal its matrix work per SIMD; the bias is read back from LDS at every row start.
// Arithmetic: per output element conv_h8_kernel's chain -- the accumulator starts at the bias, takes the nine fp16 k-tiles in tap order (each as its two
// 32-deep halves, channels 0..31 then 32..63), then the nine correction k-tiles (one scaled fp8 MFMA each, the weight operand's E8M0 byte from the table), with
// the operand bytes in the lane and k positions of gemm_h8.hip's fragment reads (chunk fg / fg + 4 of the 128-byte k-tile row).  Same instructions, same
// operands, same order: the fp32 sums have that kernel's bits, and the epilogues apply pair_h8.h's functions to them as its epilogues do.
// MODE 0: fp32 rows [M, 64] (fnet; the moments are the caller's: raft_enc.hip); MODE 1: relu(.) as a pair row; MODE 2: relu(resid + relu(.)), resid an f16c8
// pair, as a pair row.  Pair rows are f16c8 or (out_bf16) bf16 pairs.  A lane's accumulator holds four consecutive channels of one pixel -- the group
// h8_split4 / pair_split4 take -- so the rows are stored from the accumulators.
// ---------------------------------------------------------------------------------------
constexpr int L1_R = 4;                    // ring rows: y - 1, y, y + 1 and the row in flight
constexpr int L1_MAX_W = 112;
constexpr int L1_READ_SPAN = 130 * 256;    // a fragment read reaches slot 127 + 2 of its ring row, whatever W is (results of pixels >= W are not stored)
typedef int l1_i32x4 __attribute__((ext_vector_type(4)));
typedef int l1_i32x8 __attribute__((ext_vector_type(8)));
typedef _Float16 l1_f16x8 __attribute__((ext_vector_type(8)));

template <class F, int... G>
__device__ __forceinline__ void l1_static_for(std::integer_sequence<int, G...>, F&& f) { (f(std::integral_constant<int, G>{}), ...); }

struct Layer1H8Params {
    const char* in;        // [n_img * H * W, 256 bytes]
    const char* w;         // [64, 2304 bytes]: nine fp16 k-tiles of 128 bytes (tap order), then the nine correction k-tiles (ops.py h8_conv_pack)
    const float* bias;     // [64]
    const int* scale;      // the E8M0 byte of 2^-11 / sw
    float* out_f32;        // MODE 0
    char* out_pair;        // MODE 1, 2: [M, 256 bytes]
    const char* resid;     // MODE 2: f16c8 pair rows [M, 256 bytes]
    int n_img, H, W, out_bf16;
    int parts, rows_per_part, row_bytes;
};

template <int MODE, int OBF>
__global__ __launch_bounds__(512) void layer1_h8_kernel(const Layer1H8Params p) {
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ __attribute__((aligned(16))) char ring[];
    const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, fg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave & 3, wm = wave >> 2;      // (the two row halves of a channel block share a SIMD: 4 + 3 fragments at W = 112)
    const int H = p.H, W = p.W, row_bytes = p.row_bytes;
    const int sc_w = *p.scale;

    // ---- this wave's weights: per tap the two 32-deep halves of the fp16 k-tile and the 64-byte halves of the correction k-tile, output channel 16 wn + fr
    l1_i32x4 wh[9][2];
    l1_i32x8 wc[9];
    {
        const char* const wrow = p.w + (wn * 16 + fr) * 2304 + fg * 16;
#pragma unroll
        for (int t = 0; t < 9; t++) {
            wh[t][0] = *reinterpret_cast<const l1_i32x4*>(wrow + t * 128);
            wh[t][1] = *reinterpret_cast<const l1_i32x4*>(wrow + t * 128 + 64);
            wc[t].lo = *reinterpret_cast<const l1_i32x4*>(wrow + (9 + t) * 128);
            wc[t].hi = *reinterpret_cast<const l1_i32x4*>(wrow + (9 + t) * 128 + 64);
        }
    }
    // the bias lives behind the ring (read back at every row start: four registers the read-ahead needs)
    float* const bias_s = reinterpret_cast<float*>(ring + (L1_R - 1) * row_bytes + L1_READ_SPAN);
    if (tid < 64) bias_s[tid] = p.bias[tid];
    __syncthreads();

    // ---- staging: a piece = 4 pixel slots x 256 bytes; wave w issues pieces w, w + 8, ..  Lane l of a piece: slot 4 piece + (l >> 4), LDS chunk position
    // l & 15 <- global chunk (l & 15) ^ (slot & 15) of pixel slot - 1; slots outside [1, W] read out of range (zeros)
    constexpr unsigned OOB = 0x80000000u;
    const int n_pieces = row_bytes >> 10;
    // (piece q * 8 + wave sits 32 slots = 8192 bytes behind piece wave, in LDS and in the image row, with the same swizzle term)
    const int dma_x = wave * 4 + (lane >> 4) - 1;
    const unsigned dma_off0 = (unsigned)(dma_x * 256 + (((lane & 15) ^ ((dma_x + 1) & 15)) << 4));
    // ---- fragment reads: pixel px = 64 wm + 16 jj + fr reads slot px + kx of ring row y + ky - 1: chunk fg of the fp16 half; its second 32-deep half and the
    // correction halves are chunks + 4, + 8, + 12 = byte ^ 64, ^ 128, ^ 192; fragment jj sits 16 slots = 4096 bytes further with the same swizzle term
    unsigned x_off[3];
#pragma unroll
    for (int kx = 0; kx < 3; kx++) {
        const int slot = wm * 64 + fr + kx;
        x_off[kx] = (unsigned)(slot * 256 + ((fg ^ (slot & 15)) << 4));
    }
    const int nj = W - wm * 64 >= 64 ? 4 : W - wm * 64 <= 0 ? 0 : (W - wm * 64 + 15) >> 4;      // this wave's fragments that hold pixels
    typedef __attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned u32x4_t;
    typedef __attribute__((__vector_size__(2 * sizeof(unsigned)))) unsigned u32x2_t;
    // byte offset of (pixel fragment jj, this lane's four channels) inside an output image row; pixels beyond the row store out of range
    constexpr int OPX = 256;                              // bytes per output pixel: 64 fp32 or a 128-unit pair row
    constexpr int OCH = MODE == 0 ? 4 : 2;
    const int px0 = wm * 64 + fr;                         // fragment jj: pixel px0 + 16 jj, 16 * OPX bytes further
    const unsigned o_off0 = (unsigned)(px0 * OPX + (wn * 16 + fg * 4) * OCH);

    const int n_units = p.n_img * p.parts;
    for (int unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
        const int img = unit / p.parts, y0 = (unit - img * p.parts) * p.rows_per_part;
        if (y0 >= H) continue;
        const int y1 = y0 + p.rows_per_part < H ? y0 + p.rows_per_part : H;
        const int64_t ioff = (int64_t)img * H * W * 256;
        const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(p.in + ioff), 0, H * W * 256, 0x00020000);
        const auto orsrc = __builtin_amdgcn_make_buffer_rsrc(MODE == 0 ? (void*)(reinterpret_cast<char*>(p.out_f32) + ioff) : (void*)(p.out_pair + ioff), 0, H * W * OPX, 0x00020000);
        const auto rrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>((MODE == 2 ? p.resid : p.in) + ioff), 0, H * W * 256, 0x00020000);
#define L1_ISSUE(yy)                                                                                                          \
        {                                                                                                                      \
            const int so_ = ((yy) >= 0 && (yy) < H) ? (yy) * W * 256 : 0x7FFFFF00;      /* rows -1 and H: out of range, zeros */  \
            char* const dst_ = ring + ((yy) & (L1_R - 1)) * row_bytes + wave * 1024;                                           \
            _Pragma("unroll") for (int q = 0; q < 4; q++)                                                                      \
                if (q * 8 + wave < n_pieces)                                                                                   \
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (c64_lptr_t)(dst_ + q * 8192), 16,                          \
                                                             (dma_x + q * 32 >= 0 && dma_x + q * 32 < W) ? dma_off0 + q * 8192u : OOB, so_, 0, 0); \
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);               // (my rows of the previous unit have landed / been stored)
        __builtin_amdgcn_s_barrier();                     // the previous unit's last rows have been consumed by every wave: the ring is free
        L1_ISSUE(y0 - 1)
        L1_ISSUE(y0)
        L1_ISSUE(y0 + 1)
        // One output row per step.  NJ: the wave's pixel fragments (3 for the second half of a 112-pixel row; waves with fewer run 4: what they read beyond
        // the row is inside the allocation and never stored).  NST stores per step, always issued, so the counted wait is exact: behind row y + 1 (requested one
        // step ago) only the previous step's stores are outstanding.
        auto step = [&](auto nj_c, const int y) {
            constexpr int NJ = decltype(nj_c)::value;
            constexpr int NST = (MODE == 0 ? 1 : 2) * NJ;
            if (y == y0) __builtin_amdgcn_s_waitcnt(0x0F70);
            else __builtin_amdgcn_s_waitcnt(0x0F70 | NST);
            __builtin_amdgcn_s_barrier();                 // everybody's pieces of row y + 1 are in LDS; everybody is done with row y - 2
            u32x2_t rh[NJ], rl[NJ];
            if constexpr (MODE == 2) {                    // the skip operand (requested BEFORE this step's DMA: vmcnt completes in order)
#pragma unroll
                for (int jj = 0; jj < NJ; jj++) {
                    const unsigned off = px0 + jj * 16 < W ? o_off0 + (unsigned)(jj * 16 * OPX + y * W * 256) : OOB;
                    rh[jj] = __builtin_bit_cast(u32x2_t, __builtin_amdgcn_raw_buffer_load_b64(rrsrc, off, 0, 0));
                    rl[jj] = __builtin_bit_cast(u32x2_t, __builtin_amdgcn_raw_buffer_load_b64(rrsrc, off != OOB ? off + 128u : OOB, 0, 0));
                }
            }
            L1_ISSUE(y + 2)
            f32x4 acc[NJ];
#pragma unroll
            for (int jj = 0; jj < NJ; jj++) acc[jj] = *reinterpret_cast<const f32x4*>(bias_s + wn * 16 + fg * 4);
            // 36 read groups of NJ fragment reads -- per tap the two 32-deep fp16 halves (groups 0..17), then per tap the two 64-byte halves of the
            // correction k-tile (18..35) -- each requested ONE group ahead of the MFMAs that consume it (left to itself hipcc put every read right in
            // front of its MFMA: lgkmcnt(0) per instruction).  fp16: NJ MFMAs per group; correction: NJ MFMAs per pair of groups.
            l1_i32x4 xg[3][NJ];                           // group g lives in set g % 3 (a correction batch reads two sets while the third is in flight)
#define L1_READ(g)                                                                                                             \
            {                                                                                                                  \
                constexpr int t_ = (g) < 18 ? (g) / 2 : ((g) - 18) / 2;                                                        \
                constexpr unsigned cx_ = (g) < 18 ? ((g) & 1) * 64u : 128u + ((g) & 1) * 64u;                                  \
                const char* const rowp_ = ring + ((y + t_ / 3 - 1) & (L1_R - 1)) * row_bytes;                                  \
                _Pragma("unroll") for (int jj = 0; jj < NJ; jj++)                                                              \
                    xg[(g) % 3][jj] = *reinterpret_cast<const l1_i32x4*>(rowp_ + (x_off[t_ % 3] ^ cx_) + jj * 4096);           \
            }
            L1_READ(0)
            __builtin_amdgcn_sched_barrier(0);
            l1_static_for(std::make_integer_sequence<int, 36>{}, [&](auto gc) {
                constexpr int g = decltype(gc)::value;
                if constexpr (g + 1 < 36) { L1_READ(g + 1) }
                if constexpr (g < 18) {             // the fp16 k-tile of tap g / 2: channels 0..31 (even g), then 32..63
#pragma unroll
                    for (int jj = 0; jj < NJ; jj++)
                        acc[jj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(l1_f16x8, wh[g / 2][g & 1]), __builtin_bit_cast(l1_f16x8, xg[g % 3][jj]), acc[jj], 0, 0, 0);
                } else if constexpr ((g & 1) != 0) {      // the correction k-tile of tap (g - 18) / 2: weights e4m3 (scaled by the table's byte), activations e5m2 (scale 1)
#pragma unroll
                    for (int jj = 0; jj < NJ; jj++) {
                        l1_i32x8 xc;
                        xc.lo = xg[(g - 1) % 3][jj]; xc.hi = xg[g % 3][jj];
                        acc[jj] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wc[(g - 18) / 2], xc, acc[jj], 0, 1, 0, sc_w, 0, 127);
                    }
                }
                // (pin the order inside the group: the next group's reads first -- hipcc otherwise sinks them below the MFMAs to reuse their registers)
                if constexpr (g + 1 < 36) __builtin_amdgcn_sched_group_barrier(0x100, NJ, 0);
                if constexpr (g < 18 || (g & 1) != 0) __builtin_amdgcn_sched_group_barrier(0x008, NJ, 0);
                __builtin_amdgcn_sched_barrier(0);
            });
#undef L1_READ
            // ---- epilogue: NST stores, always issued
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int jj = 0; jj < NJ; jj++) {
                const bool ok = px0 + jj * 16 < W;
                const unsigned off = ok ? o_off0 + (unsigned)(jj * 16 * OPX + y * W * OPX) : OOB;
                f32x4 v = acc[jj];
                if constexpr (MODE == 0) {
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v), orsrc, off, 0, 0);
                } else {
                    v = f32x4{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
                    if constexpr (MODE == 2) {
                        v += h8_join4(rh[jj], rl[jj]);
                        v = f32x4{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
                    }
                    u32x2_t hu, lu;
                    if constexpr (OBF) {
                        bf16x4 hi, lo;
                        pair_split4(v, hi, lo);
                        hu = __builtin_bit_cast(u32x2_t, hi); lu = __builtin_bit_cast(u32x2_t, lo);
                    } else {
                        h8_split4(v, hu, lu);
                    }
                    __builtin_amdgcn_raw_buffer_store_b64(hu, orsrc, off, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b64(lu, orsrc, ok ? off + 128u : OOB, 0, 0);      // the second half: 64 units further
                }
            }
        };
        if (nj == 3) {
            for (int y = y0; y < y1; y++) step(std::integral_constant<int, 3>{}, y);
        } else {
            for (int y = y0; y < y1; y++) step(std::integral_constant<int, 4>{}, y);
        }
#undef L1_ISSUE
    }
#endif
}

}   // namespace

// x [n_img, H, W, 64] bf16 -> 3x3 / stride 1 / pad 1 convolution with w [64, 576] (+ bias): fp32 [.., 64] + moments (out_f32 != NULL) or bf16
bool conv3x3_c64_supported(int H, int W) { return W >= 16 && W <= C64_RS - 2 && H >= 1; }

size_t conv64_stats_part_floats(int n_img) { return ((size_t)n_img + 4 * (size_t)cu_count()) * 2 * 64 * 2; }   // n_img * parts < 2 * (n_img + 4 CUs)

int launch_conv3x3_c64(const void* in, const void* w, const float* bias, float* out_f32, float* stats, float* stats_part, void* out_bf16, const void* resid,
                       int n_img, int H, int W, int relu, int post_relu, hipStream_t s) {
    VTGB_REQUIRE(conv3x3_c64_supported(H, W), VTGB_EUNSUPPORTED, "conv3x3_c64: W=%d outside [16, %d]", W, C64_RS - 2);
    VTGB_REQUIRE((int64_t)H * W * 128 < 0x7FFFFF00ll, VTGB_EUNSUPPORTED, "conv3x3_c64: image too large");
    Conv64Params p;
    p.in = (const bf16_t*)in; p.w = (const bf16_t*)w; p.bias = bias; p.out_f32 = out_f32; p.stats = stats; p.stats_part = stats_part; p.out_bf16 = (bf16_t*)out_bf16;
    p.resid = (const bf16_t*)resid; p.n_img = n_img; p.H = H; p.W = W; p.relu = relu; p.post_relu = post_relu;
    // runs of rows: enough of them that the persistent grid is balanced (>= 4 per workgroup), each an even number of rows
    int parts = 1;
    while ((int64_t)n_img * parts < 4 * cu_count() && H / (parts * 2) >= 8) parts *= 2;
    p.rows_per_part = 2 * ((H + 2 * parts - 1) / (2 * parts));
    p.parts = (H + p.rows_per_part - 1) / p.rows_per_part;
    const int64_t units = (int64_t)n_img * p.parts;
    const int grid = units < cu_count() ? (int)units : cu_count();
    if (out_f32 && p.parts > 1) VTGB_REQUIRE(stats_part && (size_t)units * 128 <= conv64_stats_part_floats(n_img), VTGB_EINVAL, "conv3x3_c64: partial-moment scratch missing");
    const double flops = 2.0 * n_img * H * W * 64.0 * 576.0;
    ProfScope prof(VTGB_PROF_CONV, flops, s, flops);
    static DeviceOnce a0, a1;
    if (out_f32) {
        VTGB_REQUIRE(stats, VTGB_EINVAL, "conv3x3_c64: fp32 output needs the moments buffer");
        VTGB_FUNC_LDS_ONCE(a0, conv3x3_c64_kernel<0>, C64_LDS);
        hipLaunchKernelGGL(conv3x3_c64_kernel<0>, dim3(grid), dim3(512), C64_LDS, s, p);
        if (p.parts > 1) VTGB_TRY(launch_stats_finish_parts(stats_part, stats, n_img, p.parts, 64, s));
    } else {
        VTGB_FUNC_LDS_ONCE(a1, conv3x3_c64_kernel<1>, C64_LDS);
        hipLaunchKernelGGL(conv3x3_c64_kernel<1>, dim3(grid), dim3(512), C64_LDS, s, p);
    }
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

// the stem on raw frames: img [n_img, 3, H, W] fp32 -> [n_img, H/2, W/2, 64]; packed weights [64, 512] (vtgb.h: vtgb_raft_encoder), x3: the
// bf16x3 table's [64, 768]; out16: bf16 rows (relu; bf16 form) or pair rows (relu; x3 form, h8: f16c8 instead of bf16 pairs)
bool stem7x7_supported(int H, int W) { return (H % 2) == 0 && (W % 2) == 0 && W / 2 >= 16 && W / 2 <= 112 && H / 2 >= 4; }

static int stem7x7_launch(bool x3, const float* img, const void* w, const float* bias, float* out_f32, float* stats, float* stats_part, void* out16, int h8, int n_img,
                          int H, int W, int relu, hipStream_t s) {
    VTGB_REQUIRE(stem7x7_supported(H, W), VTGB_EUNSUPPORTED, "stem7x7: %d x %d unsupported", H, W);
    const int H2 = H / 2, W2 = W / 2;
    VTGB_REQUIRE((int64_t)H2 * W2 * 256 < 0x7FFFFF00ll, VTGB_EUNSUPPORTED, "stem7x7: image too large");
    StemParams p;
    p.img = img; p.w = (const bf16_t*)w; p.bias = bias; p.out_f32 = out_f32; p.stats = stats; p.stats_part = stats_part; p.out_bf16 = (bf16_t*)out16;
    p.n_img = n_img; p.H = H; p.W = W; p.relu = relu; p.h8 = h8;
    int parts = 1;
    while ((int64_t)n_img * parts < 4 * cu_count() && H2 / (parts * 2) >= 14) parts *= 2;
    p.rows_per_part = (H2 + parts - 1) / parts;
    p.parts = (H2 + p.rows_per_part - 1) / p.rows_per_part;
    const int64_t units = (int64_t)n_img * p.parts;
    const int grid = units < cu_count() ? (int)units : cu_count();
    if (out_f32 && stats && p.parts > 1)
        VTGB_REQUIRE(stats_part && (size_t)units * 128 <= conv64_stats_part_floats(n_img), VTGB_EINVAL, "stem7x7: partial-moment scratch missing");
    const int lds = ST_R * W2 * 256 + 8 * 32 * 2 * 4 + 64 * 4;
    constexpr int lds_max = ST_R * 112 * 256 + 8 * 32 * 2 * 4 + 64 * 4;
    const double flops = 2.0 * n_img * H2 * W2 * 64.0 * 147.0, exec = 2.0 * n_img * H2 * W2 * 64.0 * (x3 ? 768.0 : 512.0);
    ProfScope prof(VTGB_PROF_CONV, flops, s, exec);
    static DeviceOnce a0, a1, a2, a3;
    if (out_f32) {
        VTGB_REQUIRE(stats || x3, VTGB_EINVAL, "stem7x7: fp32 output needs the moments buffer");      // (x3: NULL = rows only)
        if (x3) {
            VTGB_FUNC_LDS_ONCE(a2, (stem7x7_kernel<0, true>), lds_max);
            hipLaunchKernelGGL((stem7x7_kernel<0, true>), dim3(grid), dim3(512), lds, s, p);
        } else {
            VTGB_FUNC_LDS_ONCE(a0, (stem7x7_kernel<0, false>), lds_max);
            hipLaunchKernelGGL((stem7x7_kernel<0, false>), dim3(grid), dim3(512), lds, s, p);
        }
        if (stats && p.parts > 1) VTGB_TRY(launch_stats_finish_parts(stats_part, stats, n_img, p.parts, 64, s));
    } else if (x3) {
        VTGB_FUNC_LDS_ONCE(a3, (stem7x7_kernel<2, true>), lds_max);
        hipLaunchKernelGGL((stem7x7_kernel<2, true>), dim3(grid), dim3(512), lds, s, p);
    } else {
        VTGB_FUNC_LDS_ONCE(a1, (stem7x7_kernel<1, false>), lds_max);
        hipLaunchKernelGGL((stem7x7_kernel<1, false>), dim3(grid), dim3(512), lds, s, p);
    }
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

int launch_stem7x7(const float* img, const void* w, const float* bias, float* out_f32, float* stats, float* stats_part, void* out_bf16, int n_img, int H, int W,
                   int relu, hipStream_t s) {
    return stem7x7_launch(false, img, w, bias, out_f32, stats, stats_part, out_bf16, 0, n_img, H, W, relu, s);
}
// the split-operand form: fp32 rows + moments (out_f32; fnet) or relu(.) as pair rows (out_pair; cnet)
int launch_stem7x7_x3(const float* img, const void* w, const float* bias, float* out_f32, float* stats, float* stats_part, void* out_pair, int h8, int n_img, int H,
                      int W, hipStream_t s) {
    VTGB_REQUIRE((out_f32 != nullptr) != (out_pair != nullptr), VTGB_EINVAL, "stem7x7 x3: exactly one of the fp32 rows and the pair rows");
    return stem7x7_launch(true, img, w, bias, out_f32, stats, stats_part, out_pair, h8, n_img, H, W, out_pair ? 1 : 0, s);
}

// layer1 at VTGB_F16C8 with the rows resident: x = f16c8 pair rows [n_img * H * W, 128 units], w [64, 1152 units] + scale byte (the encoder table's entries).
// Exactly one output: out_f32 (fp32 rows [M, 64]) or out_pair (relu(.), or relu(resid + relu(.)) with an f16c8 pair `resid`, as f16c8 or bf16 pair rows).
// Every element has launch_conv_h8's bits (layer1_h8_kernel).
bool layer1_h8_supported(int H, int W) { return W >= 16 && W <= L1_MAX_W && H >= 4 && (int64_t)H * W * 256 < 0x7FFFFF00ll; }

int launch_layer1_h8(const void* in, const void* w, const float* bias, const int* scale, float* out_f32, void* out_pair, const void* resid, int out_bf16, int n_img, int H,
                     int W, hipStream_t s) {
    VTGB_REQUIRE(n_img > 0 && layer1_h8_supported(H, W), VTGB_EUNSUPPORTED, "layer1_h8: %d images of %d x %d outside 16 <= W <= %d, H >= 4", n_img, H, W, L1_MAX_W);
    VTGB_REQUIRE(in && w && bias && scale && ((out_f32 != nullptr) != (out_pair != nullptr)) && (!resid || out_pair) && (!out_bf16 || resid), VTGB_EINVAL,
                 "layer1_h8: operands, the scale byte and exactly one of the fp32 rows and the pair rows (resid belongs to pair rows, bf16 pairs to the residual tail)");
    Layer1H8Params p;
    p.in = (const char*)in; p.w = (const char*)w; p.bias = bias; p.scale = scale; p.out_f32 = out_f32; p.out_pair = (char*)out_pair; p.resid = (const char*)resid;
    p.n_img = n_img; p.H = H; p.W = W; p.out_bf16 = out_bf16;
    p.row_bytes = ((W + 2 + 3) / 4) * 1024;
    // runs of rows: enough of them that the persistent grid is balanced (>= 4 per workgroup); a run re-stages two halo rows
    int parts = 1;
    while ((int64_t)n_img * parts < 4 * cu_count() && H / (parts * 2) >= 7) parts *= 2;
    p.rows_per_part = (H + parts - 1) / parts;
    p.parts = (H + p.rows_per_part - 1) / p.rows_per_part;
    const int64_t units = (int64_t)n_img * p.parts;
    const int grid = units < cu_count() ? (int)units : cu_count();
    const int lds = (L1_R - 1) * p.row_bytes + L1_READ_SPAN + 256;      // + the bias
    constexpr int lds_max = (L1_R - 1) * ((L1_MAX_W + 2 + 3) / 4) * 1024 + L1_READ_SPAN + 256;
    const double flops = 2.0 * n_img * H * W * 64.0 * 576.0;
    ProfScope prof(VTGB_PROF_CONV, flops, s, 2.0 * flops);      // (in fp16-MFMA units: an fp8 k-tile takes the matrix-pipe cycles of an fp16 one)
    static DeviceOnce a0, a1, a2, a3;
    if (out_f32) {
        VTGB_FUNC_LDS_ONCE(a0, (layer1_h8_kernel<0, 0>), lds_max);
        hipLaunchKernelGGL((layer1_h8_kernel<0, 0>), dim3(grid), dim3(512), lds, s, p);
    } else if (!resid) {
        VTGB_FUNC_LDS_ONCE(a1, (layer1_h8_kernel<1, 0>), lds_max);
        hipLaunchKernelGGL((layer1_h8_kernel<1, 0>), dim3(grid), dim3(512), lds, s, p);
    } else if (!out_bf16) {
        VTGB_FUNC_LDS_ONCE(a2, (layer1_h8_kernel<2, 0>), lds_max);
        hipLaunchKernelGGL((layer1_h8_kernel<2, 0>), dim3(grid), dim3(512), lds, s, p);
    } else {
        VTGB_FUNC_LDS_ONCE(a3, (layer1_h8_kernel<2, 1>), lds_max);
        hipLaunchKernelGGL((layer1_h8_kernel<2, 1>), dim3(grid), dim3(512), lds, s, p);
    }
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}
