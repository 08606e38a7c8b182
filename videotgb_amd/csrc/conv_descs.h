// conv_descs.h -- the GemmDesc builders of RAFT's convolution launches, shared by the translation units that launch them (raft.hip: conv_desc,
// raft_enc.hip: enc_conv, raft_x3.hip: x3_conv) and by the unit-level entry vtgb_conv_launch (raft_x3.hip), which therefore runs the descriptors
// the production callers build and not a restatement of them.
#pragma once
#include <string.h>

#include "common.h"

// update block at VTGB_BF16 / VTGB_F32 (raft.hip): Cin channels, the first `split` of them from A (row stride lda), the rest from A2 (lda2).
// KH == 0: a plain GEMM through the same kernels (the caller sets K and ldw)
static inline GemmDesc conv_desc(int dt, int M, int N, int H, int W, int KH, int KW, int Cin, int split, const void* A, int64_t lda, const void* A2,
                                 int64_t lda2, const void* Wt, const float* bias, int epi, int act, void* out, int64_t ldo, const void* zero) {
    GemmDesc d;
    memset(&d, 0, sizeof(d));
    d.dtype = dt; d.M = M; d.N = N; d.K = KH * KW * Cin; d.epi = epi; d.act = act;
    d.A = A; d.lda = lda; d.A2 = A2; d.lda2 = lda2; d.W = Wt; d.ldw = d.K; d.bias = bias; d.out = out; d.ldo = ldo;
    d.conv_H = H; d.conv_W = W; d.conv_KH = KH; d.conv_KW = KW; d.conv_Cin = Cin; d.conv_split = split; d.zero_page = zero;
    return d;
}

// encoders (raft_enc.hip): K x K, stride 1 or 2 over an Hi x Wi input grid, fp32 rows out (+ the per-tile moments into col_stats).
// VTGB_BF16X3: the input is a pair row [hi(Cin) | lo(Cin)] contracted as [hi | lo | hi] against weights packed [Wh | Wh | Wl] (raft_x3.hip)
static inline GemmDesc enc_conv(int dt, int Mo, int N, int Ho, int Wo, int K, int Cin, int stride, int Hi, int Wi, const void* A, const void* Wt, const float* bias,
                                float* out, int ldo, const void* zero, float* col_stats) {
    GemmDesc d;
    memset(&d, 0, sizeof(d));
    const bool x3 = dt == VTGB_BF16X3;
    const int Ce = x3 ? 3 * Cin : Cin;
    d.dtype = x3 ? VTGB_BF16 : dt; d.M = Mo; d.N = N; d.K = K * K * Ce; d.epi = VTGB_EPI_STORE_F32;
    d.A = A; d.lda = x3 ? 2 * Cin : Cin; d.W = Wt; d.ldw = d.K; d.bias = bias; d.out = out; d.ldo = ldo;
    d.conv_H = Ho; d.conv_W = Wo; d.conv_KH = K; d.conv_KW = K; d.conv_Cin = Ce; d.conv_split = Ce; d.conv_wrap = x3 ? 2 * Cin : 0;
    d.conv_stride = stride; d.conv_Hi = Hi; d.conv_Wi = Wi; d.zero_page = zero;
    d.col_stats = col_stats; d.stats_rows = Ho * Wo;
    if (x3) d.algo_flops = 2.0 * Mo * (double)N * (K * K * Cin);
    return d;
}
// the encoders' stem: enc_conv's 1 x 1 descriptor widened to the 4 x 1 convolution over the packed (space-to-depth) rows
static inline GemmDesc enc_stem_conv(int dt, int Mo, int N, int Ho, int Wo, int Cin, const void* A, const void* Wt, const float* bias, float* out, int ldo,
                                     const void* pad_page, float* col_stats) {
    GemmDesc d = enc_conv(dt, Mo, N, Ho, Wo, 1, Cin, 1, Ho, Wo, A, Wt, bias, out, ldo, pad_page, col_stats);
    d.conv_KH = 4; d.K = 4 * d.conv_Cin; d.ldw = d.K;
    return d;
}

// update block at VTGB_BF16X3 (raft_x3.hip): a convolution over pair operands: C1 channels from A (row [hi(C1) | lo(C1)]), optionally C2 more from A2;
// K = taps * 3 (C1 + C2)
static inline GemmDesc x3_conv(int M, int N, int H, int W, int KH, int KW, const void* A, int C1, const void* A2, int C2, const void* Wt, const float* bias, int epi,
                               int act, void* out, int64_t ldo, int split_lo, const void* zero) {
    GemmDesc d;
    memset(&d, 0, sizeof(d));
    const int Cin = 3 * (C1 + C2);
    d.dtype = VTGB_BF16; d.M = M; d.N = N; d.K = KH * KW * Cin; d.epi = epi; d.act = act;
    d.A = A; d.lda = 2 * C1; d.A2 = A2; d.lda2 = 2 * C2; d.W = Wt; d.ldw = d.K; d.bias = bias; d.out = out; d.ldo = ldo; d.split_lo = split_lo;
    d.conv_H = H; d.conv_W = W; d.conv_KH = KH; d.conv_KW = KW; d.conv_Cin = Cin; d.conv_split = 3 * C1; d.conv_wrap = 2 * C1; d.conv_wrap2 = 2 * C2;
    d.zero_page = zero;
    d.algo_flops = 2.0 * M * (double)N * (KH * KW * (C1 + C2));      // the fp32 convolution this launch stands for (executed: 3 x)
    return d;
}
