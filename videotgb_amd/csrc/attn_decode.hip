// attn_decode.hip -- split-KV ("flash-decoding") single-query attention over the static K/V cache of the decode step, for caches the
// one-wave-per-head kernel of llm.hip cannot hold (its scores live in LDS: 2048 keys) or serves badly (8 workgroups at batch 1).
// Two launches, no atomics:
//
// Pass 1, llm_decode_attn_split_kernel.  Grid (key chunk, K/V head x query-head block, batch row), fixed by tmax, so one captured graph
// serves every step: a workgroup whose chunk starts past *pos leaves after reading *pos.  A chunk is DEC_SPLIT_CHUNK = 256 keys, 64 per
// wave.  A wave holds its 64 K rows in registers -- 16-byte loads, consecutive lanes on consecutive 16-byte pieces of a row, so one load
// instruction reads 64 / LPR whole rows (LPR = lanes per row = hd * sizeof(T) / 16) -- and every query head of the block (at most
// DEC_SPLIT_HEADS = 8 heads of ONE K/V head; a larger nq / nkv takes more blocks) takes its scores from those registers; the V rows then
// replace them and serve every head again.  K/V are read once per group of query heads, in place from [B, nkv, tmax, hd].
// Per (row, query head, chunk) the workgroup leaves fp32 partials in the workspace: m = the largest scaled score of the chunk's visible
// keys (-inf: none), l = sum exp(s - m), O[hd] = sum exp(s - m) v.  A key is visible if key <= *pos (and key_valid[b, key] != 0, MASKED);
// nothing past *pos is read, and the K and V values of any other key are replaced by zeros before any product -- its score is -inf, its weight
// exactly 0 --, so what a pad slot or the cache past *pos holds (NaN included) cannot reach an output.
//
// Pass 2, llm_decode_attn_combine_kernel.  Per (row, query head): M = max_c m_c, w_c = exp(m_c - M), out = (sum_c w_c O_c) / (sum_c w_c l_c)
// over the chunks 0 .. *pos / 256 in ascending order, rounded once to T.  A chunk without a visible key (m_c = -inf) is skipped: weight 0,
// no exp(-inf - -inf).  No visible key at all: a zero row.
//
// Determinism.  Which keys share a partial sum (chunk = key / 256, wave = key / 64 % 4, a lane's keys = key % (64 / LPR)) and the order
// inside every sum depend on the key index, T and hd alone -- not on B, tmax, the grid, the number of query heads per K/V head or which
// heads share a workgroup (a head's arithmetic never sees another head's values).  An invisible key adds an exact +0.  So a row's output
// is a function of (q, K/V[0..*pos], key_valid[0..*pos]): the same bits in any batch, any cache length, grouped or replicated K/V.
#include "common.h"
#include "fp8_code.h"

#include <math.h>

constexpr int DEC_SPLIT_CHUNK = 256;      // keys per workgroup: 4 waves x 64
constexpr int DEC_SPLIT_HEADS = 8;        // query heads per workgroup (of one K/V head)
constexpr int DEC_SPLIT_MAX_T = 16384;

// v + (v of lane ^ MASK): MASK < 16 on the VALU (DPP, inside a row of 16 lanes), else through the LDS crossbar.  Both lanes of a pair
// compute the same sum (a + b == b + a), so after the steps MASK = 1, 2, 4 ... every lane of the group holds the group's total.
template <int MASK>
__device__ __forceinline__ float add_xor(float v) {
    if constexpr (MASK == 1 || MASK == 2) {
        constexpr int ctrl = MASK == 1 ? 0xB1 : 0x4E;      // quad_perm [1,0,3,2] / [2,3,0,1]
        return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, 0xF, 0xF, false));
    } else {
        return v + __shfl_xor(v, MASK);
    }
}

template <int W>      // sum over aligned groups of W lanes (W a power of two <= 64)
__device__ __forceinline__ float group_sum(float v) {
    if constexpr (W > 1) v = add_xor<1>(v);
    if constexpr (W > 2) v = add_xor<2>(v);
    if constexpr (W > 4) v = add_xor<4>(v);
    if constexpr (W > 8) v = add_xor<8>(v);
    if constexpr (W > 16) v = add_xor<16>(v);
    if constexpr (W > 32) v = add_xor<32>(v);
    return v;
}

template <typename T, int HD, bool MASKED>
__global__ __launch_bounds__(256) void llm_decode_attn_split_kernel(const T* __restrict__ q, const T* __restrict__ kc, const T* __restrict__ vc,
                                                                    float* __restrict__ ws, const int64_t* __restrict__ pos_p,
                                                                    const uint8_t* __restrict__ key_valid, int B, int nq, int nkv, int tmax,
                                                                    float scale) {
    constexpr int EPL = 16 / (int)sizeof(T);      // elements per lane: one 16-byte piece of a row
    constexpr int LPR = HD / EPL;                 // lanes per row
    constexpr int RPI = 64 / LPR;                 // rows per load instruction
    constexpr int NI = 64 / RPI;                  // load instructions per wave (== LPR)
    typedef T TV __attribute__((ext_vector_type(EPL)));
    __shared__ float qs[DEC_SPLIT_HEADS][HD];
    __shared__ float sc[DEC_SPLIT_HEADS][DEC_SPLIT_CHUNK];
    __shared__ __attribute__((aligned(16))) float red[4][DEC_SPLIT_HEADS][HD];

    const int chunk = blockIdx.x, b = blockIdx.z;
    const int pos = min((int)(*pos_p), tmax - 1);
    if (chunk * DEC_SPLIT_CHUNK > pos) return;
    const int group = nq / nkv, nhb = (group + DEC_SPLIT_HEADS - 1) / DEC_SPLIT_HEADS;
    const int kvh = blockIdx.y / nhb, hb = blockIdx.y % nhb;
    const int head0 = kvh * group + hb * DEC_SPLIT_HEADS, nh = min(DEC_SPLIT_HEADS, group - hb * DEC_SPLIT_HEADS);
    const int nc = (tmax + DEC_SPLIT_CHUNK - 1) / DEC_SPLIT_CHUNK;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane % LPR, rs = lane / LPR;      // this lane's 16-byte piece and row slot

    for (int i = tid; i < nh * HD; i += 256) qs[i / HD][i % HD] = (float)q[((int64_t)b * nq + head0) * HD + i];

    // ---- K: the wave's 64 rows -> registers (row kl0 + i * RPI of instruction i); invisible rows stay zeros
    const int kl0 = wave * 64 + rs, key0 = chunk * DEC_SPLIT_CHUNK + kl0;
    const int64_t base = ((int64_t)b * nkv + kvh) * tmax * HD + c * EPL;
    const uint8_t* kvr = MASKED ? key_valid + (int64_t)b * tmax : nullptr;
    unsigned vis = 0;
#pragma unroll
    for (int i = 0; i < NI; i++) {
        const int key = key0 + i * RPI;
        bool ok = key <= pos;
        if (MASKED && ok) ok = kvr[key] != 0;
        vis |= ok ? 1u << i : 0u;
    }
    // No branch per row: an invisible row's load goes to row *pos (in bounds, one row for the whole grid) and its value is selected away,
    // so all NI loads are in flight together and nothing a pad slot holds reaches a product.
    TV zero;
#pragma unroll
    for (int e = 0; e < EPL; e++) zero[e] = (T)0.f;
    auto load_rows = [&](const T* __restrict__ src, TV (&reg)[NI]) {
#pragma unroll
        for (int i = 0; i < NI; i++) {
            const bool ok = vis >> i & 1;
            const TV v = *reinterpret_cast<const TV*>(src + base + (int64_t)(ok ? key0 + i * RPI : pos) * HD);
            reg[i] = ok ? v : zero;
        }
    };
    TV reg[NI];
    load_rows(kc, reg);
    __syncthreads();      // qs

    // ---- scores: per head, the lane's piece of every row, then the row's LPR lanes
    for (int h = 0; h < nh; h++) {
        float qv[EPL];
#pragma unroll
        for (int e = 0; e < EPL; e++) qv[e] = qs[h][c * EPL + e];
#pragma unroll
        for (int i = 0; i < NI; i++) {
            float dot = 0.f;
#pragma unroll
            for (int e = 0; e < EPL; e++) dot = fmaf(qv[e], (float)reg[i][e], dot);
            dot = group_sum<LPR>(dot);
            if (c == 0) sc[h][kl0 + i * RPI] = (vis >> i & 1) ? dot * scale : -INFINITY;
        }
    }
    // ---- V replaces K in the registers (the loads fly behind the softmax)
    load_rows(vc, reg);
    __syncthreads();      // sc

    // ---- softmax statistics of the chunk: wave w takes the heads w, w + 4
    for (int h = wave; h < nh; h += 4) {
        float s[4], m = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            s[j] = sc[h][lane + 64 * j];
            m = fmaxf(m, s[j]);
        }
        for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
#pragma unroll
        for (int j = 0; j < 4; j++) {
            s[j] = s[j] == -INFINITY ? 0.f : expf(s[j] - m);      // (an invisible key: exactly 0, also when the chunk has no visible key)
            sc[h][lane + 64 * j] = s[j];
        }
        const float l = group_sum<64>((s[0] + s[1]) + (s[2] + s[3]));
        if (lane == 0) {
            float* ml = ws + (int64_t)B * nq * nc * HD + (((int64_t)b * nq + head0 + h) * nc + chunk) * 2;
            ml[0] = m;
            ml[1] = l;
        }
    }
    __syncthreads();      // sc = weights

    // ---- O: per head, the lane's rows in ascending order, then the wave's row slots, then (below) the four waves
    for (int h = 0; h < nh; h++) {
        float acc[EPL];
#pragma unroll
        for (int e = 0; e < EPL; e++) acc[e] = 0.f;
#pragma unroll
        for (int i = 0; i < NI; i++) {
            const float p = sc[h][kl0 + i * RPI];
#pragma unroll
            for (int e = 0; e < EPL; e++) acc[e] = fmaf(p, (float)reg[i][e], acc[e]);
        }
#pragma unroll
        for (int e = 0; e < EPL; e++) {
            float v = acc[e];
            if constexpr (RPI > 1) v += __shfl_xor(v, LPR);
            if constexpr (RPI > 2) v += __shfl_xor(v, 2 * LPR);
            if constexpr (RPI > 4) v += __shfl_xor(v, 4 * LPR);
            acc[e] = v;
        }
        if (rs == 0) {
#pragma unroll
            for (int e = 0; e < EPL; e += 4)
                *reinterpret_cast<f32x4*>(&red[wave][h][c * EPL + e]) = f32x4{acc[e], acc[e + 1], acc[e + 2], acc[e + 3]};
        }
    }
    __syncthreads();      // red
    for (int i = tid; i < nh * HD; i += 256) {
        const int h = i / HD, d = i % HD;
        ws[(((int64_t)b * nq + head0 + h) * nc + chunk) * HD + d] = ((red[0][h][d] + red[1][h][d]) + red[2][h][d]) + red[3][h][d];
    }
}

// One workgroup of hd threads per (row, query head).
template <typename T>
__global__ __launch_bounds__(128) void llm_decode_attn_combine_kernel(const float* __restrict__ ws, T* __restrict__ out, const int64_t* __restrict__ pos_p,
                                                                      int64_t rows, int hd, int tmax) {
    const int64_t row = blockIdx.x;
    const int d = threadIdx.x;
    const int nc = (tmax + DEC_SPLIT_CHUNK - 1) / DEC_SPLIT_CHUNK;
    const int pos = min((int)(*pos_p), tmax - 1);
    const int n = pos < 0 ? 0 : pos / DEC_SPLIT_CHUNK + 1;
    const float* O = ws + row * nc * hd + d;
    const float* ml = ws + rows * nc * hd + row * nc * 2;
    float M = -INFINITY;
    for (int ch = 0; ch < n; ch++) M = fmaxf(M, ml[2 * ch]);
    float num = 0.f, den = 0.f;
    for (int ch = 0; ch < n; ch++) {
        const float m = ml[2 * ch];
        if (m == -INFINITY) continue;      // no visible key in this chunk: weight 0
        const float w = expf(m - M);
        num = fmaf(w, O[(int64_t)ch * hd], num);
        den = fmaf(w, ml[2 * ch + 1], den);
    }
    out[row * hd + d] = (T)(den > 0.f ? num / den : 0.f);
}

template <typename T, int HD>
static int launch_split(const void* q, const void* kc, const void* vc, void* out, const int64_t* pos, const uint8_t* key_valid, void* workspace,
                        int B, int nq, int nkv, int tmax, float scale, hipStream_t s) {
    const int group = nq / nkv, nhb = (group + DEC_SPLIT_HEADS - 1) / DEC_SPLIT_HEADS, nc = (tmax + DEC_SPLIT_CHUNK - 1) / DEC_SPLIT_CHUNK;
    const dim3 grid(nc, nkv * nhb, B);
    float* ws = (float*)workspace;
    if (key_valid)
        hipLaunchKernelGGL((llm_decode_attn_split_kernel<T, HD, true>), grid, dim3(256), 0, s, (const T*)q, (const T*)kc, (const T*)vc, ws, pos, key_valid,
                           B, nq, nkv, tmax, scale);
    else
        hipLaunchKernelGGL((llm_decode_attn_split_kernel<T, HD, false>), grid, dim3(256), 0, s, (const T*)q, (const T*)kc, (const T*)vc, ws, pos,
                           (const uint8_t*)nullptr, B, nq, nkv, tmax, scale);
    VTGB_HIP(hipGetLastError());
    hipLaunchKernelGGL(llm_decode_attn_combine_kernel<T>, dim3((unsigned)((int64_t)B * nq)), dim3(HD), 0, s, (const float*)ws, (T*)out, pos,
                       (int64_t)B * nq, HD, tmax);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

extern "C" int64_t vtgb_llm_decode_attention_split_workspace_bytes(int32_t B, int32_t nq, int32_t hd, int32_t tmax) {
    if (B <= 0 || nq <= 0 || hd <= 0 || tmax <= 0) return 0;
    const int64_t nc = (tmax + DEC_SPLIT_CHUNK - 1) / DEC_SPLIT_CHUNK;
    return (int64_t)B * nq * nc * (hd + 2) * (int64_t)sizeof(float);
}

extern "C" int vtgb_llm_decode_attention_split(int dtype, const void* q, const void* kc, const void* vc, void* out, const int64_t* pos,
                                               const uint8_t* key_valid, void* workspace, int32_t B, int32_t nq, int32_t nkv, int32_t hd,
                                               int32_t tmax, float scale, vtgb_stream_t stream) {
    VTGB_REQUIRE(q && kc && vc && out && pos && workspace, VTGB_EINVAL, "llm_decode_attention_split: NULL operand");
    VTGB_REQUIRE((dtype == VTGB_BF16 || dtype == VTGB_F32) && B > 0 && nq > 0 && nkv > 0 && tmax > 0, VTGB_EINVAL,
                 "llm_decode_attention_split: bad argument");
    VTGB_REQUIRE(nq % nkv == 0, VTGB_EINVAL, "llm_decode_attention_split: nq=%d is not a multiple of nkv=%d", nq, nkv);
    VTGB_REQUIRE(hd == 64 || hd == 128, VTGB_EUNSUPPORTED, "llm_decode_attention_split: hd=%d, built for 64 and 128", hd);
    VTGB_REQUIRE(tmax % 64 == 0 && tmax <= DEC_SPLIT_MAX_T, VTGB_EUNSUPPORTED, "llm_decode_attention_split: tmax=%d is not a multiple of 64 up to %d",
                 tmax, DEC_SPLIT_MAX_T);
    const int nhb = (nq / nkv + DEC_SPLIT_HEADS - 1) / DEC_SPLIT_HEADS;
    VTGB_REQUIRE(B <= 65535 && (int64_t)nkv * nhb <= 65535, VTGB_EUNSUPPORTED, "llm_decode_attention_split: B=%d / nq=%d exceed the grid", B, nq);
    const auto misaligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; };
    VTGB_REQUIRE(!misaligned(q) && !misaligned(kc) && !misaligned(vc) && !misaligned(out) && !misaligned(workspace), VTGB_EUNSUPPORTED,
                 "llm_decode_attention_split: q / kc / vc / out / workspace need 16-byte alignment");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == VTGB_BF16)
        return hd == 128 ? launch_split<bf16_t, 128>(q, kc, vc, out, pos, key_valid, workspace, B, nq, nkv, tmax, scale, s)
                         : launch_split<bf16_t, 64>(q, kc, vc, out, pos, key_valid, workspace, B, nq, nkv, tmax, scale, s);
    return hd == 128 ? launch_split<float, 128>(q, kc, vc, out, pos, key_valid, workspace, B, nq, nkv, tmax, scale, s)
                     : launch_split<float, 64>(q, kc, vc, out, pos, key_valid, workspace, B, nq, nkv, tmax, scale, s);
}

// ---- fp8 K/V cache (opt-in: kv_cache="fp8").  The cache of a layer is e4m3 codes kc8 / vc8 [B, nkv, tmax, hd] (uint8) and one power-of-two
// scale per row ks / vs [B, nkv, tmax] (ops.quantize_fp8_kv; fp8_code.h), so code * scale is exactly a bf16 number and the cache is an
// ordinary bf16 cache stored in half the bytes.  Pass 1 below is llm_decode_attn_split_kernel<bf16_t, HD, MASKED> reading that format; the
// workspace and pass 2 are the ones above.
// Contract: the output equals, bit for bit, what vtgb_llm_decode_attention_split returns on the dequantised cache.  The partition is the
// bf16 instantiation's -- 8 consecutive elements of a row per lane (an 8-byte load here), LPR = hd / 8 lanes per row, the same rows per
// lane, waves and chunks -- and a scale 2^e moves through every rounding unchanged (no overflow, no subnormal: |e| <= 120 and fp32
// partial sums of bf16 products): sum_e fmaf(q, c 2^e, .) = 2^e sum_e fmaf(q, c, .), so the K scale multiplies the row's score after its
// lanes are summed, and fmaf(p, c 2^e, acc) = fmaf(p 2^e, c, acc), so the V scale multiplies the softmax weight.  Both scales are read in
// the softmax stage (four coalesced keys per lane), where the weights pass through LDS anyway.
// Visibility is the bf16 kernel's: nothing past *pos is read -- codes or scales --, an invisible key's codes are replaced by zeros and its
// scales by 1 before any product, so a stale or masked slot may hold anything (the e4m3 NaN code, a NaN scale).
template <int HD, bool MASKED>
__global__ __launch_bounds__(256) void llm_decode_attn_split_fp8_kernel(const bf16_t* __restrict__ q, const uint8_t* __restrict__ kc8,
                                                                        const uint8_t* __restrict__ vc8, const float* __restrict__ ks,
                                                                        const float* __restrict__ vs, float* __restrict__ ws,
                                                                        const int64_t* __restrict__ pos_p, const uint8_t* __restrict__ key_valid,
                                                                        int B, int nq, int nkv, int tmax, float scale) {
    constexpr int EPL = 8;                        // elements per lane: as llm_decode_attn_split_kernel<bf16_t> (there 16 bytes, here 8)
    constexpr int LPR = HD / EPL;                 // lanes per row
    constexpr int RPI = 64 / LPR;                 // rows per load instruction
    constexpr int NI = 64 / RPI;                  // load instructions per wave (== LPR)
    __shared__ float qs[DEC_SPLIT_HEADS][HD];
    __shared__ float sc[DEC_SPLIT_HEADS][DEC_SPLIT_CHUNK];
    __shared__ __attribute__((aligned(16))) float red[4][DEC_SPLIT_HEADS][HD];

    const int chunk = blockIdx.x, b = blockIdx.z;
    const int pos = min((int)(*pos_p), tmax - 1);
    if (chunk * DEC_SPLIT_CHUNK > pos) return;
    const int group = nq / nkv, nhb = (group + DEC_SPLIT_HEADS - 1) / DEC_SPLIT_HEADS;
    const int kvh = blockIdx.y / nhb, hb = blockIdx.y % nhb;
    const int head0 = kvh * group + hb * DEC_SPLIT_HEADS, nh = min(DEC_SPLIT_HEADS, group - hb * DEC_SPLIT_HEADS);
    const int nc = (tmax + DEC_SPLIT_CHUNK - 1) / DEC_SPLIT_CHUNK;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane % LPR, rs = lane / LPR;      // this lane's 8-byte piece and row slot

    for (int i = tid; i < nh * HD; i += 256) qs[i / HD][i % HD] = (float)q[((int64_t)b * nq + head0) * HD + i];

    // ---- K: the wave's 64 rows of codes -> registers (row kl0 + i * RPI of instruction i); invisible rows stay zeros
    const int kl0 = wave * 64 + rs, key0 = chunk * DEC_SPLIT_CHUNK + kl0;
    const int64_t row0 = ((int64_t)b * nkv + kvh) * tmax;      // the (b, kvh) cache's first row: codes at row * HD, scales at row
    const uint8_t* kvr = MASKED ? key_valid + (int64_t)b * tmax : nullptr;
    unsigned vis = 0;
#pragma unroll
    for (int i = 0; i < NI; i++) {
        const int key = key0 + i * RPI;
        bool ok = key <= pos;
        if (MASKED && ok) ok = kvr[key] != 0;
        vis |= ok ? 1u << i : 0u;
    }
    // (as above: an invisible row's load goes to row *pos and its value is selected away)
    auto load_rows = [&](const uint8_t* __restrict__ src, uint2 (&reg)[NI]) {
#pragma unroll
        for (int i = 0; i < NI; i++) {
            const bool ok = vis >> i & 1;
            const uint2 v = *reinterpret_cast<const uint2*>(src + (row0 + (ok ? key0 + i * RPI : pos)) * HD + c * EPL);
            reg[i] = ok ? v : make_uint2(0u, 0u);
        }
    };
    uint2 reg[NI];
    load_rows(kc8, reg);
    __syncthreads();      // qs

    // ---- unscaled scores q . codes: per head, the lane's piece of every row, then the row's LPR lanes
    for (int h = 0; h < nh; h++) {
        float qv[EPL];
#pragma unroll
        for (int e = 0; e < EPL; e++) qv[e] = qs[h][c * EPL + e];
#pragma unroll
        for (int i = 0; i < NI; i++) {
            float lo[4], hi[4];
            kv8_widen4(reg[i].x, lo);
            kv8_widen4(reg[i].y, hi);
            float dot = 0.f;
#pragma unroll
            for (int e = 0; e < 4; e++) dot = fmaf(qv[e], lo[e], dot);
#pragma unroll
            for (int e = 0; e < 4; e++) dot = fmaf(qv[4 + e], hi[e], dot);
            dot = group_sum<LPR>(dot);
            if (c == 0) sc[h][kl0 + i * RPI] = (vis >> i & 1) ? dot : -INFINITY;
        }
    }
    // ---- V replaces K in the registers (the loads fly behind the softmax)
    load_rows(vc8, reg);
    __syncthreads();      // sc

    // ---- softmax statistics of the chunk: wave w takes the heads w, w + 4.  A lane's four keys lane + 64 j: their K scale makes the
    // score (dot * 2^ek) * scale = the bf16 kernel's dot * scale, their V scale goes into the weight left in sc
    if (wave < nh) {
        float sk[4], sv[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int key = chunk * DEC_SPLIT_CHUNK + lane + 64 * j;
            bool ok = key <= pos;
            if (MASKED && ok) ok = kvr[key] != 0;
            const float a = ks[row0 + (ok ? key : pos)], v = vs[row0 + (ok ? key : pos)];
            sk[j] = ok ? a : 1.f;
            sv[j] = ok ? v : 1.f;
        }
        for (int h = wave; h < nh; h += 4) {
            float s[4], m = -INFINITY;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float d = sc[h][lane + 64 * j];
                s[j] = d == -INFINITY ? d : (d * sk[j]) * scale;
                m = fmaxf(m, s[j]);
            }
            for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
#pragma unroll
            for (int j = 0; j < 4; j++) {
                s[j] = s[j] == -INFINITY ? 0.f : expf(s[j] - m);      // (an invisible key: exactly 0, also when the chunk has no visible key)
                sc[h][lane + 64 * j] = s[j] * sv[j];
            }
            const float l = group_sum<64>((s[0] + s[1]) + (s[2] + s[3]));
            if (lane == 0) {
                float* ml = ws + (int64_t)B * nq * nc * HD + (((int64_t)b * nq + head0 + h) * nc + chunk) * 2;
                ml[0] = m;
                ml[1] = l;
            }
        }
    }
    __syncthreads();      // sc = weights x V scales

    // ---- O: per head, the lane's rows in ascending order, then the wave's row slots, then (below) the four waves
    for (int h = 0; h < nh; h++) {
        float acc[EPL];
#pragma unroll
        for (int e = 0; e < EPL; e++) acc[e] = 0.f;
#pragma unroll
        for (int i = 0; i < NI; i++) {
            const float p = sc[h][kl0 + i * RPI];
            float lo[4], hi[4];
            kv8_widen4(reg[i].x, lo);
            kv8_widen4(reg[i].y, hi);
#pragma unroll
            for (int e = 0; e < 4; e++) acc[e] = fmaf(p, lo[e], acc[e]);
#pragma unroll
            for (int e = 0; e < 4; e++) acc[4 + e] = fmaf(p, hi[e], acc[4 + e]);
        }
#pragma unroll
        for (int e = 0; e < EPL; e++) {
            float v = acc[e];
            if constexpr (RPI > 1) v += __shfl_xor(v, LPR);
            if constexpr (RPI > 2) v += __shfl_xor(v, 2 * LPR);
            if constexpr (RPI > 4) v += __shfl_xor(v, 4 * LPR);
            acc[e] = v;
        }
        if (rs == 0) {
#pragma unroll
            for (int e = 0; e < EPL; e += 4)
                *reinterpret_cast<f32x4*>(&red[wave][h][c * EPL + e]) = f32x4{acc[e], acc[e + 1], acc[e + 2], acc[e + 3]};
        }
    }
    __syncthreads();      // red
    for (int i = tid; i < nh * HD; i += 256) {
        const int h = i / HD, d = i % HD;
        ws[(((int64_t)b * nq + head0 + h) * nc + chunk) * HD + d] = ((red[0][h][d] + red[1][h][d]) + red[2][h][d]) + red[3][h][d];
    }
}

template <int HD>
static int launch_split_fp8(const void* q, const uint8_t* kc8, const uint8_t* vc8, const float* ks, const float* vs, void* out, const int64_t* pos,
                            const uint8_t* key_valid, void* workspace, int B, int nq, int nkv, int tmax, float scale, hipStream_t s) {
    const int group = nq / nkv, nhb = (group + DEC_SPLIT_HEADS - 1) / DEC_SPLIT_HEADS, nc = (tmax + DEC_SPLIT_CHUNK - 1) / DEC_SPLIT_CHUNK;
    const dim3 grid(nc, nkv * nhb, B);
    float* ws = (float*)workspace;
    if (key_valid)
        hipLaunchKernelGGL((llm_decode_attn_split_fp8_kernel<HD, true>), grid, dim3(256), 0, s, (const bf16_t*)q, kc8, vc8, ks, vs, ws, pos, key_valid, B, nq,
                           nkv, tmax, scale);
    else
        hipLaunchKernelGGL((llm_decode_attn_split_fp8_kernel<HD, false>), grid, dim3(256), 0, s, (const bf16_t*)q, kc8, vc8, ks, vs, ws, pos,
                           (const uint8_t*)nullptr, B, nq, nkv, tmax, scale);
    VTGB_HIP(hipGetLastError());
    hipLaunchKernelGGL(llm_decode_attn_combine_kernel<bf16_t>, dim3((unsigned)((int64_t)B * nq)), dim3(HD), 0, s, (const float*)ws, (bf16_t*)out, pos,
                       (int64_t)B * nq, HD, tmax);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

extern "C" int vtgb_llm_decode_attention_split_fp8(int dtype, const void* q, const uint8_t* kc8, const uint8_t* vc8, const float* ks, const float* vs,
                                                   void* out, const int64_t* pos, const uint8_t* key_valid, void* workspace, int32_t B, int32_t nq,
                                                   int32_t nkv, int32_t hd, int32_t tmax, float scale, vtgb_stream_t stream) {
    VTGB_REQUIRE(q && kc8 && vc8 && ks && vs && out && pos && workspace, VTGB_EINVAL, "llm_decode_attention_split_fp8: NULL operand");
    VTGB_REQUIRE(dtype == VTGB_BF16 && B > 0 && nq > 0 && nkv > 0 && tmax > 0, VTGB_EINVAL,
                 "llm_decode_attention_split_fp8: bad argument (activations are VTGB_BF16)");
    VTGB_REQUIRE(nq % nkv == 0, VTGB_EINVAL, "llm_decode_attention_split_fp8: nq=%d is not a multiple of nkv=%d", nq, nkv);
    VTGB_REQUIRE(hd == 64 || hd == 128, VTGB_EUNSUPPORTED, "llm_decode_attention_split_fp8: hd=%d, built for 64 and 128", hd);
    VTGB_REQUIRE(tmax % 64 == 0 && tmax <= DEC_SPLIT_MAX_T, VTGB_EUNSUPPORTED,
                 "llm_decode_attention_split_fp8: tmax=%d is not a multiple of 64 up to %d", tmax, DEC_SPLIT_MAX_T);
    const int nhb = (nq / nkv + DEC_SPLIT_HEADS - 1) / DEC_SPLIT_HEADS;
    VTGB_REQUIRE(B <= 65535 && (int64_t)nkv * nhb <= 65535, VTGB_EUNSUPPORTED, "llm_decode_attention_split_fp8: B=%d / nq=%d exceed the grid", B, nq);
    const auto misaligned = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
    VTGB_REQUIRE(!misaligned(q, 16) && !misaligned(kc8, 16) && !misaligned(vc8, 16) && !misaligned(out, 16) && !misaligned(workspace, 16) &&
                     !misaligned(ks, 4) && !misaligned(vs, 4),
                 VTGB_EUNSUPPORTED, "llm_decode_attention_split_fp8: q / kc8 / vc8 / out / workspace need 16-byte, ks / vs 4-byte alignment");
    hipStream_t s = (hipStream_t)stream;
    return hd == 128 ? launch_split_fp8<128>(q, kc8, vc8, ks, vs, out, pos, key_valid, workspace, B, nq, nkv, tmax, scale, s)
                     : launch_split_fp8<64>(q, kc8, vc8, ks, vs, out, pos, key_valid, workspace, B, nq, nkv, tmax, scale, s);
}

// ---- beam search (opt-in: beam_search="graph").  llm_decode_attn_split_kernel with two K/V sources and no K/V copies when beams are
// re-ordered: the R = B * K beam rows of a batch share ONE prompt cache per batch item, kp / vp [B, nkv, tmax_p, hd] (the prefill's, on B
// rows), and append what they generate to kg / vg [R, nkv, tmax_g, hd] at slot = the step; src_row [R, tmax_g] int32 names, for beam row r,
// the generated-cache row that holds its key of slot s (its ancestor at that step).  Global key t of row r:
//   t <  *n_prompt:  kp[r / K, kvh, t]                                        (and key_valid[r / K, t] != 0, MASKED)
//   t >= *n_prompt:  kg[clamp(src_row[r, t - *n_prompt], 0, R - 1), kvh, t - *n_prompt]
// visible while t <= *pos (clamped to *n_prompt + tmax_g - 1; *n_prompt to [0, tmax_p]).  A table entry is clamped before use: a wrong
// table gives wrong numbers, never a read outside the caches.
// Contract: chunk = t / 256, wave = t / 64 % 4, a lane's keys and the order inside every sum follow the GLOBAL key index t exactly as in
// llm_decode_attn_split_kernel, so the output equals, bit for bit, vtgb_llm_decode_attention_split on the cache [R, nkv, T, hd] that this
// gather materialises.  Nothing past *pos, no masked slot and no prompt slot >= *n_prompt reaches a product (an invisible row's load goes
// to row 0 of the item's prompt cache and is selected away).  Workspace and pass 2 are the split kernel's, with tmax = tmax_p + tmax_g.
template <typename T, int HD, bool MASKED>
__global__ __launch_bounds__(256) void llm_decode_attn_beam_kernel(const T* __restrict__ q, const T* __restrict__ kp, const T* __restrict__ vp,
                                                                   const T* __restrict__ kg, const T* __restrict__ vg,
                                                                   const int32_t* __restrict__ src_row, float* __restrict__ ws,
                                                                   const int64_t* __restrict__ np_p, const int64_t* __restrict__ pos_p,
                                                                   const uint8_t* __restrict__ key_valid, int R, int K, int nq, int nkv, int tmax_p,
                                                                   int tmax_g, float scale) {
    constexpr int EPL = 16 / (int)sizeof(T);      // elements per lane: one 16-byte piece of a row
    constexpr int LPR = HD / EPL;                 // lanes per row
    constexpr int RPI = 64 / LPR;                 // rows per load instruction
    constexpr int NI = 64 / RPI;                  // load instructions per wave (== LPR)
    typedef T TV __attribute__((ext_vector_type(EPL)));
    __shared__ float qs[DEC_SPLIT_HEADS][HD];
    __shared__ float sc[DEC_SPLIT_HEADS][DEC_SPLIT_CHUNK];
    __shared__ __attribute__((aligned(16))) float red[4][DEC_SPLIT_HEADS][HD];

    const int chunk = blockIdx.x, r = blockIdx.z, b = r / K;
    const int tmax = tmax_p + tmax_g;
    const int64_t np64 = *np_p, pos64 = *pos_p;
    const int np = (int)(np64 < 0 ? 0 : np64 > tmax_p ? tmax_p : np64);
    const int pos_c = (int)(pos64 < -1 ? -1 : pos64 > tmax - 1 ? tmax - 1 : pos64);      // what pass 2 walks: chunks 0 .. pos_c / 256
    if (chunk * DEC_SPLIT_CHUNK > pos_c) return;
    const int pos = min(pos_c, np + tmax_g - 1);                                          // the last visible key
    const int group = nq / nkv, nhb = (group + DEC_SPLIT_HEADS - 1) / DEC_SPLIT_HEADS;
    const int kvh = blockIdx.y / nhb, hb = blockIdx.y % nhb;
    const int head0 = kvh * group + hb * DEC_SPLIT_HEADS, nh = min(DEC_SPLIT_HEADS, group - hb * DEC_SPLIT_HEADS);
    const int nc = (tmax + DEC_SPLIT_CHUNK - 1) / DEC_SPLIT_CHUNK;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane % LPR, rs = lane / LPR;      // this lane's 16-byte piece and row slot

    for (int i = tid; i < nh * HD; i += 256) qs[i / HD][i % HD] = (float)q[((int64_t)r * nq + head0) * HD + i];

    // ---- K: the wave's 64 rows -> registers (row kl0 + i * RPI of instruction i); invisible rows stay zeros
    const int kl0 = wave * 64 + rs, key0 = chunk * DEC_SPLIT_CHUNK + kl0;
    const int64_t pbase = ((int64_t)b * nkv + kvh) * tmax_p * HD + c * EPL;      // row 0 of the item's prompt cache (this K/V head, this piece)
    const uint8_t* kvr = MASKED ? key_valid + (int64_t)b * tmax_p : nullptr;
    unsigned vis = 0;
    int64_t off[NI];      // element offset of the row: into kp / vp (key < np or invisible) or kg / vg
#pragma unroll
    for (int i = 0; i < NI; i++) {
        const int key = key0 + i * RPI;
        bool ok = key <= pos;
        if (MASKED && ok && key < np) ok = kvr[key] != 0;
        vis |= ok ? 1u << i : 0u;
        int64_t o = pbase;
        if (ok && key < np) {
            o = pbase + (int64_t)key * HD;
        } else if (ok) {
            const int g = key - np;      // < tmax_g: key <= pos <= np + tmax_g - 1
            int sr = src_row[(int64_t)r * tmax_g + g];
            sr = sr < 0 ? 0 : sr >= R ? R - 1 : sr;
            o = (((int64_t)sr * nkv + kvh) * tmax_g + g) * HD + c * EPL;
        }
        off[i] = o;
    }
    TV zero;
#pragma unroll
    for (int e = 0; e < EPL; e++) zero[e] = (T)0.f;
    auto load_rows = [&](const T* __restrict__ srcp, const T* __restrict__ srcg, TV (&reg)[NI]) {
#pragma unroll
        for (int i = 0; i < NI; i++) {
            const bool ok = vis >> i & 1;
            const T* p = (ok && key0 + i * RPI >= np) ? srcg : srcp;
            const TV v = *reinterpret_cast<const TV*>(p + off[i]);
            reg[i] = ok ? v : zero;
        }
    };
    TV reg[NI];
    load_rows(kp, kg, reg);
    __syncthreads();      // qs

    // ---- scores: per head, the lane's piece of every row, then the row's LPR lanes
    for (int h = 0; h < nh; h++) {
        float qv[EPL];
#pragma unroll
        for (int e = 0; e < EPL; e++) qv[e] = qs[h][c * EPL + e];
#pragma unroll
        for (int i = 0; i < NI; i++) {
            float dot = 0.f;
#pragma unroll
            for (int e = 0; e < EPL; e++) dot = fmaf(qv[e], (float)reg[i][e], dot);
            dot = group_sum<LPR>(dot);
            if (c == 0) sc[h][kl0 + i * RPI] = (vis >> i & 1) ? dot * scale : -INFINITY;
        }
    }
    // ---- V replaces K in the registers (the loads fly behind the softmax)
    load_rows(vp, vg, reg);
    __syncthreads();      // sc

    // ---- softmax statistics of the chunk: wave w takes the heads w, w + 4
    for (int h = wave; h < nh; h += 4) {
        float s[4], m = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            s[j] = sc[h][lane + 64 * j];
            m = fmaxf(m, s[j]);
        }
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
#pragma unroll
        for (int j = 0; j < 4; j++) {
            s[j] = s[j] == -INFINITY ? 0.f : expf(s[j] - m);      // (an invisible key: exactly 0, also when the chunk has no visible key)
            sc[h][lane + 64 * j] = s[j];
        }
        const float l = group_sum<64>((s[0] + s[1]) + (s[2] + s[3]));
        if (lane == 0) {
            float* ml = ws + (int64_t)R * nq * nc * HD + (((int64_t)r * nq + head0 + h) * nc + chunk) * 2;
            ml[0] = m;
            ml[1] = l;
        }
    }
    __syncthreads();      // sc = weights

    // ---- O: per head, the lane's rows in ascending order, then the wave's row slots, then (below) the four waves
    for (int h = 0; h < nh; h++) {
        float acc[EPL];
#pragma unroll
        for (int e = 0; e < EPL; e++) acc[e] = 0.f;
#pragma unroll
        for (int i = 0; i < NI; i++) {
            const float p = sc[h][kl0 + i * RPI];
#pragma unroll
            for (int e = 0; e < EPL; e++) acc[e] = fmaf(p, (float)reg[i][e], acc[e]);
        }
#pragma unroll
        for (int e = 0; e < EPL; e++) {
            float v = acc[e];
            if constexpr (RPI > 1) v += __shfl_xor(v, LPR);
            if constexpr (RPI > 2) v += __shfl_xor(v, 2 * LPR);
            if constexpr (RPI > 4) v += __shfl_xor(v, 4 * LPR);
            acc[e] = v;
        }
        if (rs == 0) {
#pragma unroll
            for (int e = 0; e < EPL; e += 4)
                *reinterpret_cast<f32x4*>(&red[wave][h][c * EPL + e]) = f32x4{acc[e], acc[e + 1], acc[e + 2], acc[e + 3]};
        }
    }
    __syncthreads();      // red
    for (int i = tid; i < nh * HD; i += 256) {
        const int h = i / HD, d = i % HD;
        ws[(((int64_t)r * nq + head0 + h) * nc + chunk) * HD + d] = ((red[0][h][d] + red[1][h][d]) + red[2][h][d]) + red[3][h][d];
    }
}

template <typename T, int HD>
static int launch_beam(const vtgb_llm_decode_attention_beam_args* a, hipStream_t s) {
    const int tmax = a->tmax_p + a->tmax_g;
    const int group = a->nq / a->nkv, nhb = (group + DEC_SPLIT_HEADS - 1) / DEC_SPLIT_HEADS, nc = (tmax + DEC_SPLIT_CHUNK - 1) / DEC_SPLIT_CHUNK;
    const dim3 grid(nc, a->nkv * nhb, a->R);
    float* ws = (float*)a->workspace;
    if (a->key_valid)
        hipLaunchKernelGGL((llm_decode_attn_beam_kernel<T, HD, true>), grid, dim3(256), 0, s, (const T*)a->q, (const T*)a->kp, (const T*)a->vp,
                           (const T*)a->kg, (const T*)a->vg, a->src_row, ws, a->n_prompt, a->pos, a->key_valid, a->R, a->K, a->nq, a->nkv, a->tmax_p,
                           a->tmax_g, a->scale);
    else
        hipLaunchKernelGGL((llm_decode_attn_beam_kernel<T, HD, false>), grid, dim3(256), 0, s, (const T*)a->q, (const T*)a->kp, (const T*)a->vp,
                           (const T*)a->kg, (const T*)a->vg, a->src_row, ws, a->n_prompt, a->pos, (const uint8_t*)nullptr, a->R, a->K, a->nq, a->nkv,
                           a->tmax_p, a->tmax_g, a->scale);
    VTGB_HIP(hipGetLastError());
    hipLaunchKernelGGL(llm_decode_attn_combine_kernel<T>, dim3((unsigned)((int64_t)a->R * a->nq)), dim3(HD), 0, s, (const float*)ws, (T*)a->out, a->pos,
                       (int64_t)a->R * a->nq, HD, tmax);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

extern "C" int vtgb_llm_decode_attention_beam(const vtgb_llm_decode_attention_beam_args* a, vtgb_stream_t stream) {
    VTGB_REQUIRE(a, VTGB_EINVAL, "llm_decode_attention_beam: NULL args");
    VTGB_REQUIRE(a->q && a->kp && a->vp && a->kg && a->vg && a->src_row && a->out && a->n_prompt && a->pos && a->workspace, VTGB_EINVAL,
                 "llm_decode_attention_beam: NULL operand");
    VTGB_REQUIRE((a->dtype == VTGB_BF16 || a->dtype == VTGB_F32) && a->R > 0 && a->K > 0 && a->nq > 0 && a->nkv > 0 && a->tmax_p > 0 && a->tmax_g > 0,
                 VTGB_EINVAL, "llm_decode_attention_beam: bad argument");
    VTGB_REQUIRE(a->R % a->K == 0, VTGB_EINVAL, "llm_decode_attention_beam: R=%d rows are not a multiple of K=%d beams", a->R, a->K);
    VTGB_REQUIRE(a->nq % a->nkv == 0, VTGB_EINVAL, "llm_decode_attention_beam: nq=%d is not a multiple of nkv=%d", a->nq, a->nkv);
    VTGB_REQUIRE(a->hd == 64 || a->hd == 128, VTGB_EUNSUPPORTED, "llm_decode_attention_beam: hd=%d, built for 64 and 128", a->hd);
    VTGB_REQUIRE(a->tmax_p % 64 == 0 && a->tmax_g % 64 == 0 && (int64_t)a->tmax_p + a->tmax_g <= DEC_SPLIT_MAX_T, VTGB_EUNSUPPORTED,
                 "llm_decode_attention_beam: tmax_p=%d / tmax_g=%d are not multiples of 64 with a sum up to %d", a->tmax_p, a->tmax_g, DEC_SPLIT_MAX_T);
    const int nhb = (a->nq / a->nkv + DEC_SPLIT_HEADS - 1) / DEC_SPLIT_HEADS;
    VTGB_REQUIRE(a->R <= 65535 && (int64_t)a->nkv * nhb <= 65535, VTGB_EUNSUPPORTED, "llm_decode_attention_beam: R=%d / nq=%d exceed the grid", a->R, a->nq);
    const auto misaligned = [](const void* p, uintptr_t al) { return (reinterpret_cast<uintptr_t>(p) & (al - 1)) != 0; };
    VTGB_REQUIRE(!misaligned(a->q, 16) && !misaligned(a->kp, 16) && !misaligned(a->vp, 16) && !misaligned(a->kg, 16) && !misaligned(a->vg, 16) &&
                     !misaligned(a->out, 16) && !misaligned(a->workspace, 16) && !misaligned(a->src_row, 4),
                 VTGB_EUNSUPPORTED, "llm_decode_attention_beam: q / kp / vp / kg / vg / out / workspace need 16-byte, src_row 4-byte alignment");
    hipStream_t s = (hipStream_t)stream;
    if (a->dtype == VTGB_BF16) return a->hd == 128 ? launch_beam<bf16_t, 128>(a, s) : launch_beam<bf16_t, 64>(a, s);
    return a->hd == 128 ? launch_beam<float, 128>(a, s) : launch_beam<float, 64>(a, s);
}
