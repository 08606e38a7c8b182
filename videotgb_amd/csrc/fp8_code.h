// fp8_code.h -- the e4m3 quantisation helpers the fp8 weight stream (gemm_skinny.hip) and the fp8 K/V cache (llm.hip, attn_decode.hip) share.
#pragma once
#include <math.h>
#include <stdint.h>

// The fp8 quantisation recipe (ops.quantize_fp8_rows states it for the host).  e: the smallest integer with amax 2^-e <= 448 = 0.875 x 2^9,
// exactly, from the binary exponent (no log2); 0 for a zero row.
__host__ __device__ inline int sk8_row_exp(float amax) {
    if (!(amax > 0.f)) return 0;
    int ex;
    const float m = frexpf(amax, &ex);                         // amax = m 2^ex, 0.5 <= m < 1
    return ex - 9 + (m > 0.875f ? 1 : 0);
}

// v (|v| <= 448) rounded to nearest even into an OCP e4m3fn code, on the bits: normal codes keep 3 mantissa bits; below 2^-6 the code is
// the integer round(|v| 2^9) (subnormals, 8 = the smallest normal)
__host__ __device__ inline uint8_t sk8_code(float v) {
    union { float f; uint32_t u; } c;
    c.f = v;
    const uint32_t sign = (c.u >> 24) & 0x80u;
    c.u &= 0x7FFFFFFFu;
    if (c.f < 0.015625f) return (uint8_t)(sign | (uint32_t)rintf(c.f * 512.f));
    c.u += 0x7FFFFu + ((c.u >> 20) & 1u);
    return (uint8_t)(sign | ((((c.u >> 23) - 120u) << 3) | ((c.u >> 20) & 7u)));
}

// ---- the fp8 K/V cache (kv_cache="fp8"; ops.quantize_fp8_kv states the recipe for the host): the rule above per cache row (one token of one
// K/V head), with e clamped below at KV8_MIN_EXP so that code * 2^e stays a normal bf16 number.
constexpr int KV8_MIN_EXP = -100;
__host__ __device__ inline int kv8_row_exp(float amax) {
    const int e = sk8_row_exp(amax);
    return e < KV8_MIN_EXP ? KV8_MIN_EXP : e;
}

// 4 e4m3 codes (one dword) -> 4 fp32, exact
__device__ __forceinline__ void kv8_widen4(unsigned w, float (&o)[4]) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((ext_vector_type(2))) float f32x2_;
    const f32x2_ a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
    o[0] = a[0], o[1] = a[1], o[2] = b[0], o[3] = b[1];
#else
    o[0] = o[1] = o[2] = o[3] = 0.f;
#endif
}
