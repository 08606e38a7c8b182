// llm.hip -- building blocks of the KV-cached, clip-batched greedy decode step.
// The LLM weights and GEMMs stay third-party (HF Llama weights, hipBLASLt via PyTorch); what is
// fused here are the ~25 small elementwise/reduction launches per layer that otherwise dominate
// a graph-replayed decode step at batch <= 64 (the GEMVs themselves are HBM-bound).
// Semantics follow transformers' modeling_llama op by op, INCLUDING where it rounds to the
// activation dtype (bf16 in the benchmark, fp32 in the parity tests):
//   LlamaRMSNorm: variance in fp32; out = weight * (x_fp32 * rsqrt(var + eps)).to(dtype)
//   residual:     hidden = residual + hidden              (one rounding)
//   rotary:       q*cos + rotate_half(q)*sin              (each product and the sum rounded)
//   MLP:          down(act(gate) * up), act = SiLU        (act and product rounded)
// The current position is read from device memory, so one captured hipGraph serves every step.
#include "common.h"

#include <math.h>

template <typename T> struct Cvt;
template <> struct Cvt<float> {
    static __device__ __forceinline__ float to(float v) { return v; }
    static __device__ __forceinline__ float rnd(float v) { return v; }
};
template <> struct Cvt<bf16_t> {
    static __device__ __forceinline__ bf16_t to(float v) { return (bf16_t)v; }
    // round-to-nearest-even to bf16 precision, by hand: hipcc may keep the excess precision of a float -> __bf16 -> float round trip (it
    // did in the rotary kernels: one product stayed unrounded and fused into an FMA, 1 ulp off HF's bf16 arithmetic in 7 % of the values)
    static __device__ __forceinline__ float rnd(float v) {
        unsigned u = __float_as_uint(v);
        if ((u & 0x7F800000u) != 0x7F800000u) u += 0x7FFFu + ((u >> 16) & 1u);      // (Inf / NaN pass through)
        return __uint_as_float(u & 0xFFFF0000u);
    }
};

// The decode step's split-K projections leave fp32 fragments (gemm_skinny_kernel; gemm_skinny.hip states their layout, "fragments"); their consumers add a
// tile's fragments in split order and round once to the activation type themselves (r5: the separate reduce launch -- three per layer -- is gone:
// same sums, same rounding, 96 launches fewer per token).  V consecutive columns starting at column i (i % V == 0, V <= 8) of row `row`:
template <typename T, int V>
__device__ __forceinline__ void parts_sum(const float* __restrict__ part, int S, int M, int64_t row, int i, float (&out)[V]) {
    const int b = i >> 7, c = i & 127;
#pragma unroll
    for (int e = 0; e < V; e++) out[e] = 0.f;
    for (int sp = 0; sp < S; sp++) {
        const float* p = part + ((int64_t)(b * S + sp) * M + row) * 128 + c;
#pragma unroll
        for (int q = 0; q < V; q += 4) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(p + q);
#pragma unroll
            for (int e = 0; e < 4; e++) out[q + e] += t[e];
        }
    }
#pragma unroll
    for (int e = 0; e < V; e++) out[e] = Cvt<T>::rnd(out[e]);
}

// ---- x (+= delta) ; h = rmsnorm(x) * w.   One workgroup per row.
template <typename T>
__global__ __launch_bounds__(256) void llm_rmsnorm_kernel(T* __restrict__ x, const T* __restrict__ delta, const T* __restrict__ w,
                                                          T* __restrict__ h, int H, float eps) {
    __shared__ float red[4];
    const int64_t row = blockIdx.x;
    T* xr = x + row * H;
    const T* dr = delta ? delta + row * H : nullptr;
    float ss = 0.f;
    for (int i = threadIdx.x; i < H; i += 256) {
        float v = (float)xr[i];
        if (dr) {
            v = Cvt<T>::rnd(v + (float)dr[i]);
            xr[i] = Cvt<T>::to(v);
        }
        ss += v * v;
    }
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    const float var = (red[0] + red[1] + red[2] + red[3]) / (float)H;
    const float rs = rsqrtf(var + eps);
    for (int i = threadIdx.x; i < H; i += 256) {
        const float n = Cvt<T>::rnd((float)xr[i] * rs);
        h[row * H + i] = Cvt<T>::to((float)w[i] * n);
    }
}

// The same with the row held in registers between the two passes (r4: the scalar loop above took 17 us per launch at 124 x 4096 -- sixteen
// dependent 2-byte round trips per pass; 65 launches per decoded token).  NV 16-byte vectors per thread: H == 256 * NV * (16 / sizeof(T)).
template <typename T, int NV>
__global__ __launch_bounds__(256) void llm_rmsnorm_vec_kernel(T* __restrict__ x, const T* __restrict__ delta, const T* __restrict__ w,
                                                              T* __restrict__ h, int H, float eps, const float* __restrict__ part = nullptr, int S = 0,
                                                              int M = 0) {
    constexpr int V = 16 / (int)sizeof(T);
    typedef T TV __attribute__((ext_vector_type(V)));
    __shared__ float red[4];
    const int64_t row = blockIdx.x;
    T* xr = x + row * H;
    float v[NV][V];
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < NV; c++) {
        const int i = (c * 256 + threadIdx.x) * V;
        const TV xv = *reinterpret_cast<const TV*>(xr + i);
#pragma unroll
        for (int e = 0; e < V; e++) v[c][e] = (float)xv[e];
        if (part) {            // delta = the sum of the K-split fragments, rounded once (what the reduce launch stored)
            float dv[V];
            parts_sum<T, V>(part, S, M, row, i, dv);
            TV o;
#pragma unroll
            for (int e = 0; e < V; e++) {
                v[c][e] = Cvt<T>::rnd(v[c][e] + dv[e]);
                o[e] = Cvt<T>::to(v[c][e]);
            }
            *reinterpret_cast<TV*>(xr + i) = o;
        } else if (delta) {
            const TV dv = *reinterpret_cast<const TV*>(delta + row * H + i);
            TV o;
#pragma unroll
            for (int e = 0; e < V; e++) {
                v[c][e] = Cvt<T>::rnd(v[c][e] + (float)dv[e]);
                o[e] = Cvt<T>::to(v[c][e]);
            }
            *reinterpret_cast<TV*>(xr + i) = o;
        }
#pragma unroll
        for (int e = 0; e < V; e++) ss += v[c][e] * v[c][e];
    }
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    const float var = (red[0] + red[1] + red[2] + red[3]) / (float)H;
    const float rs = rsqrtf(var + eps);
#pragma unroll
    for (int c = 0; c < NV; c++) {
        const int i = (c * 256 + threadIdx.x) * V;
        const TV wv = *reinterpret_cast<const TV*>(w + i);
        TV o;
#pragma unroll
        for (int e = 0; e < V; e++) o[e] = Cvt<T>::to((float)wv[e] * Cvt<T>::rnd(v[c][e] * rs));
        *reinterpret_cast<TV*>(h + row * H + i) = o;
    }
}

// ---- rotary on q and k at position *pos, k and v appended to the cache.  One workgroup per (batch, head).
// ROW_OFF (padded batches): the rotary row of batch entry b is *pos + rope_off[b] (HF's per-row position ids), the cache row stays *pos.
template <typename T, bool ROW_OFF>
__device__ __forceinline__ void rope_cache_body(const T* __restrict__ qkv, T* __restrict__ q_out, T* __restrict__ kc, T* __restrict__ vc,
                                                const T* __restrict__ cos_t, const T* __restrict__ sin_t, const int64_t* __restrict__ pos_p,
                                                const int64_t* __restrict__ rope_off, int nq, int nkv, int hd, int tmax, const float* __restrict__ part,
                                                int S, int M) {
#pragma clang fp contract(off)      // fp32: mul, mul, add are three roundings in the reference -- no FMA
    const int b = blockIdx.y, head = blockIdx.x;   // head in [0, nq + 2 nkv)
    const int64_t pos = *pos_p;
    int64_t rp = pos;
    if constexpr (ROW_OFF) {
        rp += rope_off[b];
        rp = rp < 0 ? 0 : rp >= tmax ? tmax - 1 : rp;      // (the tables have tmax rows; the decoder's offsets keep rp in [0, pos])
    }
    const T* src = qkv + ((int64_t)b * (nq + 2 * nkv) + head) * hd;
    const int half = hd >> 1;
    // part != NULL: qkv is still the projection's K-split fragments -- element (b, col) = the fragments' sum in split order, rounded once
    auto at = [&](int d) -> float {
        if (!part) return (float)src[d];
        const int col = head * hd + d;
        float t = 0.f;
        for (int sp = 0; sp < S; sp++) t += part[((int64_t)((col >> 7) * S + sp) * M + b) * 128 + (col & 127)];
        return Cvt<T>::rnd(t);
    };
    for (int d = threadIdx.x; d < hd; d += blockDim.x) {
        const float v = at(d);
        float outv = v;
        if (head < nq + nkv && cos_t) {      // (cos_t == NULL: no rotary -- T5's decoder: q passed through, k / v appended)
            const float c = (float)cos_t[rp * hd + d], sn = (float)sin_t[rp * hd + d];
            const float rot = d < half ? -at(d + half) : at(d - half);
            const float pa = Cvt<T>::rnd(v * c), pb = Cvt<T>::rnd(rot * sn);      // (contract(off): the reference's three roundings, no FMA)
            outv = Cvt<T>::rnd(pa + pb);
        }
        if (head < nq) q_out[((int64_t)b * nq + head) * hd + d] = Cvt<T>::to(outv);
        else if (head < nq + nkv) kc[(((int64_t)b * nkv + (head - nq)) * tmax + pos) * hd + d] = Cvt<T>::to(outv);
        else vc[(((int64_t)b * nkv + (head - nq - nkv)) * tmax + pos) * hd + d] = Cvt<T>::to(outv);
    }
}

template <typename T>
__global__ __launch_bounds__(128) void llm_rope_cache_kernel(const T* __restrict__ qkv, T* __restrict__ q_out, T* __restrict__ kc,
                                                             T* __restrict__ vc, const T* __restrict__ cos_t, const T* __restrict__ sin_t,
                                                             const int64_t* __restrict__ pos_p, int nq, int nkv, int hd, int tmax,
                                                             const float* __restrict__ part = nullptr, int S = 0, int M = 0) {
    rope_cache_body<T, false>(qkv, q_out, kc, vc, cos_t, sin_t, pos_p, nullptr, nq, nkv, hd, tmax, part, S, M);
}

template <typename T>
__global__ __launch_bounds__(128) void llm_rope_cache_pos_kernel(const T* __restrict__ qkv, T* __restrict__ q_out, T* __restrict__ kc,
                                                                 T* __restrict__ vc, const T* __restrict__ cos_t, const T* __restrict__ sin_t,
                                                                 const int64_t* __restrict__ pos_p, const int64_t* __restrict__ rope_off, int nq,
                                                                 int nkv, int hd, int tmax, const float* __restrict__ part = nullptr, int S = 0,
                                                                 int M = 0) {
    rope_cache_body<T, true>(qkv, q_out, kc, vc, cos_t, sin_t, pos_p, rope_off, nq, nkv, hd, tmax, part, S, M);
}

// ---- single-query attention over the cache rows [0, *pos].  One wave per (batch, q head), 4 per workgroup.
// MASKED (padded batches): key_valid[b, key] == 0 keys get no weight; neither their K nor their V rows are read, so whatever a pad slot of
// the cache holds (NaN included) cannot reach the output.  The valid keys are summed in the same order as unmasked.
constexpr int DEC_MAX_T = 2048;
template <typename T, bool MASKED>
__device__ __forceinline__ void decode_attn_body(const T* __restrict__ q, const T* __restrict__ kc, const T* __restrict__ vc, T* __restrict__ out,
                                                 const int64_t* __restrict__ pos_p, const uint8_t* __restrict__ key_valid, int B, int nq, int nkv, int hd,
                                                 int tmax, float scale) {
    extern __shared__ float dsm[];   // per wave: hd floats of q + (tmax) scores
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // (uniform: batch / head / cache bases on the scalar unit)
    const int64_t idx = (int64_t)blockIdx.x * 4 + wave;
    const bool active = idx < (int64_t)B * nq;
    const int64_t id = active ? idx : (int64_t)B * nq - 1;
    const int b = id / nq, head = id % nq, kvh = head / (nq / nkv);
    const int n_keys = (int)(*pos_p) + 1;
    float* qs = dsm + wave * (hd + tmax);
    float* sc = qs + hd;
    const T* qr = q + ((int64_t)b * nq + head) * hd;
    const T* kr = kc + ((int64_t)b * nkv + kvh) * tmax * hd;
    const T* vr = vc + ((int64_t)b * nkv + kvh) * tmax * hd;
    for (int d = lane; d < hd; d += 64) qs[d] = (float)qr[d];
    __syncthreads();
    float mx = -INFINITY;
    const uint8_t* kvr = MASKED ? key_valid + (int64_t)b * tmax : nullptr;
    for (int key = lane; key < n_keys; key += 64) {
        if constexpr (MASKED) {
            if (!kvr[key]) {
                sc[key] = -INFINITY;
                continue;
            }
        }
        const T* k = kr + (int64_t)key * hd;
        float dot = 0.f;
        if constexpr (sizeof(T) == 2) {
            // a lane owns a key row: 16-byte loads (8 elements) instead of 2-byte ones, same summation order
            if ((hd & 7) == 0) {
                for (int d = 0; d < hd; d += 8) {
                    const bf16x8 kv = *reinterpret_cast<const bf16x8*>(k + d);
#pragma unroll
                    for (int e = 0; e < 8; e++) dot = fmaf(qs[d + e], (float)kv[e], dot);
                }
            } else {
                for (int d = 0; d < hd; d++) dot = fmaf(qs[d], (float)k[d], dot);
            }
        } else {
            for (int d = 0; d < hd; d++) dot = fmaf(qs[d], (float)k[d], dot);
        }
        dot *= scale;
        sc[key] = dot;
        mx = fmaxf(mx, dot);
    }
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    float sum = 0.f;
    for (int key = lane; key < n_keys; key += 64) {
        const float e = MASKED && sc[key] == -INFINITY ? 0.f : expf(sc[key] - mx);      // (masked: exactly 0, also when every key is masked)
        sc[key] = e;
        sum += e;
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    __syncthreads();
    const float inv = MASKED && sum == 0.f ? 0.f : 1.0f / sum;
    // MASKED: a key of zero weight (masked; or valid with an underflowed weight, which adds nothing either way) contributes an exact 0.  No
    // branch: its load is redirected to row *pos (always in bounds, a cache hit) and the value selected away, so every load of the
    // sixteen-key group is issued before the first wait and a pad slot's contents (NaN included) never reach a product.
    const int last = n_keys - 1;
    auto vrow = [&](int key) { return MASKED && sc[key] == 0.f ? last : key; };
    auto vload2 = [&](int key, int d) {
        typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
        const bf16x2_t v = *reinterpret_cast<const bf16x2_t*>(vr + (int64_t)vrow(key) * hd + d);
        return MASKED && sc[key] == 0.f ? bf16x2_t{(bf16_t)0.f, (bf16_t)0.f} : v;
    };
    if constexpr (sizeof(T) == 2) {
        if ((hd & 1) == 0) {
            // a lane owns two adjacent channels: one 4-byte load per key (a key row = one coalesced 2 hd-byte read), sixteen keys in flight
            // (r4: four in flight made the ~68 keys of the bench seventeen dependent memory round trips: 38 us per launch), same summation order
            typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
            for (int d = lane * 2; d < hd; d += 128) {
                float a0 = 0.f, a1 = 0.f;
                int key = 0;
                for (; key + 16 <= n_keys; key += 16) {
                    bf16x2_t v[16];
#pragma unroll
                    for (int u = 0; u < 16; u++) v[u] = vload2(key + u, d);
#pragma unroll
                    for (int u = 0; u < 16; u++) { a0 = fmaf(sc[key + u], (float)v[u][0], a0); a1 = fmaf(sc[key + u], (float)v[u][1], a1); }
                }
                for (; key + 4 <= n_keys; key += 4) {
                    bf16x2_t v[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) v[u] = vload2(key + u, d);
#pragma unroll
                    for (int u = 0; u < 4; u++) { a0 = fmaf(sc[key + u], (float)v[u][0], a0); a1 = fmaf(sc[key + u], (float)v[u][1], a1); }
                }
                for (; key < n_keys; key++) {
                    const bf16x2_t v = vload2(key, d);
                    a0 = fmaf(sc[key], (float)v[0], a0); a1 = fmaf(sc[key], (float)v[1], a1);
                }
                if (active) *reinterpret_cast<bf16x2_t*>(out + ((int64_t)b * nq + head) * hd + d) = bf16x2_t{(bf16_t)(a0 * inv), (bf16_t)(a1 * inv)};
            }
            return;
        }
    }
    for (int d = lane; d < hd; d += 64) {
        float acc = 0.f;
        for (int key = 0; key < n_keys; key++) {
            const float v = (float)vr[(int64_t)vrow(key) * hd + d];
            acc = fmaf(sc[key], MASKED && sc[key] == 0.f ? 0.f : v, acc);
        }
        if (active) out[((int64_t)b * nq + head) * hd + d] = Cvt<T>::to(acc * inv);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void llm_decode_attn_kernel(const T* __restrict__ q, const T* __restrict__ kc, const T* __restrict__ vc,
                                                              T* __restrict__ out, const int64_t* __restrict__ pos_p, int B, int nq, int nkv,
                                                              int hd, int tmax, float scale) {
    decode_attn_body<T, false>(q, kc, vc, out, pos_p, nullptr, B, nq, nkv, hd, tmax, scale);
}

template <typename T>
__global__ __launch_bounds__(256) void llm_decode_attn_masked_kernel(const T* __restrict__ q, const T* __restrict__ kc, const T* __restrict__ vc,
                                                                     T* __restrict__ out, const int64_t* __restrict__ pos_p,
                                                                     const uint8_t* __restrict__ key_valid, int B, int nq, int nkv, int hd, int tmax,
                                                                     float scale) {
    decode_attn_body<T, true>(q, kc, vc, out, pos_p, key_valid, B, nq, nkv, hd, tmax, scale);
}

// ---- act[b, i] = silu(gu[b, i]) * gu[b, I + i]
template <typename T>
__global__ void llm_silu_mul_kernel(const T* __restrict__ gu, T* __restrict__ act, int64_t rows, int I) {
    const int64_t n = rows * I;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / I, c = i - r * I;
        const float g = (float)gu[r * 2 * I + c], u = (float)gu[r * 2 * I + I + c];
        const float s = Cvt<T>::rnd(g / (1.0f + expf(-g)));
        act[i] = Cvt<T>::to(s * u);
    }
}

// one 16-byte vector per thread, row = blockIdx.y (r4: the scalar form above divides a 64-bit index per element: 14 us for 124 x 11008)
template <typename T>
__global__ __launch_bounds__(256) void llm_silu_mul_vec_kernel(const T* __restrict__ gu, T* __restrict__ act, int I) {
    constexpr int V = 16 / (int)sizeof(T);
    typedef T TV __attribute__((ext_vector_type(V)));
    const int c = (blockIdx.x * 256 + threadIdx.x) * V;
    if (c >= I) return;
    const int64_t r = blockIdx.y;
    const TV g = *reinterpret_cast<const TV*>(gu + r * 2 * I + c), u = *reinterpret_cast<const TV*>(gu + r * 2 * I + I + c);
    TV o;
#pragma unroll
    for (int e = 0; e < V; e++) {
        const float gf = (float)g[e];
        o[e] = Cvt<T>::to(Cvt<T>::rnd(gf / (1.0f + expf(-gf))) * (float)u[e]);
    }
    *reinterpret_cast<TV*>(act + r * I + c) = o;
}

extern "C" int vtgb_llm_rmsnorm(int dtype, void* x, const void* delta, const void* w, void* h, int64_t rows, int32_t H, float eps,
                                vtgb_stream_t s) {
    VTGB_REQUIRE(x && w && h && rows > 0 && H > 0, VTGB_EINVAL, "llm_rmsnorm: bad argument");
    const bool al = (((uintptr_t)x | (uintptr_t)delta | (uintptr_t)w | (uintptr_t)h) & 15) == 0;
    if (dtype == VTGB_BF16 && al && H == 256 * 8 * 2)
        hipLaunchKernelGGL((llm_rmsnorm_vec_kernel<bf16_t, 2>), dim3((unsigned)rows), dim3(256), 0, s, (bf16_t*)x, (const bf16_t*)delta, (const bf16_t*)w, (bf16_t*)h, H, eps);
    else if (dtype == VTGB_BF16 && al && H == 256 * 8)
        hipLaunchKernelGGL((llm_rmsnorm_vec_kernel<bf16_t, 1>), dim3((unsigned)rows), dim3(256), 0, s, (bf16_t*)x, (const bf16_t*)delta, (const bf16_t*)w, (bf16_t*)h, H, eps);
    else if (dtype == VTGB_F32 && al && H == 256 * 4 * 4)
        hipLaunchKernelGGL((llm_rmsnorm_vec_kernel<float, 4>), dim3((unsigned)rows), dim3(256), 0, s, (float*)x, (const float*)delta, (const float*)w, (float*)h, H, eps);
    else if (dtype == VTGB_F32 && al && H == 256 * 4 * 2)
        hipLaunchKernelGGL((llm_rmsnorm_vec_kernel<float, 2>), dim3((unsigned)rows), dim3(256), 0, s, (float*)x, (const float*)delta, (const float*)w, (float*)h, H, eps);
    else if (dtype == VTGB_BF16)
        hipLaunchKernelGGL(llm_rmsnorm_kernel<bf16_t>, dim3((unsigned)rows), dim3(256), 0, s, (bf16_t*)x, (const bf16_t*)delta, (const bf16_t*)w, (bf16_t*)h, H, eps);
    else
        hipLaunchKernelGGL(llm_rmsnorm_kernel<float>, dim3((unsigned)rows), dim3(256), 0, s, (float*)x, (const float*)delta, (const float*)w, (float*)h, H, eps);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

// delta = the K-split fragments of a vtgb_gemm_skinny call with defer_reduce (bf16 activations; M = rows)
extern "C" int vtgb_llm_rmsnorm_parts(int dtype, void* x, const float* part, int32_t S, const void* w, void* h, int64_t rows, int32_t H, float eps,
                                      vtgb_stream_t s) {
    VTGB_REQUIRE(x && part && w && h && rows > 0 && rows <= 128 && S > 1 && dtype == VTGB_BF16, VTGB_EINVAL, "llm_rmsnorm_parts: bad argument");
    VTGB_REQUIRE((((uintptr_t)x | (uintptr_t)part | (uintptr_t)w | (uintptr_t)h) & 15) == 0 && (H == 4096 || H == 2048), VTGB_EUNSUPPORTED,
                 "llm_rmsnorm_parts: hidden size %d (4096 or 2048, 16-byte aligned operands)", H);
    if (H == 4096)
        hipLaunchKernelGGL((llm_rmsnorm_vec_kernel<bf16_t, 2>), dim3((unsigned)rows), dim3(256), 0, s, (bf16_t*)x, (const bf16_t*)nullptr, (const bf16_t*)w, (bf16_t*)h, H, eps,
                           part, S, (int)rows);
    else
        hipLaunchKernelGGL((llm_rmsnorm_vec_kernel<bf16_t, 1>), dim3((unsigned)rows), dim3(256), 0, s, (bf16_t*)x, (const bf16_t*)nullptr, (const bf16_t*)w, (bf16_t*)h, H, eps,
                           part, S, (int)rows);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

extern "C" int vtgb_llm_rope_cache_parts(int dtype, const float* part, int32_t S, void* q_out, void* kc, void* vc, const void* cos_t, const void* sin_t,
                                         const int64_t* pos, int32_t B, int32_t nq, int32_t nkv, int32_t hd, int32_t tmax, vtgb_stream_t s) {
    VTGB_REQUIRE(part && S > 1 && q_out && kc && vc && ((cos_t == nullptr) == (sin_t == nullptr)) && pos && B > 0 && B <= 128 && nq > 0 && nkv > 0 && (hd % 2) == 0 &&
                     dtype == VTGB_BF16,
                 VTGB_EINVAL, "llm_rope_cache_parts: bad argument");
    hipLaunchKernelGGL(llm_rope_cache_kernel<bf16_t>, dim3(nq + 2 * nkv, B), dim3(128), 0, s, (const bf16_t*)nullptr, (bf16_t*)q_out, (bf16_t*)kc, (bf16_t*)vc,
                       (const bf16_t*)cos_t, (const bf16_t*)sin_t, pos, nq, nkv, hd, tmax, part, S, B);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

extern "C" int vtgb_llm_rope_cache_parts_pos(int dtype, const float* part, int32_t S, void* q_out, void* kc, void* vc, const void* cos_t, const void* sin_t,
                                             const int64_t* pos, const int64_t* rope_off, int32_t B, int32_t nq, int32_t nkv, int32_t hd, int32_t tmax,
                                             vtgb_stream_t s) {
    VTGB_REQUIRE(part && S > 1 && q_out && kc && vc && cos_t && sin_t && pos && rope_off && B > 0 && B <= 128 && nq > 0 && nkv > 0 && (hd % 2) == 0 &&
                     tmax > 0 && dtype == VTGB_BF16,
                 VTGB_EINVAL, "llm_rope_cache_parts_pos: bad argument");
    hipLaunchKernelGGL(llm_rope_cache_pos_kernel<bf16_t>, dim3(nq + 2 * nkv, B), dim3(128), 0, s, (const bf16_t*)nullptr, (bf16_t*)q_out, (bf16_t*)kc, (bf16_t*)vc,
                       (const bf16_t*)cos_t, (const bf16_t*)sin_t, pos, rope_off, nq, nkv, hd, tmax, part, S, B);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

// ---- the prefill's counterpart: rotary on q and k of EVERY position, in place in qkv [B, S, (nq + 2 nkv) * hd] (the attention then reads q
// and k from there), k and v copied to the cache rows 0 .. S - 1.  One workgroup per (position, batch); bf16: a thread takes 8 channels of
// the first half of a head together with their partners in the second half (16-byte loads and stores); HF's roundings (each product, then
// the sum: LlamaRotaryEmbedding / apply_rotary_pos_emb in the model's dtype).
// pos_ids != NULL (padded batches): the rotary row of (b, spos) is pos_ids[b, spos] (HF: attention_mask.cumsum(-1) - 1, pads at 0).
template <typename T, bool POS_IDS>
__device__ __forceinline__ void rope_cache_prefill_body(T* __restrict__ qkv, T* __restrict__ kc, T* __restrict__ vc, const T* __restrict__ cos_t,
                                                        const T* __restrict__ sin_t, const int64_t* __restrict__ pos_ids, int S, int nq, int nkv, int hd,
                                                        int tmax) {
#pragma clang fp contract(off)      // fp32: mul, mul, add are three roundings in the reference -- no FMA
    constexpr int V = 16 / (int)sizeof(T);                     // elements per 16-byte vector
    typedef T TV __attribute__((ext_vector_type(V)));
    const int spos = blockIdx.x, b = blockIdx.y, half = hd >> 1, cph = half / V;      // vectors per half head
    T* const row = qkv + ((int64_t)b * S + spos) * (nq + 2 * nkv) * hd;
    int64_t rp = spos;
    if constexpr (POS_IDS) {
        rp = pos_ids[(int64_t)b * S + spos];
        rp = rp < 0 ? 0 : rp >= tmax ? tmax - 1 : rp;
    }
    const T* const cr = cos_t + rp * hd;
    const T* const sr = sin_t + rp * hd;
    for (int it = threadIdx.x; it < (nq + nkv) * cph; it += blockDim.x) {
        const int head = it / cph, d = (it - head * cph) * V;
        T* const hp = row + head * hd;
        const TV x0 = *reinterpret_cast<const TV*>(hp + d), x1 = *reinterpret_cast<const TV*>(hp + d + half);
        const TV c0 = *reinterpret_cast<const TV*>(cr + d), c1 = *reinterpret_cast<const TV*>(cr + d + half);
        const TV s0 = *reinterpret_cast<const TV*>(sr + d), s1 = *reinterpret_cast<const TV*>(sr + d + half);
        TV o0, o1;
#pragma unroll
        for (int e = 0; e < V; e++) {
            // plain operators under `fp contract(off)` (the __fmul_rn / __fadd_rn of the HIP headers are inlined WITH their contract flags)
            const float p00 = Cvt<T>::rnd((float)x0[e] * (float)c0[e]), p01 = Cvt<T>::rnd(-(float)x1[e] * (float)s0[e]);
            const float p10 = Cvt<T>::rnd((float)x1[e] * (float)c1[e]), p11 = Cvt<T>::rnd((float)x0[e] * (float)s1[e]);
            o0[e] = Cvt<T>::to(Cvt<T>::rnd(p00 + p01));
            o1[e] = Cvt<T>::to(Cvt<T>::rnd(p10 + p11));
        }
        *reinterpret_cast<TV*>(hp + d) = o0;
        *reinterpret_cast<TV*>(hp + d + half) = o1;
        if (head >= nq) {
            T* const kd = kc + (((int64_t)b * nkv + (head - nq)) * tmax + spos) * hd;
            *reinterpret_cast<TV*>(kd + d) = o0;
            *reinterpret_cast<TV*>(kd + d + half) = o1;
        }
    }
    for (int it = threadIdx.x; it < nkv * (hd / V); it += blockDim.x) {
        const int head = it / (hd / V), d = (it - head * (hd / V)) * V;
        *reinterpret_cast<TV*>(vc + (((int64_t)b * nkv + head) * tmax + spos) * hd + d) = *reinterpret_cast<const TV*>(row + (nq + nkv + head) * hd + d);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void llm_rope_cache_prefill_kernel(T* __restrict__ qkv, T* __restrict__ kc, T* __restrict__ vc, const T* __restrict__ cos_t,
                                                                     const T* __restrict__ sin_t, int S, int nq, int nkv, int hd, int tmax) {
    rope_cache_prefill_body<T, false>(qkv, kc, vc, cos_t, sin_t, nullptr, S, nq, nkv, hd, tmax);
}

template <typename T>
__global__ __launch_bounds__(256) void llm_rope_cache_prefill_pos_kernel(T* __restrict__ qkv, T* __restrict__ kc, T* __restrict__ vc, const T* __restrict__ cos_t,
                                                                         const T* __restrict__ sin_t, const int64_t* __restrict__ pos_ids, int S, int nq, int nkv,
                                                                         int hd, int tmax) {
    rope_cache_prefill_body<T, true>(qkv, kc, vc, cos_t, sin_t, pos_ids, S, nq, nkv, hd, tmax);
}

extern "C" int vtgb_llm_rope_cache(int dtype, const void* qkv, void* q_out, void* kc, void* vc, const void* cos_t, const void* sin_t,
                                   const int64_t* pos, int32_t B, int32_t nq, int32_t nkv, int32_t hd, int32_t tmax, vtgb_stream_t s) {
    VTGB_REQUIRE(qkv && q_out && kc && vc && ((cos_t == nullptr) == (sin_t == nullptr)) && pos && B > 0 && nq > 0 && nkv > 0 && (hd % 2) == 0, VTGB_EINVAL, "llm_rope_cache: bad argument");
    const dim3 grid(nq + 2 * nkv, B);
    if (dtype == VTGB_BF16)
        hipLaunchKernelGGL(llm_rope_cache_kernel<bf16_t>, grid, dim3(128), 0, s, (const bf16_t*)qkv, (bf16_t*)q_out, (bf16_t*)kc, (bf16_t*)vc,
                           (const bf16_t*)cos_t, (const bf16_t*)sin_t, pos, nq, nkv, hd, tmax);
    else
        hipLaunchKernelGGL(llm_rope_cache_kernel<float>, grid, dim3(128), 0, s, (const float*)qkv, (float*)q_out, (float*)kc, (float*)vc,
                           (const float*)cos_t, (const float*)sin_t, pos, nq, nkv, hd, tmax);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

extern "C" int vtgb_llm_rope_cache_pos(int dtype, const void* qkv, void* q_out, void* kc, void* vc, const void* cos_t, const void* sin_t,
                                       const int64_t* pos, const int64_t* rope_off, int32_t B, int32_t nq, int32_t nkv, int32_t hd, int32_t tmax,
                                       vtgb_stream_t s) {
    VTGB_REQUIRE(qkv && q_out && kc && vc && cos_t && sin_t && pos && rope_off && B > 0 && nq > 0 && nkv > 0 && (hd % 2) == 0 && tmax > 0, VTGB_EINVAL,
                 "llm_rope_cache_pos: bad argument");
    const dim3 grid(nq + 2 * nkv, B);
    if (dtype == VTGB_BF16)
        hipLaunchKernelGGL(llm_rope_cache_pos_kernel<bf16_t>, grid, dim3(128), 0, s, (const bf16_t*)qkv, (bf16_t*)q_out, (bf16_t*)kc, (bf16_t*)vc,
                           (const bf16_t*)cos_t, (const bf16_t*)sin_t, pos, rope_off, nq, nkv, hd, tmax);
    else
        hipLaunchKernelGGL(llm_rope_cache_pos_kernel<float>, grid, dim3(128), 0, s, (const float*)qkv, (float*)q_out, (float*)kc, (float*)vc,
                           (const float*)cos_t, (const float*)sin_t, pos, rope_off, nq, nkv, hd, tmax);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

extern "C" int vtgb_llm_rope_cache_prefill(int dtype, void* qkv, void* kc, void* vc, const void* cos_t, const void* sin_t, int32_t B, int32_t S, int32_t nq,
                                           int32_t nkv, int32_t hd, int32_t tmax, vtgb_stream_t s) {
    VTGB_REQUIRE(qkv && kc && vc && cos_t && sin_t && B > 0 && S > 0 && S <= tmax && nq > 0 && nkv > 0, VTGB_EINVAL, "llm_rope_cache_prefill: bad argument");
    VTGB_REQUIRE(dtype == VTGB_BF16 ? (hd % 16) == 0 : (hd % 8) == 0, VTGB_EUNSUPPORTED, "llm_rope_cache_prefill: head_dim=%d (16-byte vectors per half head)", hd);
    const dim3 grid(S, B);
    if (dtype == VTGB_BF16)
        hipLaunchKernelGGL(llm_rope_cache_prefill_kernel<bf16_t>, grid, dim3(256), 0, s, (bf16_t*)qkv, (bf16_t*)kc, (bf16_t*)vc, (const bf16_t*)cos_t, (const bf16_t*)sin_t,
                           S, nq, nkv, hd, tmax);
    else
        hipLaunchKernelGGL(llm_rope_cache_prefill_kernel<float>, grid, dim3(256), 0, s, (float*)qkv, (float*)kc, (float*)vc, (const float*)cos_t, (const float*)sin_t, S,
                           nq, nkv, hd, tmax);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

extern "C" int vtgb_llm_rope_cache_prefill_pos(int dtype, void* qkv, void* kc, void* vc, const void* cos_t, const void* sin_t, const int64_t* pos_ids,
                                               int32_t B, int32_t S, int32_t nq, int32_t nkv, int32_t hd, int32_t tmax, vtgb_stream_t s) {
    VTGB_REQUIRE(qkv && kc && vc && cos_t && sin_t && pos_ids && B > 0 && S > 0 && S <= tmax && nq > 0 && nkv > 0, VTGB_EINVAL,
                 "llm_rope_cache_prefill_pos: bad argument");
    VTGB_REQUIRE(dtype == VTGB_BF16 ? (hd % 16) == 0 : (hd % 8) == 0, VTGB_EUNSUPPORTED, "llm_rope_cache_prefill_pos: head_dim=%d (16-byte vectors per half head)", hd);
    const dim3 grid(S, B);
    if (dtype == VTGB_BF16)
        hipLaunchKernelGGL(llm_rope_cache_prefill_pos_kernel<bf16_t>, grid, dim3(256), 0, s, (bf16_t*)qkv, (bf16_t*)kc, (bf16_t*)vc, (const bf16_t*)cos_t,
                           (const bf16_t*)sin_t, pos_ids, S, nq, nkv, hd, tmax);
    else
        hipLaunchKernelGGL(llm_rope_cache_prefill_pos_kernel<float>, grid, dim3(256), 0, s, (float*)qkv, (float*)kc, (float*)vc, (const float*)cos_t,
                           (const float*)sin_t, pos_ids, S, nq, nkv, hd, tmax);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

extern "C" int vtgb_llm_decode_attention(int dtype, const void* q, const void* kc, const void* vc, void* out, const int64_t* pos, int32_t B,
                                         int32_t nq, int32_t nkv, int32_t hd, int32_t tmax, float scale, vtgb_stream_t s) {
    VTGB_REQUIRE(q && kc && vc && out && pos && B > 0 && nq > 0 && nkv > 0 && nq % nkv == 0, VTGB_EINVAL, "llm_decode_attention: bad argument");
    VTGB_REQUIRE(tmax <= DEC_MAX_T && hd <= 256, VTGB_EUNSUPPORTED, "llm_decode_attention: tmax=%d hd=%d too large", tmax, hd);
    const size_t lds = 4 * (size_t)(hd + tmax) * sizeof(float);
    const dim3 grid((unsigned)(((int64_t)B * nq + 3) / 4));
    if (dtype == VTGB_BF16)
        hipLaunchKernelGGL(llm_decode_attn_kernel<bf16_t>, grid, dim3(256), lds, s, (const bf16_t*)q, (const bf16_t*)kc, (const bf16_t*)vc, (bf16_t*)out,
                           pos, B, nq, nkv, hd, tmax, scale);
    else
        hipLaunchKernelGGL(llm_decode_attn_kernel<float>, grid, dim3(256), lds, s, (const float*)q, (const float*)kc, (const float*)vc, (float*)out, pos,
                           B, nq, nkv, hd, tmax, scale);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

extern "C" int vtgb_llm_decode_attention_masked(int dtype, const void* q, const void* kc, const void* vc, void* out, const int64_t* pos,
                                                const uint8_t* key_valid, int32_t B, int32_t nq, int32_t nkv, int32_t hd, int32_t tmax, float scale,
                                                vtgb_stream_t s) {
    VTGB_REQUIRE(q && kc && vc && out && pos && key_valid && B > 0 && nq > 0 && nkv > 0 && nq % nkv == 0 && tmax > 0, VTGB_EINVAL,
                 "llm_decode_attention_masked: bad argument");
    VTGB_REQUIRE(tmax <= DEC_MAX_T && hd <= 256, VTGB_EUNSUPPORTED, "llm_decode_attention_masked: tmax=%d hd=%d too large", tmax, hd);
    const size_t lds = 4 * (size_t)(hd + tmax) * sizeof(float);
    const dim3 grid((unsigned)(((int64_t)B * nq + 3) / 4));
    if (dtype == VTGB_BF16)
        hipLaunchKernelGGL(llm_decode_attn_masked_kernel<bf16_t>, grid, dim3(256), lds, s, (const bf16_t*)q, (const bf16_t*)kc, (const bf16_t*)vc, (bf16_t*)out,
                           pos, key_valid, B, nq, nkv, hd, tmax, scale);
    else
        hipLaunchKernelGGL(llm_decode_attn_masked_kernel<float>, grid, dim3(256), lds, s, (const float*)q, (const float*)kc, (const float*)vc, (float*)out,
                           pos, key_valid, B, nq, nkv, hd, tmax, scale);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

extern "C" int vtgb_llm_silu_mul(int dtype, const void* gu, void* act, int64_t rows, int32_t I, vtgb_stream_t s) {
    VTGB_REQUIRE(gu && act && rows > 0 && I > 0, VTGB_EINVAL, "llm_silu_mul: bad argument");
    const int V = dtype == VTGB_BF16 ? 8 : 4;
    if ((I % V) == 0 && rows <= 65535 && ((((uintptr_t)gu | (uintptr_t)act) & 15) == 0)) {
        const dim3 grid((unsigned)((I / V + 255) / 256), (unsigned)rows);
        if (dtype == VTGB_BF16) hipLaunchKernelGGL(llm_silu_mul_vec_kernel<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)gu, (bf16_t*)act, I);
        else hipLaunchKernelGGL(llm_silu_mul_vec_kernel<float>, grid, dim3(256), 0, s, (const float*)gu, (float*)act, I);
        VTGB_HIP(hipGetLastError());
        return VTGB_OK;
    }
    int64_t blocks = (rows * I + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (dtype == VTGB_BF16)
        hipLaunchKernelGGL(llm_silu_mul_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, s, (const bf16_t*)gu, (bf16_t*)act, rows, I);
    else
        hipLaunchKernelGGL(llm_silu_mul_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, s, (const float*)gu, (float*)act, rows, I);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

// ---- attention of independent query rows over strided K / V with an additive per-(query position, head, key) bias: the T5 language
// model of the BLIP-2 flavours (transformers' modeling_t5: unscaled scores + bucketed relative position bias, softmax in fp32).  One
// wave per (row, head), 4 per workgroup.  Row r belongs to K/V batch r / rows_per_batch and query position r % rows_per_batch; it sees
// keys [0, n_keys) -- n_keys fixed, or *pos + 1 (decode step over a static cache, bias row *pos).  Covers the decoder's self-attention
// (rows_per_batch 1, cache [B, H, N, dk], bias), its cross-attention (fixed n_keys = encoder length, no bias) and the ENCODER's
// self-attention (rows = B x P straight out of the q|k|v projection: token-major strides, bias row = query position).
// MASKED (padded encoder inputs): key_valid[b * kv_stride + key] == 0 keys get no weight and their K / V rows are not read (HF: the
// attention mask added to the scores as finfo.min -- an exact 0 after the softmax).
template <typename T, bool MASKED>
__device__ __forceinline__ void attn_rows_body(const vtgb_llm_attn_rows_args& a, const uint8_t* __restrict__ key_valid, int64_t kv_stride) {
    extern __shared__ float dsm[];   // per wave: hd floats of q + t_pad scores
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int hd = a.head_dim, nq = a.heads;
    const int64_t idx = (int64_t)blockIdx.x * 4 + wave;
    const int64_t total = (int64_t)a.rows * nq;
    const int64_t id = idx < total ? idx : total - 1;
    const int64_t r = id / nq;
    const int head = (int)(id - r * nq);
    const int64_t b = r / a.rows_per_batch;
    const int qpos = a.pos ? (int)(*a.pos) : (int)(r - b * a.rows_per_batch);
    const int n_keys = a.pos ? (int)(*a.pos) + 1 : a.n_keys;
    float* qs = dsm + wave * (hd + a.t_pad);
    float* sc = qs + hd;
    const T* qr = reinterpret_cast<const T*>(a.q) + r * a.q_row + (int64_t)head * hd;
    const T* kr = reinterpret_cast<const T*>(a.k) + b * a.kv_batch + (int64_t)head * a.kv_head;
    const T* vr = reinterpret_cast<const T*>(a.v) + b * a.kv_batch + (int64_t)head * a.kv_head;
    const T* br = a.bias ? reinterpret_cast<const T*>(a.bias) + (int64_t)qpos * a.bias_pos + (int64_t)head * a.bias_head : nullptr;
    for (int d = lane; d < hd; d += 64) qs[d] = (float)qr[d];
    __syncthreads();
    float mx = -INFINITY;
    const uint8_t* kvr = MASKED ? key_valid + b * kv_stride : nullptr;
    for (int key = lane; key < n_keys; key += 64) {
        if constexpr (MASKED) {
            if (!kvr[key]) {
                sc[key] = -INFINITY;
                continue;
            }
        }
        const T* k = kr + (int64_t)key * a.kv_tok;
        float dot = 0.f;
        for (int d = 0; d < hd; d++) dot = fmaf(qs[d], (float)k[d], dot);
        dot = Cvt<T>::rnd(dot * a.scale);                    // HF: scores in the model's dtype ...
        if (br) dot = Cvt<T>::rnd(dot + (float)br[key]);     // ... += position_bias, softmax in fp32
        sc[key] = dot;
        mx = fmaxf(mx, dot);
    }
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    float sum = 0.f;
    for (int key = lane; key < n_keys; key += 64) {
        const float e = MASKED && sc[key] == -INFINITY ? 0.f : expf(sc[key] - mx);
        sc[key] = e;
        sum += e;
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    __syncthreads();
    const float inv = MASKED && sum == 0.f ? 0.f : 1.0f / sum;
    if (idx < total) {
        T* o = reinterpret_cast<T*>(a.out) + r * a.o_row + (int64_t)head * hd;
        for (int d = lane; d < hd; d += 64) {
            float acc = 0.f;
            for (int key = 0; key < n_keys; key++) {
                // (MASKED, zero weight: the load goes to row n_keys - 1 and the value is selected away -- no branch, see decode_attn_body)
                const bool skip = MASKED && sc[key] == 0.f;
                const float v = (float)vr[(int64_t)(skip ? n_keys - 1 : key) * a.kv_tok + d];
                acc = fmaf(Cvt<T>::rnd(sc[key] * inv), skip ? 0.f : v, acc);      // (weights as the model's dtype holds them)
            }
            o[d] = Cvt<T>::to(acc);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void llm_attn_rows_kernel(const vtgb_llm_attn_rows_args a) {
    attn_rows_body<T, false>(a, nullptr, 0);
}

template <typename T>
__global__ __launch_bounds__(256) void llm_attn_rows_masked_kernel(const vtgb_llm_attn_rows_args a, const uint8_t* __restrict__ key_valid, int64_t kv_stride) {
    attn_rows_body<T, true>(a, key_valid, kv_stride);
}

static int attn_rows_check(const vtgb_llm_attn_rows_args* a) {
    VTGB_REQUIRE(a && a->q && a->k && a->v && a->out && a->rows > 0 && a->heads > 0 && a->head_dim > 0 && a->rows_per_batch > 0, VTGB_EINVAL,
                 "llm_attention_rows: bad argument");
    VTGB_REQUIRE(a->pos || a->n_keys > 0, VTGB_EINVAL, "llm_attention_rows: n_keys or pos");
    VTGB_REQUIRE(a->t_pad >= (a->pos ? 1 : a->n_keys) && a->t_pad <= DEC_MAX_T && a->head_dim <= 256, VTGB_EUNSUPPORTED,
                 "llm_attention_rows: t_pad=%d head_dim=%d outside [n_keys .. %d], <= 256", a->t_pad, a->head_dim, DEC_MAX_T);
    return VTGB_OK;
}

extern "C" int vtgb_llm_attention_rows(const vtgb_llm_attn_rows_args* a, vtgb_stream_t s) {
    if (const int rc = attn_rows_check(a)) return rc;
    const size_t lds = 4 * (size_t)(a->head_dim + a->t_pad) * sizeof(float);
    const dim3 grid((unsigned)(((int64_t)a->rows * a->heads + 3) / 4));
    if (a->dtype == VTGB_BF16) hipLaunchKernelGGL(llm_attn_rows_kernel<bf16_t>, grid, dim3(256), lds, s, *a);
    else hipLaunchKernelGGL(llm_attn_rows_kernel<float>, grid, dim3(256), lds, s, *a);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

extern "C" int vtgb_llm_attention_rows_masked(const vtgb_llm_attn_rows_args* a, const uint8_t* key_valid, int64_t key_valid_batch_stride, vtgb_stream_t s) {
    if (const int rc = attn_rows_check(a)) return rc;
    VTGB_REQUIRE(key_valid && key_valid_batch_stride >= (a->pos ? a->t_pad : a->n_keys), VTGB_EINVAL,
                 "llm_attention_rows_masked: key_valid and a batch stride >= the key count");
    const size_t lds = 4 * (size_t)(a->head_dim + a->t_pad) * sizeof(float);
    const dim3 grid((unsigned)(((int64_t)a->rows * a->heads + 3) / 4));
    if (a->dtype == VTGB_BF16) hipLaunchKernelGGL(llm_attn_rows_masked_kernel<bf16_t>, grid, dim3(256), lds, s, *a, key_valid, key_valid_batch_stride);
    else hipLaunchKernelGGL(llm_attn_rows_masked_kernel<float>, grid, dim3(256), lds, s, *a, key_valid, key_valid_batch_stride);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

// ---- beam search on the T5 decoder (opt-in: beam_search="graph+t5"): attn_rows_body's decode form (pos given, keys [0, *pos], bias row
// *pos) where K and V of key t of query row r come from cache row clamp(src_row[r * src_stride + t], 0, cache_rows - 1) -- the beam that
// wrote slot t of row r's ancestry -- instead of row r / rows_per_batch, so re-ordering beams re-orders an int32 table and never K/V.  The
// lane that owns key t (t % 64) reads its table entry once and leaves the clamped row in LDS next to the score; the V pass reads it back
// for every lane (one address per wave: a broadcast).  Rounding points and the order of every sum are attn_rows_body's, so the output
// equals vtgb_llm_attention_rows on the gathered cache bit for bit.  Table entries and K/V slots past *pos are never read (*pos itself is
// clamped to t_pad - 1: the score and row buffers hold t_pad entries).
constexpr int ATTN_ROWS_BEAM_MAX_T = VTGB_LLM_ATTN_ROWS_BEAM_MAX_T;      // 1920: 4 waves x (head_dim <= 256 + 2 x t_pad) words = the 64 KiB a launch gets without opting in to more

template <typename T>
__global__ __launch_bounds__(256) void llm_attn_rows_beam_kernel(const vtgb_llm_attn_rows_args a, const int32_t* __restrict__ src_row, int64_t src_stride,
                                                                 int cache_rows) {
    extern __shared__ float dsm[];   // per wave: hd floats of q + t_pad scores + t_pad cache rows
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int hd = a.head_dim, nq = a.heads;
    const int64_t idx = (int64_t)blockIdx.x * 4 + wave;
    const int64_t total = (int64_t)a.rows * nq;
    const int64_t id = idx < total ? idx : total - 1;
    const int64_t r = id / nq;
    const int head = (int)(id - r * nq);
    const int64_t p64 = *a.pos;
    const int qpos = (int)(p64 < 0 ? 0 : p64 >= a.t_pad ? a.t_pad - 1 : p64);
    const int n_keys = p64 < 0 ? 0 : qpos + 1;
    float* qs = dsm + wave * (hd + 2 * a.t_pad);
    float* sc = qs + hd;
    int* rows = reinterpret_cast<int*>(sc + a.t_pad);
    const T* qr = reinterpret_cast<const T*>(a.q) + r * a.q_row + (int64_t)head * hd;
    const T* kr = reinterpret_cast<const T*>(a.k) + (int64_t)head * a.kv_head;
    const T* vr = reinterpret_cast<const T*>(a.v) + (int64_t)head * a.kv_head;
    const T* br = a.bias ? reinterpret_cast<const T*>(a.bias) + (int64_t)qpos * a.bias_pos + (int64_t)head * a.bias_head : nullptr;
    const int32_t* sr = src_row + r * src_stride;
    for (int d = lane; d < hd; d += 64) qs[d] = (float)qr[d];
    __syncthreads();
    float mx = -INFINITY;
    for (int key = lane; key < n_keys; key += 64) {
        const int s = sr[key];
        const int row = s < 0 ? 0 : s >= cache_rows ? cache_rows - 1 : s;
        rows[key] = row;
        const T* k = kr + (int64_t)row * a.kv_batch + (int64_t)key * a.kv_tok;
        float dot = 0.f;
        for (int d = 0; d < hd; d++) dot = fmaf(qs[d], (float)k[d], dot);
        dot = Cvt<T>::rnd(dot * a.scale);
        if (br) dot = Cvt<T>::rnd(dot + (float)br[key]);
        sc[key] = dot;
        mx = fmaxf(mx, dot);
    }
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    float sum = 0.f;
    for (int key = lane; key < n_keys; key += 64) {
        const float e = expf(sc[key] - mx);
        sc[key] = e;
        sum += e;
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    __syncthreads();
    const float inv = 1.0f / sum;
    if (idx < total) {
        T* o = reinterpret_cast<T*>(a.out) + r * a.o_row + (int64_t)head * hd;
        for (int d = lane; d < hd; d += 64) {
            float acc = 0.f;
            for (int key = 0; key < n_keys; key++) {
                const float v = (float)vr[(int64_t)rows[key] * a.kv_batch + (int64_t)key * a.kv_tok + d];
                acc = fmaf(Cvt<T>::rnd(sc[key] * inv), v, acc);
            }
            o[d] = Cvt<T>::to(acc);
        }
    }
}

extern "C" int vtgb_llm_attention_rows_beam(const vtgb_llm_attn_rows_args* a, const int32_t* src_row, int64_t src_row_stride, int32_t cache_rows,
                                            vtgb_stream_t s) {
    if (const int rc = attn_rows_check(a)) return rc;
    VTGB_REQUIRE(src_row && a->pos && cache_rows >= 1 && src_row_stride >= a->t_pad, VTGB_EINVAL,
                 "llm_attention_rows_beam: src_row, pos, cache_rows >= 1 and a table stride >= t_pad");
    VTGB_REQUIRE(a->t_pad <= ATTN_ROWS_BEAM_MAX_T, VTGB_EUNSUPPORTED, "llm_attention_rows_beam: t_pad=%d, built for up to %d (scores and the table in LDS)",
                 a->t_pad, ATTN_ROWS_BEAM_MAX_T);
    const size_t lds = 4 * (size_t)(a->head_dim + 2 * a->t_pad) * sizeof(float);
    const dim3 grid((unsigned)(((int64_t)a->rows * a->heads + 3) / 4));
    if (a->dtype == VTGB_BF16) hipLaunchKernelGGL(llm_attn_rows_beam_kernel<bf16_t>, grid, dim3(256), lds, s, *a, src_row, src_row_stride, cache_rows);
    else hipLaunchKernelGGL(llm_attn_rows_beam_kernel<float>, grid, dim3(256), lds, s, *a, src_row, src_row_stride, cache_rows);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

// ---- feed-forward activations of the language models: act[r, i] = f(gu[r, i]) (* gu[r, I + i] when gated).  kind 0 SiLU (Llama's SwiGLU = vtgb_llm_silu_mul),
// 1 gelu_new (T5 v1.1 / Flan-T5 "gated-gelu": 0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3)))), 2 ReLU (original T5), 3 exact GELU.
template <typename T>
__global__ void llm_gated_act_kernel(const T* __restrict__ gu, T* __restrict__ act, int64_t rows, int I, int kind, int gated) {
    const int64_t n = rows * I;
    const int ld = gated ? 2 * I : I;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / I, c = i - r * I;
        const float g = (float)gu[r * ld + c];
        float f;
        if (kind == 0) f = g / (1.0f + expf(-g));
        else if (kind == 1) f = 0.5f * g * (1.0f + tanhf(0.7978845608028654f * (g + 0.044715f * g * g * g)));
        else if (kind == 2) f = fmaxf(g, 0.f);
        else f = 0.5f * g * (1.0f + erff(g * 0.70710678118654752440f));
        f = Cvt<T>::rnd(f);
        act[i] = gated ? Cvt<T>::to(f * (float)gu[r * ld + I + c]) : Cvt<T>::to(f);
    }
}

extern "C" int vtgb_llm_gated_act(int dtype, const void* gu, void* act, int64_t rows, int32_t I, int32_t kind, int32_t gated, vtgb_stream_t s) {
    VTGB_REQUIRE(gu && act && rows > 0 && I > 0 && kind >= 0 && kind <= 3, VTGB_EINVAL, "llm_gated_act: bad argument");
    int64_t blocks = (rows * I + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (dtype == VTGB_BF16)
        hipLaunchKernelGGL(llm_gated_act_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, s, (const bf16_t*)gu, (bf16_t*)act, rows, I, kind, gated);
    else
        hipLaunchKernelGGL(llm_gated_act_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, s, (const float*)gu, (float*)act, rows, I, kind, gated);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

// ---- fp8 K/V cache (opt-in: kv_cache="fp8"; attn_decode.hip reads it).  The writers: rotary + append of the decode step and rotary +
// cache fill of the prefill, with the row quantisation of ops.quantize_fp8_kv (fp8_code.h: e from the row's amax, clamped at -100, codes =
// row * 2^-e rounded to nearest even) reproduced bit for bit.  One WAVE per head row (one token of one head), so the row's amax is a
// wave reduction: no atomics, no LDS.  A lane holds the channel pair (d, d + hd / 2), d = lane < hd / 2 -- rotary partners, so the
// arithmetic is rope_cache_body's / rope_cache_prefill_body's with both operands in registers (hd <= 128: one pair per lane).
#include "fp8_code.h"

// largest |value| of the wave's row: every lane ends with it
__device__ __forceinline__ float kv8_wave_amax(float a, float b) {
    float m = fmaxf(fabsf(a), fabsf(b));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    return m;
}

// the value an e4m3 code stands for (exact)
__device__ __forceinline__ float kv8_value(uint8_t code) {
    float o[4];
    kv8_widen4(code, o);
    return o[0];
}

// Decode step: grid (ceil((nq + 2 nkv) / 4), B), 4 waves = 4 head rows per workgroup.  q heads: q_out as vtgb_llm_rope_cache writes it;
// k heads: rotary, rounded to bf16, quantised into row *pos of kc8 / ks; v heads: quantised into row *pos of vc8 / vs.
__global__ __launch_bounds__(256) void llm_rope_cache_fp8_kernel(const vtgb_llm_rope_cache_fp8_args a) {
#pragma clang fp contract(off)      // (rope_cache_body's three roundings, no FMA)
    const int nq = a.nq, nkv = a.nkv, hd = a.hd, half = hd >> 1;
    const int b = blockIdx.y, head = blockIdx.x * 4 + (threadIdx.x >> 6), d = threadIdx.x & 63;
    if (head >= nq + 2 * nkv) return;      // (whole waves)
    const int64_t pos = *a.pos;
    int64_t rp = pos;
    if (a.rope_off) rp += a.rope_off[b];
    rp = rp < 0 ? 0 : rp >= a.tmax ? a.tmax - 1 : rp;      // (the tables have tmax rows; the decoder keeps rp in [0, pos])
    const bf16_t* src = a.qkv ? (const bf16_t*)a.qkv + ((int64_t)b * (nq + 2 * nkv) + head) * hd : nullptr;
    const float* part = a.part;
    const int S = a.n_splits, M = a.B;
    auto at = [&](int dd) -> float {      // (rope_cache_body's: the value, or the fragments' sum in split order rounded once)
        if (!part) return (float)src[dd];
        const int col = head * hd + dd;
        float t = 0.f;
        for (int sp = 0; sp < S; sp++) t += part[((int64_t)((col >> 7) * S + sp) * M + b) * 128 + (col & 127)];
        return Cvt<bf16_t>::rnd(t);
    };
    const bool active = d < half;
    float o0 = 0.f, o1 = 0.f;
    if (active) {
        const float x0 = at(d), x1 = at(d + half);
        o0 = x0, o1 = x1;
        if (head < nq + nkv) {
            const bf16_t* cr = (const bf16_t*)a.cos_t + rp * hd;
            const bf16_t* sr = (const bf16_t*)a.sin_t + rp * hd;
            const float c0 = (float)cr[d], s0 = (float)sr[d], c1 = (float)cr[d + half], s1 = (float)sr[d + half];
            const float p00 = Cvt<bf16_t>::rnd(x0 * c0), p01 = Cvt<bf16_t>::rnd(-x1 * s0);
            const float p10 = Cvt<bf16_t>::rnd(x1 * c1), p11 = Cvt<bf16_t>::rnd(x0 * s1);
            o0 = Cvt<bf16_t>::rnd(p00 + p01);
            o1 = Cvt<bf16_t>::rnd(p10 + p11);
        }
    }
    if (head < nq) {
        if (active) {
            bf16_t* qo = (bf16_t*)a.q_out + ((int64_t)b * nq + head) * hd;
            qo[d] = (bf16_t)o0;
            qo[d + half] = (bf16_t)o1;
        }
        return;
    }
    if (pos < 0 || pos >= a.tmax) return;      // (no cache row to write)
    const bool isk = head < nq + nkv;
    const int64_t row = ((int64_t)b * nkv + (isk ? head - nq : head - nq - nkv)) * a.tmax + pos;
    const int e = kv8_row_exp(kv8_wave_amax(o0, o1));
    if (active) {
        uint8_t* c8 = (isk ? a.kc8 : a.vc8) + row * hd;
        c8[d] = sk8_code(ldexpf(o0, -e));
        c8[d + half] = sk8_code(ldexpf(o1, -e));
    }
    if (d == 0) (isk ? a.ks : a.vs)[row] = ldexpf(1.f, e);
}

// Prefill: grid (S, B), 4 waves; wave w takes the head rows w, w + 4 ... of its position.  q and k rotated in place in qkv as
// vtgb_llm_rope_cache_prefill{,_pos} does; codes and scales of k and v into the cache rows 0 .. S - 1; and the DEQUANTISED k and v written
// back in place, so that the prefill attention (unchanged kernels) attends over the values every later step reads from the cache.
__global__ __launch_bounds__(256) void llm_rope_cache_prefill_fp8_kernel(bf16_t* __restrict__ qkv, uint8_t* __restrict__ kc8, uint8_t* __restrict__ vc8,
                                                                         float* __restrict__ ks, float* __restrict__ vs, const bf16_t* __restrict__ cos_t,
                                                                         const bf16_t* __restrict__ sin_t, const int64_t* __restrict__ pos_ids, int S, int nq,
                                                                         int nkv, int hd, int tmax) {
#pragma clang fp contract(off)
    const int spos = blockIdx.x, b = blockIdx.y, half = hd >> 1, d = threadIdx.x & 63;
    bf16_t* const row = qkv + ((int64_t)b * S + spos) * (nq + 2 * nkv) * hd;
    int64_t rp = spos;
    if (pos_ids) {
        rp = pos_ids[(int64_t)b * S + spos];
        rp = rp < 0 ? 0 : rp >= tmax ? tmax - 1 : rp;
    }
    const bf16_t* const cr = cos_t + rp * hd;
    const bf16_t* const sr = sin_t + rp * hd;
    const bool active = d < half;
    for (int head = threadIdx.x >> 6; head < nq + 2 * nkv; head += 4) {
        bf16_t* const hp = row + head * hd;
        float o0 = 0.f, o1 = 0.f;
        if (active) {
            const float x0 = (float)hp[d], x1 = (float)hp[d + half];
            o0 = x0, o1 = x1;
            if (head < nq + nkv) {
                const float c0 = (float)cr[d], s0 = (float)sr[d], c1 = (float)cr[d + half], s1 = (float)sr[d + half];
                const float p00 = Cvt<bf16_t>::rnd(x0 * c0), p01 = Cvt<bf16_t>::rnd(-x1 * s0);
                const float p10 = Cvt<bf16_t>::rnd(x1 * c1), p11 = Cvt<bf16_t>::rnd(x0 * s1);
                o0 = Cvt<bf16_t>::rnd(p00 + p01);
                o1 = Cvt<bf16_t>::rnd(p10 + p11);
            }
        }
        if (head >= nq) {
            const bool isk = head < nq + nkv;
            const int64_t crow = ((int64_t)b * nkv + (isk ? head - nq : head - nq - nkv)) * tmax + spos;
            const int e = kv8_row_exp(kv8_wave_amax(o0, o1));
            const float sc = ldexpf(1.f, e);
            if (active) {
                const uint8_t q0 = sk8_code(ldexpf(o0, -e)), q1 = sk8_code(ldexpf(o1, -e));
                uint8_t* c8 = (isk ? kc8 : vc8) + crow * hd;
                c8[d] = q0;
                c8[d + half] = q1;
                o0 = kv8_value(q0) * sc;      // (exact: a bf16 number)
                o1 = kv8_value(q1) * sc;
            }
            if (d == 0) (isk ? ks : vs)[crow] = sc;
        }
        if (active) {
            hp[d] = (bf16_t)o0;
            hp[d + half] = (bf16_t)o1;
        }
    }
}

extern "C" int vtgb_llm_rope_cache_fp8(const vtgb_llm_rope_cache_fp8_args* a, vtgb_stream_t s) {
    VTGB_REQUIRE(a, VTGB_EINVAL, "llm_rope_cache_fp8: NULL args");
    VTGB_REQUIRE(a->q_out && a->kc8 && a->vc8 && a->ks && a->vs && a->cos_t && a->sin_t && a->pos, VTGB_EINVAL, "llm_rope_cache_fp8: NULL operand");
    VTGB_REQUIRE((a->qkv != nullptr) != (a->part != nullptr), VTGB_EINVAL, "llm_rope_cache_fp8: exactly one of qkv and part");
    VTGB_REQUIRE(!a->part || (a->n_splits > 1 && a->B <= 128), VTGB_EINVAL, "llm_rope_cache_fp8: part needs n_splits > 1 and B <= 128");
    VTGB_REQUIRE(a->dtype == VTGB_BF16 && a->B > 0 && a->B <= 65535 && a->nq > 0 && a->nkv > 0 && a->tmax > 0, VTGB_EINVAL,
                 "llm_rope_cache_fp8: bad argument (activations are VTGB_BF16)");
    VTGB_REQUIRE(a->hd == 64 || a->hd == 128, VTGB_EUNSUPPORTED, "llm_rope_cache_fp8: hd=%d, built for 64 and 128", a->hd);
    hipLaunchKernelGGL(llm_rope_cache_fp8_kernel, dim3((a->nq + 2 * a->nkv + 3) / 4, a->B), dim3(256), 0, (hipStream_t)s, *a);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

extern "C" int vtgb_llm_rope_cache_prefill_fp8(int dtype, void* qkv, uint8_t* kc8, uint8_t* vc8, float* ks, float* vs, const void* cos_t,
                                               const void* sin_t, const int64_t* pos_ids, int32_t B, int32_t S, int32_t nq, int32_t nkv, int32_t hd,
                                               int32_t tmax, vtgb_stream_t s) {
    VTGB_REQUIRE(qkv && kc8 && vc8 && ks && vs && cos_t && sin_t, VTGB_EINVAL, "llm_rope_cache_prefill_fp8: NULL operand");
    VTGB_REQUIRE(dtype == VTGB_BF16 && B > 0 && B <= 65535 && S > 0 && S <= tmax && nq > 0 && nkv > 0, VTGB_EINVAL,
                 "llm_rope_cache_prefill_fp8: bad argument (activations are VTGB_BF16)");
    VTGB_REQUIRE(hd == 64 || hd == 128, VTGB_EUNSUPPORTED, "llm_rope_cache_prefill_fp8: hd=%d, built for 64 and 128", hd);
    hipLaunchKernelGGL(llm_rope_cache_prefill_fp8_kernel, dim3(S, B), dim3(256), 0, (hipStream_t)s, (bf16_t*)qkv, kc8, vc8, ks, vs, (const bf16_t*)cos_t,
                       (const bf16_t*)sin_t, pos_ids, S, nq, nkv, hd, tmax);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}
