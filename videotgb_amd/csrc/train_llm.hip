// train_llm.hip -- what the language model's TRAINING pass (train.llama_with_grad: a Llama under LoRA, config C5) needs next to the GEMM of
// train_ops.hip: fp32, token-major, forward and backward, every sum in a fixed order and no atomics (a launch is bit-reproducible).
//
//   vtgb_rmsnorm_train_forward / _backward   LlamaRMSNorm with the residual add in front of it:  sum = x (+ delta),
//                                             y = gamma * (sum * rstd),  rstd = rsqrt(mean(sum^2) + eps);
//                                             ds = rstd (g . dy) - sum rstd^3 / D  SUM(g . dy . sum) (+ dsum: what the residual stream
//                                             brings back to `sum` from its later consumers)              (gamma is frozen: no dgamma)
//   vtgb_rope_train                           apply_rotary_pos_emb (rotate-half form) on the q and k heads of a [B, S, (nh + 2 nkv) hd] projection,
//                                             v copied; `conjugate` applies the transposed rotation = the backward
//   vtgb_swiglu_train_forward / _backward     act = silu(gate) * up on gu = [gate | up];  silu'(g) = sig(g) (1 + g (1 - sig(g)))
//   vtgb_attn_train_causal_forward / _backward   the attention of train_attn.hip with a causal key range (key chunks above the diagonal are
//                                             never staged, the diagonal chunk is masked per element) and grouped heads (query head h reads K/V
//                                             head h / group; dk / dv of a K/V head are summed over its query heads in head order in one workgroup)
//
// The attention keeps train_attn.hip's shape -- four lanes per row, the other operand through LDS in chunks of 64 rows -- but one workgroup
// per 64-row chunk (grid.y) instead of a loop over the chunks: a language-model batch has few (batch, head) pairs per CU and long rows.
#include <math.h>

#include "common.h"

constexpr int TC_ROWS = 64;   // rows per LDS chunk = rows per workgroup (256 threads / 4 lanes per row)

__device__ __forceinline__ float tl_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ============================================================================ RMSNorm
// one wave per row, four rows per workgroup; the row is parked in y between the two passes (this lane's own elements)
__global__ __launch_bounds__(256) void rmsnorm_train_fwd_kernel(const vtgb_rmsnorm_train_args a) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.rows) return;
    const int D = a.D;
    const float* x = a.x + (int64_t)row * D;
    const float* dl = a.delta ? a.delta + (int64_t)row * D : nullptr;
    float* sp = a.sum ? a.sum + (int64_t)row * D : nullptr;
    float* y = a.y + (int64_t)row * D;
    float acc = 0.f;
    for (int c = lane * 4; c < D; c += 256) {
        f32x4 v = *reinterpret_cast<const f32x4*>(x + c);
        if (dl) v += *reinterpret_cast<const f32x4*>(dl + c);
        if (sp) *reinterpret_cast<f32x4*>(sp + c) = v;
        *reinterpret_cast<f32x4*>(y + c) = v;
        acc += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
    }
    const float rstd = rsqrtf(tl_wave_sum(acc) / (float)D + a.eps);
    for (int c = lane * 4; c < D; c += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(y + c) * rstd;
        *reinterpret_cast<f32x4*>(y + c) = *reinterpret_cast<const f32x4*>(a.gamma + c) * v;
    }
    if (lane == 0) a.rstd[row] = rstd;
}

__global__ __launch_bounds__(256) void rmsnorm_train_bwd_kernel(const vtgb_rmsnorm_train_args a) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.rows) return;
    const int D = a.D;
    const float* s = a.sum + (int64_t)row * D;
    const float* dy = a.dy + (int64_t)row * D;
    const float* dsum = a.dsum ? a.dsum + (int64_t)row * D : nullptr;
    float* ds = a.ds + (int64_t)row * D;
    float acc = 0.f;
    for (int c = lane * 4; c < D; c += 256) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(a.gamma + c) * *reinterpret_cast<const f32x4*>(dy + c);
        const f32x4 gs = g * *reinterpret_cast<const f32x4*>(s + c);
        acc += (gs[0] + gs[1]) + (gs[2] + gs[3]);
    }
    const float rstd = a.rstd[row];
    const float k = rstd * rstd * rstd / (float)D * tl_wave_sum(acc);
    for (int c = lane * 4; c < D; c += 256) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(a.gamma + c) * *reinterpret_cast<const f32x4*>(dy + c);
        f32x4 d = g * rstd - *reinterpret_cast<const f32x4*>(s + c) * k;
        if (dsum) d += *reinterpret_cast<const f32x4*>(dsum + c);
        *reinterpret_cast<f32x4*>(ds + c) = d;
    }
}

// ============================================================================ rotary embedding
// one thread per (token, head, i < hd / 2): the pair (x[i], x[i + hd/2]).  forward  y1 = c1 x1 - s1 x2,  y2 = c2 x2 + s2 x1
// (q cos + rotate_half(q) sin with the table's own two halves);  conjugate  y1 = c1 x1 + s2 x2,  y2 = c2 x2 - s1 x1  (its transpose)
__global__ __launch_bounds__(256) void rope_train_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ cs,
                                                         const float* __restrict__ sn, int64_t n_pairs, int S, int nh, int nkv, int hd, int conjugate) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_pairs) return;
    const int half = hd >> 1, heads = nh + 2 * nkv;
    const int64_t t = idx / half;
    const int i = (int)(idx - t * half);
    const int64_t tok = t / heads;
    const int h = (int)(t - tok * heads), pos = (int)(tok % S);
    const int64_t base = t * hd;
    const float x1 = x[base + i], x2 = x[base + half + i];
    float y1 = x1, y2 = x2;
    if (h < nh + nkv) {
        const float* c = cs + (int64_t)pos * hd;
        const float* s = sn + (int64_t)pos * hd;
        if (!conjugate) {
            y1 = x1 * c[i] - x2 * s[i];
            y2 = x2 * c[half + i] + x1 * s[half + i];
        } else {
            y1 = x1 * c[i] + x2 * s[half + i];
            y2 = x2 * c[half + i] - x1 * s[i];
        }
    }
    y[base + i] = y1;
    y[base + half + i] = y2;
}

// ============================================================================ SwiGLU
__global__ __launch_bounds__(256) void swiglu_train_fwd_kernel(const float* __restrict__ gu, float* __restrict__ act, int64_t n, int I) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int64_t m = idx / I;
    const int c = (int)(idx - m * I);
    const float g = gu[m * 2 * I + c], u = gu[m * 2 * I + I + c];
    act[idx] = g / (1.0f + expf(-g)) * u;
}

__global__ __launch_bounds__(256) void swiglu_train_bwd_kernel(const float* __restrict__ gu, const float* __restrict__ dact, float* __restrict__ dgu,
                                                               int64_t n, int I) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int64_t m = idx / I;
    const int c = (int)(idx - m * I);
    const float g = gu[m * 2 * I + c], u = gu[m * 2 * I + I + c], d = dact[idx];
    const float sig = 1.0f / (1.0f + expf(-g));
    dgu[m * 2 * I + c] = d * u * (sig * (1.0f + g * (1.0f - sig)));
    dgu[m * 2 * I + I + c] = d * (g * sig);
}

// ============================================================================ causal attention with grouped heads
template <int EPL>
__device__ __forceinline__ float tc_dot4(const float (&a)[EPL], const float* __restrict__ b) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; e++) s = fmaf(a[e], b[e], s);
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    return s;
}

// rows [r0, r0 + TC_ROWS) of a [*, heads * hd] token-major operand into LDS as [TC_ROWS][4 * EPL] (zero padded), times `mul`
template <int EPL>
__device__ __forceinline__ void tc_stage_rows(float* lds, const float* __restrict__ src, int64_t tok_stride, int r0, int n_rows, int hd, float mul) {
    constexpr int W = 4 * EPL;
    for (int idx = threadIdx.x; idx < TC_ROWS * W; idx += blockDim.x) {
        const int r = idx / W, c = idx - r * W;
        float v = 0.f;
        if (r0 + r < n_rows && c < hd) v = src[(int64_t)(r0 + r) * tok_stride + c] * mul;
        lds[idx] = v;
    }
}

// grid (batch * heads, query chunks): four lanes per QUERY row; the key chunks 0 .. the workgroup's own stream through LDS
template <int EPL>
__global__ __launch_bounds__(256) void attn_causal_fwd_kernel(const vtgb_attn_train_args a, const int group) {
    constexpr int W = 4 * EPL;
    __shared__ float Ks[TC_ROWS * W], Vs[TC_ROWS * W];
    const int bh = blockIdx.x, b = bh / a.heads, h = bh - b * a.heads, hd = a.head_dim, S = a.s_q;
    const int sub = threadIdx.x & 3, slot = threadIdx.x >> 2, c0 = sub * EPL;
    const int i0 = blockIdx.y * TC_ROWS, i = i0 + slot;
    const bool live = i < S;
    const float* qb = a.q + (int64_t)b * a.q_batch + h * hd;
    const float* kb = a.k + (int64_t)b * a.kv_batch + (h / group) * hd;
    const float* vb = a.v + (int64_t)b * a.kv_batch + (h / group) * hd;
    float q[EPL], o[EPL];
#pragma unroll
    for (int e = 0; e < EPL; e++) {
        q[e] = (live && c0 + e < hd) ? qb[(int64_t)i * a.q_tok + c0 + e] * a.scale : 0.f;
        o[e] = 0.f;
    }
    float m = -INFINITY, l = 0.f;
    for (int j0 = 0; j0 <= i0; j0 += TC_ROWS) {
        __syncthreads();
        tc_stage_rows<EPL>(Ks, kb, a.kv_tok, j0, S, hd, 1.0f);
        tc_stage_rows<EPL>(Vs, vb, a.kv_tok, j0, S, hd, 1.0f);
        __syncthreads();
        const int nj = min(TC_ROWS, S - j0);
        for (int j = 0; j < nj; j++) {
            float s = tc_dot4<EPL>(q, Ks + j * W + c0);
            if (a.key_mask) s += a.key_mask[(int64_t)b * S + j0 + j];
            if (j0 + j <= i) {                                                                 // (the four lanes of a row agree)
                const float mn = fmaxf(m, s), alpha = __expf(m - mn), p = __expf(s - mn);      // (m = -inf: alpha = 0)
                l = l * alpha + p;
#pragma unroll
                for (int e = 0; e < EPL; e++) o[e] = fmaf(p, Vs[j * W + c0 + e], o[e] * alpha);
                m = mn;
            }
        }
    }
    if (live) {
        const float inv = 1.0f / l;
#pragma unroll
        for (int e = 0; e < EPL; e++)
            if (c0 + e < hd) a.out[(int64_t)b * a.o_batch + (int64_t)i * a.o_tok + h * hd + c0 + e] = o[e] * inv;
        if (sub == 0) a.lse[((int64_t)b * a.heads + h) * S + i] = m + __logf(l);
    }
}

// dq and delta_i = dout_i . out_i (parked for the dk / dv pass): the forward's shape
template <int EPL>
__global__ __launch_bounds__(256) void attn_causal_dq_kernel(const vtgb_attn_train_args a, const int group) {
    constexpr int W = 4 * EPL;
    __shared__ float Ks[TC_ROWS * W], Vs[TC_ROWS * W];
    const int bh = blockIdx.x, b = bh / a.heads, h = bh - b * a.heads, hd = a.head_dim, S = a.s_q;
    const int sub = threadIdx.x & 3, slot = threadIdx.x >> 2, c0 = sub * EPL;
    const int i0 = blockIdx.y * TC_ROWS, i = i0 + slot;
    const bool live = i < S;
    const float* qb = a.q + (int64_t)b * a.q_batch + h * hd;
    const float* kb = a.k + (int64_t)b * a.kv_batch + (h / group) * hd;
    const float* vb = a.v + (int64_t)b * a.kv_batch + (h / group) * hd;
    float q[EPL], go[EPL], dq[EPL];
    float dl = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; e++) {
        const bool ok = live && c0 + e < hd;
        q[e] = ok ? qb[(int64_t)i * a.q_tok + c0 + e] * a.scale : 0.f;
        go[e] = ok ? a.dout[(int64_t)b * a.o_batch + (int64_t)i * a.o_tok + h * hd + c0 + e] : 0.f;
        const float ov = ok ? a.out[(int64_t)b * a.o_batch + (int64_t)i * a.o_tok + h * hd + c0 + e] : 0.f;
        dl = fmaf(go[e], ov, dl);
        dq[e] = 0.f;
    }
    dl += __shfl_xor(dl, 1);
    dl += __shfl_xor(dl, 2);
    const float lse = live ? a.lse[((int64_t)b * a.heads + h) * S + i] : 0.f;
    if (live && sub == 0) a.delta[((int64_t)b * a.heads + h) * S + i] = dl;
    for (int j0 = 0; j0 <= i0; j0 += TC_ROWS) {
        __syncthreads();
        tc_stage_rows<EPL>(Ks, kb, a.kv_tok, j0, S, hd, 1.0f);
        tc_stage_rows<EPL>(Vs, vb, a.kv_tok, j0, S, hd, 1.0f);
        __syncthreads();
        const int nj = min(TC_ROWS, S - j0);
        for (int j = 0; j < nj; j++) {
            float s = tc_dot4<EPL>(q, Ks + j * W + c0);
            if (a.key_mask) s += a.key_mask[(int64_t)b * S + j0 + j];
            const float dpd = tc_dot4<EPL>(go, Vs + j * W + c0);
            if (j0 + j <= i) {
                const float ds = __expf(s - lse) * (dpd - dl);
#pragma unroll
                for (int e = 0; e < EPL; e++) dq[e] = fmaf(ds, Ks[j * W + c0 + e], dq[e]);
            }
        }
    }
    if (live) {
#pragma unroll
        for (int e = 0; e < EPL; e++)
            if (c0 + e < hd) a.dq[(int64_t)b * a.q_batch + (int64_t)i * a.q_tok + h * hd + c0 + e] = dq[e] * a.scale;
    }
}

// LDS: the <32> instances (head_dim 65 .. 128) hold two 64 x 128 fp32 chunks = 64 KiB (the dK / dV kernel 512 B more for lse / delta): inside
// gfx950's 160 KiB, over the 64 KiB static limit of earlier targets, and two workgroups per CU at the most.  At EPL = 32 the four lanes of a row
// read LDS 32 floats apart, i.e. the same bank: a conflict in every inner-loop read that a padded row (W + 1 ... ) would remove -- left as it
// is in train_attn.hip (correctness first); the first thing to change when these kernels are tuned.
// dk, dv: grid (batch * kv_heads, key chunks), four lanes per KEY row; for each query head of the group in head order, the (scaled) queries and
// dout of the query chunks from the workgroup's own onwards stream through LDS with the rows' lse / delta
template <int EPL>
__global__ __launch_bounds__(256) void attn_causal_dkv_kernel(const vtgb_attn_train_args a, const int group) {
    constexpr int W = 4 * EPL;
    __shared__ float Qs[TC_ROWS * W], Gs[TC_ROWS * W], Ls[TC_ROWS], Ds[TC_ROWS];
    const int kvh_n = a.heads / group;
    const int bh = blockIdx.x, b = bh / kvh_n, kvh = bh - b * kvh_n, hd = a.head_dim, S = a.s_q;
    const int sub = threadIdx.x & 3, slot = threadIdx.x >> 2, c0 = sub * EPL;
    const int j0 = blockIdx.y * TC_ROWS, j = j0 + slot;
    const bool live = j < S;
    const float* kb = a.k + (int64_t)b * a.kv_batch + kvh * hd;
    const float* vb = a.v + (int64_t)b * a.kv_batch + kvh * hd;
    float k[EPL], v[EPL], dk[EPL], dv[EPL];
#pragma unroll
    for (int e = 0; e < EPL; e++) {
        const bool ok = live && c0 + e < hd;
        k[e] = ok ? kb[(int64_t)j * a.kv_tok + c0 + e] : 0.f;
        v[e] = ok ? vb[(int64_t)j * a.kv_tok + c0 + e] : 0.f;
        dk[e] = 0.f; dv[e] = 0.f;
    }
    const float mask = (a.key_mask && live) ? a.key_mask[(int64_t)b * S + j] : 0.f;
    for (int hh = 0; hh < group; hh++) {
        const int h = kvh * group + hh;
        const float* qb = a.q + (int64_t)b * a.q_batch + h * hd;
        const float* gb = a.dout + (int64_t)b * a.o_batch + h * hd;
        for (int i0 = j0; i0 < S; i0 += TC_ROWS) {
            __syncthreads();
            tc_stage_rows<EPL>(Qs, qb, a.q_tok, i0, S, hd, a.scale);
            tc_stage_rows<EPL>(Gs, gb, a.o_tok, i0, S, hd, 1.0f);
            if (threadIdx.x < TC_ROWS) {
                const int i = i0 + threadIdx.x;
                Ls[threadIdx.x] = i < S ? a.lse[((int64_t)b * a.heads + h) * S + i] : 0.f;
                Ds[threadIdx.x] = i < S ? a.delta[((int64_t)b * a.heads + h) * S + i] : 0.f;
            }
            __syncthreads();
            const int ni = min(TC_ROWS, S - i0);
            for (int i = 0; i < ni; i++) {
                const float s = tc_dot4<EPL>(k, Qs + i * W + c0) + mask;
                const float dpd = tc_dot4<EPL>(v, Gs + i * W + c0);
                if (i0 + i >= j) {
                    const float A = __expf(s - Ls[i]), ds = A * (dpd - Ds[i]);
#pragma unroll
                    for (int e = 0; e < EPL; e++) {
                        dv[e] = fmaf(A, Gs[i * W + c0 + e], dv[e]);
                        dk[e] = fmaf(ds, Qs[i * W + c0 + e], dk[e]);      // (Qs holds q * scale)
                    }
                }
            }
        }
    }
    if (live) {
#pragma unroll
        for (int e = 0; e < EPL; e++)
            if (c0 + e < hd) {
                a.dk[(int64_t)b * a.kv_batch + (int64_t)j * a.kv_tok + kvh * hd + c0 + e] = dk[e];
                a.dv[(int64_t)b * a.kv_batch + (int64_t)j * a.kv_tok + kvh * hd + c0 + e] = dv[e];
            }
    }
}

// ============================================================================ entry points
static inline bool tl_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int rmsnorm_train_check(const vtgb_rmsnorm_train_args* a, const char* what) {
    VTGB_REQUIRE(a && a->gamma && a->rstd, VTGB_EINVAL, "%s: NULL argument", what);
    VTGB_REQUIRE(a->rows > 0 && a->D > 0, VTGB_EINVAL, "%s: bad dims rows=%d D=%d", what, a->rows, a->D);
    VTGB_REQUIRE((a->D & 3) == 0 && a->D <= 8192, VTGB_EUNSUPPORTED, "%s: D=%d (D must be a multiple of 4, at most 8192)", what, a->D);
    return VTGB_OK;
}

extern "C" int vtgb_rmsnorm_train_forward(const vtgb_rmsnorm_train_args* a, vtgb_stream_t stream) {
    VTGB_TRY(rmsnorm_train_check(a, "rmsnorm_train_forward"));
    VTGB_REQUIRE(a->x && a->y, VTGB_EINVAL, "rmsnorm_train_forward: NULL x / y");
    VTGB_REQUIRE(a->sum || !a->delta, VTGB_EINVAL, "rmsnorm_train_forward: `sum` is required with a delta");
    VTGB_REQUIRE(tl_aligned16(a->x) && tl_aligned16(a->y) && tl_aligned16(a->gamma) && tl_aligned16(a->delta) && tl_aligned16(a->sum), VTGB_EINVAL,
                 "rmsnorm_train_forward: buffers must be 16-byte aligned");
    hipLaunchKernelGGL(rmsnorm_train_fwd_kernel, dim3((a->rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, *a);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

extern "C" int vtgb_rmsnorm_train_backward(const vtgb_rmsnorm_train_args* a, vtgb_stream_t stream) {
    VTGB_TRY(rmsnorm_train_check(a, "rmsnorm_train_backward"));
    VTGB_REQUIRE(a->sum && a->dy && a->ds, VTGB_EINVAL, "rmsnorm_train_backward: NULL sum / dy / ds");
    VTGB_REQUIRE(tl_aligned16(a->sum) && tl_aligned16(a->dy) && tl_aligned16(a->ds) && tl_aligned16(a->gamma) && tl_aligned16(a->dsum), VTGB_EINVAL,
                 "rmsnorm_train_backward: buffers must be 16-byte aligned");
    hipLaunchKernelGGL(rmsnorm_train_bwd_kernel, dim3((a->rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, *a);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

extern "C" int vtgb_rope_train(const float* x, float* y, const float* cos_t, const float* sin_t, int32_t B, int32_t S, int32_t nh, int32_t nkv, int32_t hd,
                               int32_t conjugate, vtgb_stream_t stream) {
    VTGB_REQUIRE(x && y && cos_t && sin_t, VTGB_EINVAL, "rope_train: NULL operand");
    VTGB_REQUIRE(B > 0 && S > 0 && nh > 0 && nkv > 0 && hd > 0 && (hd & 1) == 0 && x != y, VTGB_EINVAL,
                 "rope_train: bad argument B=%d S=%d nh=%d nkv=%d hd=%d (hd must be even; y must not be x)", B, S, nh, nkv, hd);
    VTGB_REQUIRE(hd <= 128, VTGB_EUNSUPPORTED, "rope_train: head_dim=%d (at most 128)", hd);
    const int64_t n_pairs = (int64_t)B * S * (nh + 2 * nkv) * (hd / 2), blocks = (n_pairs + 255) / 256;
    VTGB_REQUIRE(blocks <= 0x7fffffffLL, VTGB_EUNSUPPORTED, "rope_train: %lld element pairs", (long long)n_pairs);
    hipLaunchKernelGGL(rope_train_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, y, cos_t, sin_t, n_pairs, S, nh, nkv, hd, conjugate);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

extern "C" int vtgb_swiglu_train_forward(const float* gu, float* act, int32_t M, int32_t I, vtgb_stream_t stream) {
    VTGB_REQUIRE(gu && act && M > 0 && I > 0, VTGB_EINVAL, "swiglu_train_forward: gu=%p act=%p M=%d I=%d", (const void*)gu, (void*)act, M, I);
    const int64_t n = (int64_t)M * I;
    hipLaunchKernelGGL(swiglu_train_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, gu, act, n, I);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

extern "C" int vtgb_swiglu_train_backward(const float* gu, const float* dact, float* dgu, int32_t M, int32_t I, vtgb_stream_t stream) {
    VTGB_REQUIRE(gu && dact && dgu && M > 0 && I > 0, VTGB_EINVAL, "swiglu_train_backward: gu=%p dact=%p dgu=%p M=%d I=%d", (const void*)gu,
                 (const void*)dact, (void*)dgu, M, I);
    const int64_t n = (int64_t)M * I;
    hipLaunchKernelGGL(swiglu_train_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, gu, dact, dgu, n, I);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

static int attn_causal_check(const vtgb_attn_train_args* a, int kv_heads, bool bwd) {
    VTGB_REQUIRE(a, VTGB_EINVAL, "attn_train_causal: NULL args");
    VTGB_REQUIRE(a->batch > 0 && a->heads > 0 && kv_heads > 0 && a->head_dim > 0 && a->s_q > 0 && a->s_kv > 0, VTGB_EINVAL,
                 "attn_train_causal: bad dims B=%d H=%d KVH=%d hd=%d Sq=%d Skv=%d", a->batch, a->heads, kv_heads, a->head_dim, a->s_q, a->s_kv);
    VTGB_REQUIRE(a->s_q == a->s_kv, VTGB_EINVAL, "attn_train_causal: s_q=%d and s_kv=%d differ (self-attention only)", a->s_q, a->s_kv);
    VTGB_REQUIRE(a->heads % kv_heads == 0, VTGB_EINVAL, "attn_train_causal: heads=%d is no multiple of kv_heads=%d", a->heads, kv_heads);
    VTGB_REQUIRE(!a->drop, VTGB_EINVAL, "attn_train_causal: a dropout mask (drop must be NULL)");
    VTGB_REQUIRE(a->head_dim <= 128, VTGB_EUNSUPPORTED, "attn_train_causal: head_dim=%d (at most 128)", a->head_dim);
    VTGB_REQUIRE((int64_t)a->batch * a->heads <= 0x7fffffffLL && (a->s_q + TC_ROWS - 1) / TC_ROWS <= 65535, VTGB_EUNSUPPORTED,
                 "attn_train_causal: B=%d H=%d S=%d exceed the launch grid", a->batch, a->heads, a->s_q);
    VTGB_REQUIRE(a->q && a->k && a->v && a->out && a->lse, VTGB_EINVAL, "attn_train_causal: NULL operand");
    if (bwd) VTGB_REQUIRE(a->dout && a->dq && a->dk && a->dv && a->delta, VTGB_EINVAL, "attn_train_causal backward: NULL gradient operand");
    return VTGB_OK;
}

#define TC_DISPATCH(KERNEL, BH)                                                                                  \
    do {                                                                                                         \
        const dim3 grid((unsigned)(BH), (unsigned)((a->s_q + TC_ROWS - 1) / TC_ROWS));                           \
        if (a->head_dim <= 32) hipLaunchKernelGGL(KERNEL<8>, grid, dim3(256), 0, s, *a, group);                  \
        else if (a->head_dim <= 64) hipLaunchKernelGGL(KERNEL<16>, grid, dim3(256), 0, s, *a, group);            \
        else hipLaunchKernelGGL(KERNEL<32>, grid, dim3(256), 0, s, *a, group);                                   \
        VTGB_HIP(hipGetLastError());                                                                             \
    } while (0)

extern "C" int vtgb_attn_train_causal_forward(const vtgb_attn_train_args* a, int32_t kv_heads, vtgb_stream_t stream) {
    VTGB_TRY(attn_causal_check(a, kv_heads, false));
    hipStream_t s = (hipStream_t)stream;
    const int group = a->heads / kv_heads;
    TC_DISPATCH(attn_causal_fwd_kernel, a->batch * a->heads);
    return VTGB_OK;
}

extern "C" int vtgb_attn_train_causal_backward(const vtgb_attn_train_args* a, int32_t kv_heads, vtgb_stream_t stream) {
    VTGB_TRY(attn_causal_check(a, kv_heads, true));
    hipStream_t s = (hipStream_t)stream;
    const int group = a->heads / kv_heads;
    TC_DISPATCH(attn_causal_dq_kernel, a->batch * a->heads);       // also writes delta
    TC_DISPATCH(attn_causal_dkv_kernel, a->batch * kv_heads);
    return VTGB_OK;
}
