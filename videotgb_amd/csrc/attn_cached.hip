// attn_cached.hip -- causal softmax(scale * Q K^T) V of a CHUNK of queries over the language model's KV cache on gfx950: the chunked
// prefill's attention (prompts past the one-shot prefill's 2048 tokens).  Queries q [batch, s_q, heads * hd] bf16 are the prompt positions
// q0 .. q0 + s_q - 1; K and V are the decoder's caches [batch, kv_heads, tmax, hd] -- bf16, or e4m3 codes with one fp32 power-of-two scale
// per row ([batch, kv_heads, tmax]: vtgb_llm_decode_attention_split_fp8's layout) -- up to 16384 slots.  Query i sees cache rows
// 0 .. q0 + i; nothing at or past row q0 + s_q is read.
//
// This is attn_tiled.hip's kernel with another global side: the same 64-key tiles from key 0 upward, one wave per 16-query tile per query
// head, HG query heads of one K/V head per workgroup, the same transposed MFMA products, online-softmax update, single rounding of P, LDS
// images and one-tile-ahead staging (see that file for all of them).  What differs:
//   - a cache row is hd contiguous values of one K/V head (tile loads are 64 contiguous rows, not rows strided by the token);
//   - fp8 rows travel global -> registers as codes (8 bytes per thread and piece) with their row scale, and are widened (kv8_widen4) and
//     multiplied by the scale on the way registers -> LDS, after the tile's MFMAs: code * scale is exactly a bf16 number, so the LDS image is
//     the bf16 cache's, bit for bit;
//   - the causal offset is q0 (the tiled kernel's s_kv - s_q with s_kv = q0 + s_q);
//   - the key mask is key_valid [batch, tmax] uint8 (the decode kernels' convention): a key with 0 gets score -inf (weight exactly 0) and
//     neither its K / V row nor its codes or scales are loaded (the LDS rows are zeros), so a pad slot may hold NaN.
// Hence the output equals vtgb_attention_tiled's with s_kv = q0 + s_q on the same K / V values token-major (key_valid 0 <-> a hard
// key_mask), bit for bit, wherever that kernel takes the call.  A query with no visible key gets an all-zero row.  A row's result depends
// on that row alone: no atomics, no split of a query's keys over workgroups, a fixed tile order.
#include "common.h"
#include "fp8_code.h"

#include <math.h>

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4_t;

constexpr int CACHED_MAX_T = 16384;

template <int HD>
struct CachedCfg {      // (TiledCfg of attn_tiled.hip: the same LDS images)
    static constexpr int KT = 64;                   // keys per tile
    static constexpr bool KSWZ = HD > 64;
    static constexpr int KS = KSWZ ? 256 : HD * 2 + 16;
    static __device__ __forceinline__ int koff(int row, int piece) { return row * KS + ((KSWZ ? (piece ^ (row & 15)) : piece) << 4); }
    static constexpr int VS = HD * 2 + 32;
    static constexpr int K_BYTES = KT * KS;
    static constexpr int V_BYTES = KT * VS;
    static constexpr int BUF = K_BYTES + V_BYTES + KT * 4;      // K | V | the tile's mask row
    static constexpr int LDS = 2 * BUF;
};

// 8 codes (two dwords) x the row's scale -> 8 bf16, exact
__device__ __forceinline__ bf16x8 kv8_row_piece(uint2 w, float sc) {
    float lo[4], hi[4];
    kv8_widen4(w.x, lo);
    kv8_widen4(w.y, hi);
    return bf16x8{(bf16_t)(lo[0] * sc), (bf16_t)(lo[1] * sc), (bf16_t)(lo[2] * sc), (bf16_t)(lo[3] * sc),
                  (bf16_t)(hi[0] * sc), (bf16_t)(hi[1] * sc), (bf16_t)(hi[2] * sc), (bf16_t)(hi[3] * sc)};
}

template <int HD, int HG, bool MASKED, bool FP8>
__global__ __launch_bounds__(256, 2) void attn_cached_kernel(const vtgb_attention_cached_args p) {
    using C = CachedCfg<HD>;
    constexpr int KT = C::KT, CH = HD / 8, KI = KT * CH / 256, QW = 4 / HG;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fg = lane >> 4;
    const int qblk = gridDim.x - 1 - blockIdx.x;                 // longest key walk first
    const int b = blockIdx.z;
    const int head = blockIdx.y * HG + (wave % HG);
    const int kvh = (blockIdx.y * HG) / (p.heads / p.kv_heads);  // HG divides heads / kv_heads: one K/V head per workgroup
    const int qt = qblk * QW + wave / HG;
    const int off = p.q0, s_kv = p.q0 + p.s_q;
    const int64_t crow0 = ((int64_t)b * p.kv_heads + kvh) * p.tmax;      // the (batch, K/V head)'s first cache row
    const bf16_t* __restrict__ Q = reinterpret_cast<const bf16_t*>(p.q) + (int64_t)b * p.q_batch_stride + head * HD;
    const bf16_t* __restrict__ K = reinterpret_cast<const bf16_t*>(p.kc) + crow0 * HD;      // (!FP8)
    const bf16_t* __restrict__ V = reinterpret_cast<const bf16_t*>(p.vc) + crow0 * HD;
    const uint8_t* __restrict__ K8 = reinterpret_cast<const uint8_t*>(p.kc) + crow0 * HD;   // (FP8)
    const uint8_t* __restrict__ V8 = reinterpret_cast<const uint8_t*>(p.vc) + crow0 * HD;
    const float* __restrict__ KSc = FP8 ? p.ks + crow0 : nullptr;
    const float* __restrict__ VSc = FP8 ? p.vs + crow0 : nullptr;
    bf16_t* __restrict__ O = reinterpret_cast<bf16_t*>(p.out) + (int64_t)b * p.out_batch_stride + head * HD;
    const uint8_t* __restrict__ valid = MASKED ? p.key_valid + (int64_t)b * p.tmax : nullptr;
    const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

    // key tiles of the workgroup / of this wave: up to the diagonal of the last query
    const int nkt_all = (s_kv + KT - 1) / KT;
    const int qb = min(p.s_q, (qblk + 1) * QW * 16) - 1 + off, qw = min(p.s_q, qt * 16 + 16) - 1 + off;
    const int nkt_blk = min(nkt_all, qb / KT + 1);
    const int nkt_w = qt * 16 < p.s_q ? min(nkt_all, qw / KT + 1) : 0;

    const int q = qt * 16 + fr;
    const bool qvalid = q < p.s_q;
    bf16x8 qf[HD / 32];
#pragma unroll
    for (int ks = 0; ks < HD / 32; ks++)
        qf[ks] = qvalid ? *reinterpret_cast<const bf16x8*>(Q + (int64_t)q * p.q_tok_stride + (ks * 4 + fg) * 8) : zero8;
    const int klim = q + off;                                   // query q sees cache rows <= q0 + q

    // the tile in flight: bf16 pieces, or (FP8) the pieces' codes and their rows' scales
    bf16x8 kreg[FP8 ? 1 : KI], vreg[FP8 ? 1 : KI];
    uint2 kraw[FP8 ? KI : 1], vraw[FP8 ? KI : 1];
    float kscl[FP8 ? KI : 1], vscl[FP8 ? KI : 1];
    float mreg = 0.f;
    // tile t: global -> registers.  A key past the chunk's end or masked is not loaded: its rows are zeros, its mask entry -inf.
    auto load_tile = [&](int t) {
#pragma unroll
        for (int i = 0; i < KI; i++) {
            const int idx = tid + i * 256, key = t * KT + idx / CH, c = idx % CH;
            bool ok = key < s_kv;
            if (MASKED && ok) ok = valid[key] != 0;
            if constexpr (FP8) {
                kraw[i] = uint2{0u, 0u}; vraw[i] = uint2{0u, 0u};      // (code 0 is +0)
                kscl[i] = 0.f; vscl[i] = 0.f;
                if (ok) {
                    kraw[i] = *reinterpret_cast<const uint2*>(K8 + (int64_t)key * HD + c * 8);
                    vraw[i] = *reinterpret_cast<const uint2*>(V8 + (int64_t)key * HD + c * 8);
                    kscl[i] = KSc[key];
                    vscl[i] = VSc[key];
                }
            } else {
                kreg[i] = zero8; vreg[i] = zero8;
                if (ok) {
                    kreg[i] = *reinterpret_cast<const bf16x8*>(K + (int64_t)key * HD + c * 8);
                    vreg[i] = *reinterpret_cast<const bf16x8*>(V + (int64_t)key * HD + c * 8);
                }
            }
        }
        if (tid < KT) {
            const int key = t * KT + tid;
            float m = -INFINITY;
            if (key < s_kv) {
                m = 0.f;
                if (MASKED && valid[key] == 0) m = -INFINITY;
            }
            mreg = m;
        }
    };
    auto store_tile = [&](int buf) {
        char* Ks = smem + buf * C::BUF;
        char* Vs = Ks + C::K_BYTES;
#pragma unroll
        for (int i = 0; i < KI; i++) {
            const int idx = tid + i * 256, key = idx / CH, c = idx % CH;
            if constexpr (FP8) {
                *reinterpret_cast<bf16x8*>(Ks + C::koff(key, c)) = kv8_row_piece(kraw[i], kscl[i]);
                *reinterpret_cast<bf16x8*>(Vs + key * C::VS + c * 16) = kv8_row_piece(vraw[i], vscl[i]);
            } else {
                *reinterpret_cast<bf16x8*>(Ks + C::koff(key, c)) = kreg[i];
                *reinterpret_cast<bf16x8*>(Vs + key * C::VS + c * 16) = vreg[i];
            }
        }
        if (tid < KT) reinterpret_cast<float*>(Vs + C::V_BYTES)[tid] = mreg;
    };

    float m_run = -INFINITY, l_run = 0.f;      // l_run: this lane's share (its 4 key rows of every 16); the lane groups are added at the end
    f32x4 o[HD / 16];
#pragma unroll
    for (int dt = 0; dt < HD / 16; dt++) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

    if (nkt_blk > 0) {
        load_tile(0);
        store_tile(0);
    }
    __syncthreads();
    for (int t = 0; t < nkt_blk; t++) {
        if (t + 1 < nkt_blk) load_tile(t + 1);
        if (t < nkt_w) {
            const char* Ks = smem + (t & 1) * C::BUF;
            const char* Vs = Ks + C::K_BYTES;
            const float* maskv = reinterpret_cast<const float*>(Vs + C::V_BYTES);
            // ---- S^T: four 16-key tiles
            f32x4 s[4];
#pragma unroll
            for (int tt = 0; tt < 4; tt++) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < HD / 32; ks++) {
                    const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Ks + C::koff(tt * 16 + fr, ks * 4 + fg));
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], acc, 0, 0, 0);
                }
                s[tt] = acc;
            }
            // ---- online softmax: registers (tt, r) x lane groups fg hold the 64 keys of query column fr
            float mt = -INFINITY;
#pragma unroll
            for (int tt = 0; tt < 4; tt++) {
                const float4 mk = *reinterpret_cast<const float4*>(maskv + tt * 16 + fg * 4);
                const int k0 = t * KT + tt * 16 + fg * 4;
                s[tt][0] = k0 <= klim ? s[tt][0] * p.scale + mk.x : -INFINITY;
                s[tt][1] = k0 + 1 <= klim ? s[tt][1] * p.scale + mk.y : -INFINITY;
                s[tt][2] = k0 + 2 <= klim ? s[tt][2] * p.scale + mk.z : -INFINITY;
                s[tt][3] = k0 + 3 <= klim ? s[tt][3] * p.scale + mk.w : -INFINITY;
                mt = fmaxf(mt, fmaxf(fmaxf(s[tt][0], s[tt][1]), fmaxf(s[tt][2], s[tt][3])));
            }
            mt = fmaxf(mt, __shfl_xor(mt, 16));
            mt = fmaxf(mt, __shfl_xor(mt, 32));
            const float m_new = fmaxf(m_run, mt);
            const float m_use = m_new == -INFINITY ? 0.f : m_new;      // no visible key so far: every exponential below is exp(-inf) = 0
            const float alpha = __expf(m_run - m_use);
            m_run = m_new;
            float ps = 0.f;
#pragma unroll
            for (int tt = 0; tt < 4; tt++) {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float e = __expf(s[tt][r] - m_use);
                    s[tt][r] = e;
                    ps += e;
                }
            }
            l_run = l_run * alpha + ps;
#pragma unroll
            for (int dt = 0; dt < HD / 16; dt++) o[dt] *= alpha;
            // ---- O^T += V^T P^T, one 32-key pair per step (fragment addressing: attn.hip)
            const char* const vbase = Vs + (fg * 4 + (fr >> 2)) * C::VS + (fr & 3) * 8;
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const bf16x8 pf = {(bf16_t)s[2 * u][0],     (bf16_t)s[2 * u][1],     (bf16_t)s[2 * u][2],     (bf16_t)s[2 * u][3],
                                   (bf16_t)s[2 * u + 1][0], (bf16_t)s[2 * u + 1][1], (bf16_t)s[2 * u + 1][2], (bf16_t)s[2 * u + 1][3]};
#pragma unroll
                for (int dt = 0; dt < HD / 16; dt++) {
                    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_t*)(vbase + (u * 32) * C::VS + dt * 32));
                    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_t*)(vbase + (u * 32 + 16) * C::VS + dt * 32));
                    const bf16x8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[dt], 0, 0, 0);
                }
            }
        }
        if (t + 1 < nkt_blk) store_tile((t + 1) & 1);
        __syncthreads();
    }

    l_run += __shfl_xor(l_run, 16);
    l_run += __shfl_xor(l_run, 32);
    const float inv = l_run > 0.f ? 1.0f / l_run : 0.f;
    if (qvalid) {
#pragma unroll
        for (int dt = 0; dt < HD / 16; dt++) {
            const int d = dt * 16 + fg * 4;
            const bf16x4 pk = {(bf16_t)(o[dt][0] * inv), (bf16_t)(o[dt][1] * inv), (bf16_t)(o[dt][2] * inv), (bf16_t)(o[dt][3] * inv)};
            *reinterpret_cast<bf16x4*>(O + (int64_t)q * p.out_tok_stride + d) = pk;
        }
    }
}

template <int HD, int HG, bool MASKED, bool FP8>
static int launch_cached_v(const vtgb_attention_cached_args& a, hipStream_t s) {
    using C = CachedCfg<HD>;
    static DeviceOnce attr_set;
    VTGB_FUNC_LDS_ONCE(attr_set, (attn_cached_kernel<HD, HG, MASKED, FP8>), C::LDS);
    const int q_per_block = 64 / HG;
    const dim3 grid((a.s_q + q_per_block - 1) / q_per_block, a.heads / HG, a.batch);
    const double pairs = (double)a.s_q * (a.q0 + 0.5 * (a.s_q + 1));
    ProfScope prof(VTGB_PROF_ATTN, 4.0 * a.batch * a.heads * pairs * a.head_dim, s);
    hipLaunchKernelGGL((attn_cached_kernel<HD, HG, MASKED, FP8>), grid, dim3(256), C::LDS, s, a);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

template <int HD, int HG>
static int launch_cached_m(const vtgb_attention_cached_args& a, hipStream_t s) {
    if (a.ks) return a.key_valid ? launch_cached_v<HD, HG, true, true>(a, s) : launch_cached_v<HD, HG, false, true>(a, s);
    return a.key_valid ? launch_cached_v<HD, HG, true, false>(a, s) : launch_cached_v<HD, HG, false, false>(a, s);
}

template <int HD>
static int launch_cached(const vtgb_attention_cached_args& a, hipStream_t s) {
    const int group = a.heads / a.kv_heads;
    if (group % 4 == 0) return launch_cached_m<HD, 4>(a, s);
    if (group % 2 == 0) return launch_cached_m<HD, 2>(a, s);
    return launch_cached_m<HD, 1>(a, s);
}

extern "C" int vtgb_attention_cached(const vtgb_attention_cached_args* a, vtgb_stream_t stream) {
    VTGB_REQUIRE(a, VTGB_EINVAL, "attention cached: NULL args");
    VTGB_REQUIRE(a->q && a->kc && a->vc && a->out, VTGB_EINVAL, "attention cached: NULL operand");
    VTGB_REQUIRE(a->batch > 0 && a->heads > 0 && a->kv_heads > 0 && a->s_q > 0 && a->tmax > 0, VTGB_EINVAL, "attention cached: empty problem");
    VTGB_REQUIRE(a->q0 >= 0, VTGB_EINVAL, "attention cached: negative q0=%d", a->q0);
    VTGB_REQUIRE(a->heads % a->kv_heads == 0, VTGB_EINVAL, "attention cached: heads=%d is not a multiple of kv_heads=%d", a->heads, a->kv_heads);
    VTGB_REQUIRE((a->ks != nullptr) == (a->vs != nullptr), VTGB_EINVAL, "attention cached: ks and vs come together (fp8 codes) or not at all (bf16)");
    VTGB_REQUIRE(a->head_dim == 64 || a->head_dim == 128, VTGB_EUNSUPPORTED, "attention cached: head_dim=%d, built for 64 and 128", a->head_dim);
    VTGB_REQUIRE(a->tmax <= CACHED_MAX_T, VTGB_EUNSUPPORTED, "attention cached: tmax=%d exceeds %d slots", a->tmax, CACHED_MAX_T);
    VTGB_REQUIRE((int64_t)a->q0 + a->s_q <= a->tmax, VTGB_EUNSUPPORTED, "attention cached: q0=%d + s_q=%d exceed the cache, tmax=%d", a->q0, a->s_q, a->tmax);
    VTGB_REQUIRE(a->batch <= 65535 && a->heads <= 65535, VTGB_EUNSUPPORTED, "attention cached: batch=%d / heads=%d exceed the grid", a->batch, a->heads);
    VTGB_REQUIRE((a->q_tok_stride % 8) == 0 && (a->out_tok_stride % 4) == 0 && (a->q_batch_stride % 8) == 0 && (a->out_batch_stride % 4) == 0,
                 VTGB_EUNSUPPORTED, "attention cached: strides must keep 16-byte alignment");
    const auto misaligned = [](const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) != 0; };
    VTGB_REQUIRE(!misaligned(a->q, 16) && !misaligned(a->kc, 16) && !misaligned(a->vc, 16) && !misaligned(a->out, 8) && !misaligned(a->ks, 4) &&
                     !misaligned(a->vs, 4),
                 VTGB_EUNSUPPORTED, "attention cached: q / kc / vc need 16-byte, out 8-byte, ks / vs 4-byte alignment");
    return a->head_dim == 128 ? launch_cached<128>(*a, stream) : launch_cached<64>(*a, stream);
}
