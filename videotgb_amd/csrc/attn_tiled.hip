// attn_tiled.hip -- causal softmax(scale * Q K^T + key_mask) V for the language model's prefill on gfx950: any prompt length up to
// 4096 keys and grouped-query heads, bf16 in / out, fp32 scores, softmax statistics and output accumulator.
//
// attn.hip keeps the whole K and V of one (batch, head) in LDS, which ends at 288 keys of head_dim 128.  Here K and V pass through
// LDS in tiles of KT = 64 keys and the softmax is the online one (running maximum m and sum l per query, accumulator rescaled by
// exp(m_old - m_new) once per key tile).
//
// Work split.  A workgroup is 4 waves; a wave owns one 16-query tile of one query head for the whole key walk (its Q fragments, m, l
// and the O^T accumulator stay in registers).  The 4 wave slots of a workgroup are HG query heads of ONE K/V head x 4 / HG consecutive
// 16-query tiles, HG = the largest of {4, 2, 1} that divides heads / kv_heads: the query heads of a group share every staged K/V tile,
// K/V are read in place (head h reads K/V head h / (heads / kv_heads)), nothing is replicated.  What a wave computes for its 16 queries
// does not depend on which other waves share its workgroup, so grouped heads give the bits that replicated K/V give.
// Causal: a workgroup walks key tiles 0 .. the tile of its last query's diagonal, a wave stops computing after its own diagonal tile
// (it still stages and meets the barriers), so the matrix work is the triangle's.  Workgroups are issued longest walk first.
// No atomics, no split of a query's keys over workgroups, a fixed tile order: a row's result depends on that row alone.
//
// Staging.  Tile t + 1 is loaded global -> registers before tile t's MFMAs and written to the other LDS buffer after them (the
// load-everything-then-write form of attn.hip's staging, one tile ahead): one barrier per tile, the HBM / L2 latency sits behind the
// matrix work.  LDS images are attn.hip's: K [key][d] in 256-byte rows with the 16-byte piece XOR-swizzled by the row (head_dim 128)
// or rows padded by 16 bytes (64); V row-major [key][d], rows padded by 32 bytes, read transposed with ds_read_b64_tr_b16.
// LDS: 2 x (64 x 256 + 64 x 288 + 64 x 4) = 70 144 bytes at head_dim 128, 39 424 at 64: two workgroups per CU.
//
// Products, transposed as in attn.hip so that P never passes through LDS (v_mfma_f32_16x16x32_bf16):
//   S^T[key][q] = K (A: LDS) x Q^T (B: registers, loaded once);   O^T[d][q] = V^T (A: LDS, transposing read) x P^T (B: the S^T accumulators,
//   exponentiated and packed to bf16 -- rounded once, as in attn.hip; the sum l adds the unrounded fp32 values, as there).
//
// Key mask (additive fp32 [batch, s_kv]): a value <= finfo(float32).min is a HARD mask -- the key's score is -inf (weight exactly 0)
// and its K and V rows are not loaded (the LDS rows are zeros), so whatever a pad slot holds, NaN included, cannot reach an output.
// Any other value is added to the scaled score.  A query without any visible key gets an all-zero output row.
#include "common.h"

#include <float.h>
#include <math.h>

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4_t;

constexpr int TILED_MAX_KV = 4096;

template <int HD>
struct TiledCfg {
    static constexpr int KT = 64;                   // keys per tile
    static constexpr bool KSWZ = HD > 64;           // (AttnCfg's K image: see attn.hip)
    static constexpr int KS = KSWZ ? 256 : HD * 2 + 16;
    static __device__ __forceinline__ int koff(int row, int piece) { return row * KS + ((KSWZ ? (piece ^ (row & 15)) : piece) << 4); }
    static constexpr int VS = HD * 2 + 32;
    static constexpr int K_BYTES = KT * KS;
    static constexpr int V_BYTES = KT * VS;
    static constexpr int BUF = K_BYTES + V_BYTES + KT * 4;      // K | V | the tile's mask row
    static constexpr int LDS = 2 * BUF;
};

template <int HD, int HG, bool MASKED>
__global__ __launch_bounds__(256, 2) void attn_tiled_kernel(const vtgb_attention_tiled_args p) {
    using C = TiledCfg<HD>;
    constexpr int KT = C::KT, CH = HD / 8, KI = KT * CH / 256, QW = 4 / HG;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fg = lane >> 4;
    const int qblk = gridDim.x - 1 - blockIdx.x;                 // longest key walk first
    const int b = blockIdx.z;
    const int head = blockIdx.y * HG + (wave % HG);
    const int kvh = (blockIdx.y * HG) / (p.heads / p.kv_heads);  // HG divides heads / kv_heads: one K/V head per workgroup
    const int qt = qblk * QW + wave / HG;
    const int off = p.s_kv - p.s_q;
    const bf16_t* __restrict__ Q = reinterpret_cast<const bf16_t*>(p.q) + (int64_t)b * p.q_batch_stride + head * HD;
    const bf16_t* __restrict__ K = reinterpret_cast<const bf16_t*>(p.k) + (int64_t)b * p.kv_batch_stride + kvh * HD;
    const bf16_t* __restrict__ V = reinterpret_cast<const bf16_t*>(p.v) + (int64_t)b * p.kv_batch_stride + kvh * HD;
    bf16_t* __restrict__ O = reinterpret_cast<bf16_t*>(p.out) + (int64_t)b * p.out_batch_stride + head * HD;
    const float* __restrict__ mask = MASKED ? p.key_mask + (int64_t)b * p.s_kv : nullptr;
    const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

    // key tiles of the workgroup / of this wave: up to the diagonal of the last query (causal), all of them otherwise
    const int nkt_all = (p.s_kv + KT - 1) / KT;
    int nkt_blk = nkt_all, nkt_w = qt * 16 < p.s_q ? nkt_all : 0;
    if (p.causal) {
        const int qb = min(p.s_q, (qblk + 1) * QW * 16) - 1 + off, qw = min(p.s_q, qt * 16 + 16) - 1 + off;
        nkt_blk = min(nkt_all, qb >= 0 ? qb / KT + 1 : 0);
        nkt_w = min(nkt_w, qw >= 0 ? qw / KT + 1 : 0);
    }

    const int q = qt * 16 + fr;
    const bool qvalid = q < p.s_q;
    bf16x8 qf[HD / 32];
#pragma unroll
    for (int ks = 0; ks < HD / 32; ks++)
        qf[ks] = qvalid ? *reinterpret_cast<const bf16x8*>(Q + (int64_t)q * p.q_tok_stride + (ks * 4 + fg) * 8) : zero8;
    const int klim = p.causal ? q + off : 0x7fffffff;           // query q sees keys <= q + (s_kv - s_q)

    bf16x8 kreg[KI], vreg[KI];
    float mreg = 0.f;
    // tile t: global -> registers.  A key past s_kv or hard-masked is not loaded: its rows are zeros, its mask entry -inf.
    auto load_tile = [&](int t) {
#pragma unroll
        for (int i = 0; i < KI; i++) {
            const int idx = tid + i * 256, key = t * KT + idx / CH, c = idx % CH;
            bool ok = key < p.s_kv;
            if (MASKED && ok) ok = mask[key] > -FLT_MAX;
            kreg[i] = zero8; vreg[i] = zero8;
            if (ok) {
                kreg[i] = *reinterpret_cast<const bf16x8*>(K + (int64_t)key * p.kv_tok_stride + c * 8);
                vreg[i] = *reinterpret_cast<const bf16x8*>(V + (int64_t)key * p.kv_tok_stride + c * 8);
            }
        }
        if (tid < KT) {
            const int key = t * KT + tid;
            float m = -INFINITY;
            if (key < p.s_kv) {
                m = 0.f;
                if (MASKED) {
                    m = mask[key];
                    if (!(m > -FLT_MAX)) m = -INFINITY;
                }
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
            *reinterpret_cast<bf16x8*>(Ks + C::koff(key, c)) = kreg[i];
            *reinterpret_cast<bf16x8*>(Vs + key * C::VS + c * 16) = vreg[i];
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

template <int HD, int HG, bool MASKED>
static int launch_tiled_v(const vtgb_attention_tiled_args& a, hipStream_t s) {
    using C = TiledCfg<HD>;
    static DeviceOnce attr_set;
    VTGB_FUNC_LDS_ONCE(attr_set, (attn_tiled_kernel<HD, HG, MASKED>), C::LDS);
    const int q_per_block = 64 / HG;
    const dim3 grid((a.s_q + q_per_block - 1) / q_per_block, a.heads / HG, a.batch);
    const double pairs = a.causal ? (double)a.s_q * (a.s_kv - a.s_q + 0.5 * (a.s_q + 1)) : (double)a.s_q * a.s_kv;
    ProfScope prof(VTGB_PROF_ATTN, 4.0 * a.batch * a.heads * pairs * a.head_dim, s);
    hipLaunchKernelGGL((attn_tiled_kernel<HD, HG, MASKED>), grid, dim3(256), C::LDS, s, a);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

template <int HD, int HG>
static int launch_tiled_m(const vtgb_attention_tiled_args& a, hipStream_t s) {
    return a.key_mask ? launch_tiled_v<HD, HG, true>(a, s) : launch_tiled_v<HD, HG, false>(a, s);
}

template <int HD>
static int launch_tiled(const vtgb_attention_tiled_args& a, hipStream_t s) {
    const int group = a.heads / a.kv_heads;
    if (group % 4 == 0) return launch_tiled_m<HD, 4>(a, s);
    if (group % 2 == 0) return launch_tiled_m<HD, 2>(a, s);
    return launch_tiled_m<HD, 1>(a, s);
}

extern "C" int vtgb_attention_tiled(const vtgb_attention_tiled_args* a, vtgb_stream_t stream) {
    VTGB_REQUIRE(a, VTGB_EINVAL, "attention tiled: NULL args");
    VTGB_REQUIRE(a->q && a->k && a->v && a->out, VTGB_EINVAL, "attention tiled: NULL operand");
    VTGB_REQUIRE(a->batch > 0 && a->heads > 0 && a->kv_heads > 0 && a->s_q > 0 && a->s_kv > 0, VTGB_EINVAL, "attention tiled: empty problem");
    VTGB_REQUIRE(a->heads % a->kv_heads == 0, VTGB_EINVAL, "attention tiled: heads=%d is not a multiple of kv_heads=%d", a->heads, a->kv_heads);
    VTGB_REQUIRE(a->head_dim == 64 || a->head_dim == 128, VTGB_EUNSUPPORTED, "attention tiled: head_dim=%d, built for 64 and 128", a->head_dim);
    VTGB_REQUIRE(a->s_kv <= TILED_MAX_KV, VTGB_EUNSUPPORTED, "attention tiled: s_kv=%d exceeds %d keys", a->s_kv, TILED_MAX_KV);
    VTGB_REQUIRE(a->batch <= 65535 && a->heads <= 65535, VTGB_EUNSUPPORTED, "attention tiled: batch=%d / heads=%d exceed the grid", a->batch, a->heads);
    VTGB_REQUIRE((a->q_tok_stride % 8) == 0 && (a->kv_tok_stride % 8) == 0 && (a->out_tok_stride % 4) == 0 && (a->q_batch_stride % 8) == 0 &&
                     (a->kv_batch_stride % 8) == 0 && (a->out_batch_stride % 4) == 0,
                 VTGB_EUNSUPPORTED, "attention tiled: strides must keep 16-byte alignment");
    const auto misaligned = [](const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) != 0; };
    VTGB_REQUIRE(!misaligned(a->q, 16) && !misaligned(a->k, 16) && !misaligned(a->v, 16) && !misaligned(a->out, 8) && !misaligned(a->key_mask, 4),
                 VTGB_EUNSUPPORTED, "attention tiled: q / k / v need 16-byte, out 8-byte, key_mask 4-byte alignment");
    return a->head_dim == 128 ? launch_tiled<128>(*a, stream) : launch_tiled<64>(*a, stream);
}
