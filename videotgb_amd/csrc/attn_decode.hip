// attn_decode.hip -- split-KV ("flash-decoding") single-query attention over the static K/V cache of the decode step, for caches the
// one-wave-per-head kernel of llm.hip cannot hold (its scores live in LDS: 2048 keys) or serves badly (8 workgroups at batch 1).
// Two launches, no atomics.  Pass 1 is written once (decode_attn_pass1) and reads its keys through a key source; four entries, one source each:
//   vtgb_llm_decode_attention_split      DenseKV   one cache kc / vc [B, nkv, tmax, hd] of bf16 or fp32
//   vtgb_llm_decode_attention_split_fp8  Fp8KV     e4m3 codes and one power-of-two scale per row (kv_cache="fp8")
//   vtgb_llm_decode_attention_beam       BeamKV    a prompt cache per batch item + a generated cache read through src_row (beam_search="graph")
//   vtgb_llm_decode_attention_beam_fp8   BeamFp8KV BeamKV's two caches and table over Fp8KV's codes and scales (beam_search="graph+kv8")
// The later three compute, bit for bit, what the first computes on the cache they stand for (see the sources below).
//
// Pass 1.  Grid (key chunk, K/V head x query-head block, row), fixed by tmax, so one captured graph serves every step: a workgroup whose
// chunk starts past *pos leaves after reading *pos.  A chunk is DEC_SPLIT_CHUNK = 256 keys, 64 per wave.  A wave holds its 64 K rows in
// registers -- one load per lane and row, consecutive lanes on consecutive pieces of EPL elements of a row, so one load instruction reads
// 64 / LPR whole rows (LPR = lanes per row = hd / EPL) -- and every query head of the block (at most DEC_SPLIT_HEADS = 8 heads of ONE K/V
// head; a larger nq / nkv takes more blocks) takes its scores from those registers; the V rows then replace them and serve every head
// again.  K/V are read once per group of query heads, in place.
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
// inside every sum depend on the key index, EPL and hd alone -- not on the rows, tmax, the grid, the number of query heads per K/V head,
// which heads share a workgroup (a head's arithmetic never sees another head's values) or the key source.  An invisible key adds an exact
// +0.  So a row's output is a function of (q, K/V[0..*pos], key_valid[0..*pos]): the same bits in any batch, any cache length, grouped or
// replicated K/V, and from any source that presents the same K/V values.
#include "common.h"
#include "fp8_code.h"

#include <math.h>

#include <initializer_list>

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

// ---- key sources.  A source supplies what differs between the entries and no arithmetic of the attention itself:
//   HD, EPL, Reg       head_dim; elements per lane and row; the register that holds them
//   SCALED             whether a row carries scales (scales() below)
//   walk_pos, pos      the clamped positions: pass 2 walks the chunks 0 .. walk_pos / 256, the last visible key is pos <= walk_pos
//   seat<MASKED>(r, kvh, c)   this workgroup's row and K/V head, this lane's piece of a row (called once, before any load: BeamFp8KV starts its scale loads here)
//   visible<MASKED>(key)
//   row(key, ok)       where the key's row lies (Row; ok = visible): an invisible key gets a safe in-bounds row, one for the whole grid
//   k(), v()           the K and the V cache (Cache), handed to load()
//   zero()             a register of zeros
//   load(cache, row, key, ok, zero)   the lane's piece of the row, selected to ``zero`` for an invisible key, so nothing a pad slot holds
//                      reaches a product
//   widen(reg, f)      the piece as fp32, exact
//   scales(key, ok, sk, sv)   SCALED only: the row's K and V scale, read from the safe row and selected to 1 for an invisible key

// One cache of T, kc / vc [B, nkv, tmax, hd]: 16-byte pieces.  OneCacheKeys is what it shares with the fp8 cache.
struct OneCacheKeys {
    const uint8_t* kvr;      // key_valid of the row (MASKED)
    int pos, walk_pos;
    __device__ __forceinline__ OneCacheKeys(const int64_t* pos_p, int tmax) : kvr(nullptr), pos(min((int)(*pos_p), tmax - 1)), walk_pos(pos) {}
    template <bool MASKED>
    __device__ __forceinline__ bool visible(int key) const {
        bool ok = key <= pos;
        if (MASKED && ok) ok = kvr[key] != 0;
        return ok;
    }
    typedef int Row;      // the row to load: the key's, or row *pos for an invisible key
    __device__ __forceinline__ Row row(int key, bool ok) const { return ok ? key : pos; }
};

template <typename T, int HD_>
struct DenseKV : OneCacheKeys {
    static constexpr int HD = HD_, EPL = 16 / (int)sizeof(T);
    static constexpr bool SCALED = false;
    typedef T Reg __attribute__((ext_vector_type(EPL)));
    const T* __restrict__ kc;
    const T* __restrict__ vc;
    const uint8_t* key_valid;
    int nkv, tmax;
    int64_t base;      // the (row, kvh) cache's first row, this lane's piece
    __device__ __forceinline__ DenseKV(const T* __restrict__ kc, const T* __restrict__ vc, const int64_t* pos_p, const uint8_t* key_valid, int nkv, int tmax)
        : OneCacheKeys(pos_p, tmax), kc(kc), vc(vc), key_valid(key_valid), nkv(nkv), tmax(tmax) {}
    template <bool MASKED>
    __device__ __forceinline__ void seat(int r, int kvh, int c) {
        base = ((int64_t)r * nkv + kvh) * tmax * HD + c * EPL;
        if (MASKED) kvr = key_valid + (int64_t)r * tmax;
    }
    typedef const T* Cache;
    __device__ __forceinline__ Cache k() const { return kc; }
    __device__ __forceinline__ Cache v() const { return vc; }
    static __device__ __forceinline__ Reg zero() {
        Reg z;
#pragma unroll
        for (int e = 0; e < EPL; e++) z[e] = (T)0.f;
        return z;
    }
    __device__ __forceinline__ Reg load(const T* __restrict__ src, Row row, int, bool ok, const Reg& zero) const {
        const Reg v = *reinterpret_cast<const Reg*>(src + base + (int64_t)row * HD);
        return ok ? v : zero;
    }
    static __device__ __forceinline__ void widen(const Reg& v, float (&f)[EPL]) {
#pragma unroll
        for (int e = 0; e < EPL; e++) f[e] = (float)v[e];
    }
};

// fp8 K/V cache (opt-in: kv_cache="fp8").  The cache of a layer is e4m3 codes kc8 / vc8 [B, nkv, tmax, hd] (uint8) and one power-of-two
// scale per row ks / vs [B, nkv, tmax] (ops.quantize_fp8_kv; fp8_code.h), so code * scale is exactly a bf16 number and the cache is an
// ordinary bf16 cache stored in half the bytes.
// Contract: the output equals, bit for bit, what vtgb_llm_decode_attention_split returns on the dequantised cache.  The partition is
// DenseKV<bf16_t>'s -- 8 consecutive elements of a row per lane (an 8-byte load here), LPR = hd / 8 lanes per row, the same rows per
// lane, waves and chunks -- and a scale 2^e moves through every rounding unchanged (no overflow, no subnormal: |e| <= 120 and fp32
// partial sums of bf16 products): sum_e fmaf(q, c 2^e, .) = 2^e sum_e fmaf(q, c, .), so the K scale multiplies the row's score after its
// lanes are summed, and fmaf(p, c 2^e, acc) = fmaf(p 2^e, c, acc), so the V scale multiplies the softmax weight.  Pass 1 reads both scales
// in the softmax stage (four coalesced keys per lane), where the weights pass through LDS anyway.
// Visibility is the dense cache's: nothing past *pos is read -- codes or scales --, an invisible key's codes are replaced by zeros and its
// scales by 1 before any product, so a stale or masked slot may hold anything (the e4m3 NaN code, a NaN scale).
template <int HD_>
struct Fp8KV : OneCacheKeys {
    static constexpr int HD = HD_, EPL = 8;
    static constexpr bool SCALED = true;
    typedef uint2 Reg;
    const uint8_t* __restrict__ kc8;
    const uint8_t* __restrict__ vc8;
    const float* __restrict__ ks;
    const float* __restrict__ vs;
    const uint8_t* key_valid;
    int nkv, tmax, c;
    int64_t row0;      // the (row, kvh) cache's first row: codes at row * HD, scales at row
    __device__ __forceinline__ Fp8KV(const uint8_t* __restrict__ kc8, const uint8_t* __restrict__ vc8, const float* __restrict__ ks,
                                     const float* __restrict__ vs, const int64_t* pos_p, const uint8_t* key_valid, int nkv, int tmax)
        : OneCacheKeys(pos_p, tmax), kc8(kc8), vc8(vc8), ks(ks), vs(vs), key_valid(key_valid), nkv(nkv), tmax(tmax) {}
    template <bool MASKED>
    __device__ __forceinline__ void seat(int r, int kvh, int c_) {
        row0 = ((int64_t)r * nkv + kvh) * tmax;
        c = c_;
        if (MASKED) kvr = key_valid + (int64_t)r * tmax;
    }
    typedef const uint8_t* Cache;
    __device__ __forceinline__ Cache k() const { return kc8; }
    __device__ __forceinline__ Cache v() const { return vc8; }
    static __device__ __forceinline__ Reg zero() { return make_uint2(0u, 0u); }
    __device__ __forceinline__ Reg load(const uint8_t* __restrict__ src, Row row, int, bool ok, const Reg&) const {
        const uint2 v = *reinterpret_cast<const uint2*>(src + (row0 + row) * HD + c * EPL);
        return ok ? v : make_uint2(0u, 0u);      // (an immediate, not the body's ``zero``: with that one hipcc takes 180 VGPRs at hd 128, 101 at hd 64)
    }
    static __device__ __forceinline__ void widen(const Reg& v, float (&f)[EPL]) {
        float lo[4], hi[4];
        kv8_widen4(v.x, lo);
        kv8_widen4(v.y, hi);
#pragma unroll
        for (int e = 0; e < 4; e++) f[e] = lo[e], f[4 + e] = hi[e];
    }
    __device__ __forceinline__ void scales(int key, bool ok, float& sk, float& sv) const {
        const float a = ks[row0 + row(key, ok)], v = vs[row0 + row(key, ok)];
        sk = ok ? a : 1.f;
        sv = ok ? v : 1.f;
    }
};

// Beam search (opt-in: beam_search="graph").  Two K/V sources and no K/V copies when beams are re-ordered: the R = B * K beam rows of a
// batch share ONE prompt cache per batch item, kp / vp [B, nkv, tmax_p, hd] (the prefill's, on B rows), and append what they generate to
// kg / vg [R, nkv, tmax_g, hd] at slot = the step; src_row [R, tmax_g] int32 names, for beam row r, the generated-cache row that holds
// its key of slot s (its ancestor at that step).  Global key t of row r:
//   t <  *n_prompt:  kp[r / K, kvh, t]                                        (and key_valid[r / K, t] != 0, MASKED)
//   t >= *n_prompt:  kg[clamp(src_row[r, t - *n_prompt], 0, R - 1), kvh, t - *n_prompt]
// visible while t <= *pos (clamped to *n_prompt + tmax_g - 1; *n_prompt to [0, tmax_p]).  A table entry is clamped before use: a wrong
// table gives wrong numbers, never a read outside the caches.
// Contract: chunk, wave, a lane's keys and the order inside every sum follow the GLOBAL key index t, so the output equals, bit for bit,
// vtgb_llm_decode_attention_split on the cache [R, nkv, T, hd] that this gather materialises.  Nothing past *pos, no masked slot and no
// prompt slot >= *n_prompt reaches a product (an invisible row's load goes to row 0 of the item's prompt cache and is selected away).
// Workspace and pass 2 see tmax = tmax_p + tmax_g.
template <typename T, int HD_>
struct BeamKV {
    static constexpr int HD = HD_, EPL = 16 / (int)sizeof(T);
    static constexpr bool SCALED = false;
    typedef T Reg __attribute__((ext_vector_type(EPL)));
    typedef int64_t Row;      // element offset of the row: into kp / vp (key < np or invisible) or kg / vg; the table is read once per key
    const T* __restrict__ kp;
    const T* __restrict__ vp;
    const T* __restrict__ kg;
    const T* __restrict__ vg;
    const int32_t* __restrict__ src_row;
    const uint8_t* key_valid;
    const uint8_t* kvr;
    int R, K, nkv, tmax_p, tmax_g, np, pos, walk_pos, r, kvh, c;
    int64_t pbase;      // row 0 of the item's prompt cache (this K/V head, this piece)
    __device__ __forceinline__ BeamKV(const T* __restrict__ kp, const T* __restrict__ vp, const T* __restrict__ kg, const T* __restrict__ vg,
                                      const int32_t* __restrict__ src_row, const int64_t* np_p, const int64_t* pos_p, const uint8_t* key_valid, int R,
                                      int K, int nkv, int tmax_p, int tmax_g)
        : kp(kp), vp(vp), kg(kg), vg(vg), src_row(src_row), key_valid(key_valid), kvr(nullptr), R(R), K(K), nkv(nkv), tmax_p(tmax_p), tmax_g(tmax_g) {
        const int tmax = tmax_p + tmax_g;
        const int64_t np64 = *np_p, pos64 = *pos_p;
        np = (int)(np64 < 0 ? 0 : np64 > tmax_p ? tmax_p : np64);
        walk_pos = (int)(pos64 < -1 ? -1 : pos64 > tmax - 1 ? tmax - 1 : pos64);
        pos = min(walk_pos, np + tmax_g - 1);
    }
    template <bool MASKED>
    __device__ __forceinline__ void seat(int r_, int kvh_, int c_) {
        r = r_, kvh = kvh_, c = c_;
        const int b = r / K;
        pbase = ((int64_t)b * nkv + kvh) * tmax_p * HD + c * EPL;
        if (MASKED) kvr = key_valid + (int64_t)b * tmax_p;
    }
    template <bool MASKED>
    __device__ __forceinline__ bool visible(int key) const {
        bool ok = key <= pos;
        if (MASKED && ok && key < np) ok = kvr[key] != 0;
        return ok;
    }
    __device__ __forceinline__ Row row(int key, bool ok) const {
        int64_t o = pbase;
        if (ok && key < np) {
            o = pbase + (int64_t)key * HD;
        } else if (ok) {
            const int g = key - np;      // < tmax_g: key <= pos <= np + tmax_g - 1
            int sr = src_row[(int64_t)r * tmax_g + g];
            sr = sr < 0 ? 0 : sr >= R ? R - 1 : sr;
            o = (((int64_t)sr * nkv + kvh) * tmax_g + g) * HD + c * EPL;
        }
        return o;
    }
    struct Cache {
        const T* __restrict__ p;
        const T* __restrict__ g;
    };
    __device__ __forceinline__ Cache k() const { return Cache{kp, kg}; }
    __device__ __forceinline__ Cache v() const { return Cache{vp, vg}; }
    static __device__ __forceinline__ Reg zero() { return DenseKV<T, HD_>::zero(); }
    __device__ __forceinline__ Reg load(Cache cache, Row row, int key, bool ok, const Reg& zero) const {
        const T* p = (ok && key >= np) ? cache.g : cache.p;
        const Reg v = *reinterpret_cast<const Reg*>(p + row);
        return ok ? v : zero;
    }
    static __device__ __forceinline__ void widen(const Reg& v, float (&f)[EPL]) { DenseKV<T, HD_>::widen(v, f); }
};

// Beam search over the fp8 K/V cache (opt-in: beam_search="graph+kv8" with kv_cache="fp8").  BeamKV's two caches, visibility and ancestry
// table over Fp8KV's storage: kp8 / vp8 [B, nkv, tmax_p, hd] codes with kps / vps [B, nkv, tmax_p] scales (the fp8 prefill's, on B rows),
// kg8 / vg8 [R, nkv, tmax_g, hd] with kgs / vgs [R, nkv, tmax_g] (vtgb_llm_rope_cache_fp8 at slot = the step).  A key resolves to ONE cache
// row (Row: its index in rows of HD codes, into the prompt or the generated cache), which serves its codes (row * HD) and its scales (row)
// alike; an invisible key resolves to row 0 of the item's prompt cache, its codes selected to zeros and its scales to 1.
// Contract: the partition is Fp8KV's (EPL = 8, 8-byte loads, scales applied in the softmax stage) on the global key index, so the output equals,
// bit for bit, vtgb_llm_decode_attention_beam on the dequantised caches -- and so vtgb_llm_decode_attention_split on the gathered one.
template <int HD_>
struct BeamFp8KV {
    static constexpr int HD = HD_, EPL = 8;
    static constexpr bool SCALED = true;
    typedef uint2 Reg;
    typedef int64_t Row;
    const uint8_t* __restrict__ kp8;
    const uint8_t* __restrict__ vp8;
    const float* __restrict__ kps;
    const float* __restrict__ vps;
    const uint8_t* __restrict__ kg8;
    const uint8_t* __restrict__ vg8;
    const float* __restrict__ kgs;
    const float* __restrict__ vgs;
    const int32_t* __restrict__ src_row;
    const uint8_t* key_valid;
    const uint8_t* kvr;
    int R, K, nkv, tmax_p, tmax_g, np, pos, walk_pos, r, kvh, c, softmax_waves;
    int64_t prow0;      // row 0 of the item's prompt cache (this K/V head)
    float psk[4], psv[4];      // the scales of this lane's four softmax keys, fetched in seat() (indexed by constants only: registers)
    __device__ __forceinline__ BeamFp8KV(const vtgb_llm_decode_attention_beam_fp8_args& a)
        : kp8(a.kp8), vp8(a.vp8), kps(a.kps), vps(a.vps), kg8(a.kg8), vg8(a.vg8), kgs(a.kgs), vgs(a.vgs), src_row(a.src_row), key_valid(a.key_valid),
          kvr(nullptr), R(a.R), K(a.K), nkv(a.nkv), tmax_p(a.tmax_p), tmax_g(a.tmax_g), softmax_waves(min(DEC_SPLIT_HEADS, a.nq / a.nkv)) {
        const int tmax = tmax_p + tmax_g;
        const int64_t np64 = *a.n_prompt, pos64 = *a.pos;
        np = (int)(np64 < 0 ? 0 : np64 > tmax_p ? tmax_p : np64);
        walk_pos = (int)(pos64 < -1 ? -1 : pos64 > tmax - 1 ? tmax - 1 : pos64);
        pos = min(walk_pos, np + tmax_g - 1);
    }
    template <bool MASKED>
    __device__ __forceinline__ void seat(int r_, int kvh_, int c_) {
        r = r_, kvh = kvh_, c = c_;
        const int b = r / K;
        prow0 = ((int64_t)b * nkv + kvh) * tmax_p;
        if (MASKED) kvr = key_valid + (int64_t)b * tmax_p;
        // A generated key's scale lies behind two dependent loads (the table, then the row's scale).  Pass 1 asks for the scales in its softmax
        // stage, behind a barrier, where that chain would be on the workgroup's critical path (measured: the kernel 9 % slower than the bf16
        // beam kernel on half the bytes); so the waves that can take part in that stage (wave < min(DEC_SPLIT_HEADS, nq / nkv) >= nh) fetch the
        // scales of their four softmax keys -- key = chunk * 256 + lane + 64 j, chunk = blockIdx.x, as pass 1 defines them -- here, where
        // the loads fly behind the K loads.  scales() hands them out and checks nothing but the key's j.
#pragma unroll
        for (int j = 0; j < 4; j++) psk[j] = psv[j] = 1.f;
        if ((int)(threadIdx.x >> 6) < softmax_waves) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int key = blockIdx.x * DEC_SPLIT_CHUNK + (threadIdx.x & 63) + 64 * j;
                const bool ok = visible<MASKED>(key), gen = ok && key >= np;
                const Row o = row(key, ok);
                psk[j] = (gen ? kgs : kps)[o];
                psv[j] = (gen ? vgs : vps)[o];
            }
        }
    }
    template <bool MASKED>
    __device__ __forceinline__ bool visible(int key) const {
        bool ok = key <= pos;
        if (MASKED && ok && key < np) ok = kvr[key] != 0;
        return ok;
    }
    __device__ __forceinline__ Row row(int key, bool ok) const {
        int64_t o = prow0;
        if (ok && key < np) {
            o = prow0 + key;
        } else if (ok) {
            const int g = key - np;      // < tmax_g: key <= pos <= np + tmax_g - 1
            int sr = src_row[(int64_t)r * tmax_g + g];
            sr = sr < 0 ? 0 : sr >= R ? R - 1 : sr;
            o = ((int64_t)sr * nkv + kvh) * tmax_g + g;
        }
        return o;
    }
    struct Cache {
        const uint8_t* __restrict__ p;
        const uint8_t* __restrict__ g;
    };
    __device__ __forceinline__ Cache k() const { return Cache{kp8, kg8}; }
    __device__ __forceinline__ Cache v() const { return Cache{vp8, vg8}; }
    static __device__ __forceinline__ Reg zero() { return make_uint2(0u, 0u); }
    __device__ __forceinline__ Reg load(Cache cache, Row row, int key, bool ok, const Reg&) const {
        const uint8_t* p = (ok && key >= np) ? cache.g : cache.p;
        const uint2 v = *reinterpret_cast<const uint2*>(p + row * HD + c * EPL);
        return ok ? v : make_uint2(0u, 0u);      // (an immediate, as in Fp8KV::load)
    }
    static __device__ __forceinline__ void widen(const Reg& v, float (&f)[EPL]) { Fp8KV<HD_>::widen(v, f); }
    __device__ __forceinline__ void scales(int key, bool ok, float& sk, float& sv) const {
        const int j = key >> 6 & 3;      // (key = chunk * 256 + lane + 64 j)
        const float a = j == 0 ? psk[0] : j == 1 ? psk[1] : j == 2 ? psk[2] : psk[3];
        const float v = j == 0 ? psv[0] : j == 1 ? psv[1] : j == 2 ? psv[2] : psv[3];
        sk = ok ? a : 1.f;
        sv = ok ? v : 1.f;
    }
};

// ---- pass 1, for the workgroup (blockIdx.x = chunk,blockIdx.y = K/V head x head block, blockIdx.z = row); ``rows`` = gridDim.z
template <bool MASKED, typename Src, typename TQ>
__device__ __forceinline__ void decode_attn_pass1(Src src, const TQ* __restrict__ q, float* __restrict__ ws, int rows, int nq, int nkv, int tmax,
                                                  float scale) {
    constexpr int HD = Src::HD, EPL = Src::EPL;
    constexpr int LPR = HD / EPL;                 // lanes per row
    constexpr int RPI = 64 / LPR;                 // rows per load instruction
    constexpr int NI = 64 / RPI;                  // load instructions per wave (== LPR)
    typedef typename Src::Reg Reg;
    __shared__ float qs[DEC_SPLIT_HEADS][HD];
    __shared__ float sc[DEC_SPLIT_HEADS][DEC_SPLIT_CHUNK];
    __shared__ __attribute__((aligned(16))) float red[4][DEC_SPLIT_HEADS][HD];

    const int chunk = blockIdx.x, r = blockIdx.z;
    if (chunk * DEC_SPLIT_CHUNK > src.walk_pos) return;
    const int group = nq / nkv, nhb = (group + DEC_SPLIT_HEADS - 1) / DEC_SPLIT_HEADS;
    const int kvh = blockIdx.y / nhb, hb = blockIdx.y % nhb;
    const int head0 = kvh * group + hb * DEC_SPLIT_HEADS, nh = min(DEC_SPLIT_HEADS, group - hb * DEC_SPLIT_HEADS);
    const int nc = (tmax + DEC_SPLIT_CHUNK - 1) / DEC_SPLIT_CHUNK;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane % LPR, rs = lane / LPR;      // this lane's piece of a row and row slot
    src.template seat<MASKED>(r, kvh, c);

    for (int i = tid; i < nh * HD; i += 256) qs[i / HD][i % HD] = (float)q[((int64_t)r * nq + head0) * HD + i];

    // ---- K: the wave's 64 rows -> registers (row kl0 + i * RPI of instruction i); invisible rows are zeros
    const int kl0 = wave * 64 + rs, key0 = chunk * DEC_SPLIT_CHUNK + kl0;
    unsigned vis = 0;
    typename Src::Row row[NI];
#pragma unroll
    for (int i = 0; i < NI; i++) {
        const bool ok = src.template visible<MASKED>(key0 + i * RPI);
        vis |= ok ? 1u << i : 0u;
        row[i] = src.row(key0 + i * RPI, ok);
    }
    // No branch per row is written: an invisible row's load goes to its safe row and its value is selected away.  hipcc turns such a
    // select into a skip of the load, the address computed next to it, and that keeps the former copies' registers -- but only in
    // this shape: one lambda called for K and for V, ``zero`` built once outside it and taken by reference, the row resolved above.
    // As a plain loop over src.load() the selects stay, and the NI row addresses live from the K loads to the V loads: 181 VGPRs
    // and 2 waves per SIMD at bf16 hd 128 instead of 168 and 3 (tools/kernel_resources.sh).
    const Reg zero = Src::zero();
    auto load_rows = [&](typename Src::Cache cache, Reg (&reg)[NI]) {
#pragma unroll
        for (int i = 0; i < NI; i++) {
            const bool ok = vis >> i & 1;
            reg[i] = src.load(cache, row[i], key0 + i * RPI, ok, zero);
        }
    };
    Reg reg[NI];
    load_rows(src.k(), reg);
    __syncthreads();      // qs

    // ---- scores: per head, the lane's piece of every row, then the row's LPR lanes (SCALED: still without the K scale and ``scale``)
    for (int h = 0; h < nh; h++) {
        float qv[EPL];
#pragma unroll
        for (int e = 0; e < EPL; e++) qv[e] = qs[h][c * EPL + e];
#pragma unroll
        for (int i = 0; i < NI; i++) {
            float kf[EPL];
            Src::widen(reg[i], kf);
            float dot = 0.f;
#pragma unroll
            for (int e = 0; e < EPL; e++) dot = fmaf(qv[e], kf[e], dot);
            dot = group_sum<LPR>(dot);
            if (c == 0) sc[h][kl0 + i * RPI] = (vis >> i & 1) ? (Src::SCALED ? dot : dot * scale) : -INFINITY;
        }
    }
    // ---- V replaces K in the registers (the loads fly behind the softmax)
    load_rows(src.v(), reg);
    __syncthreads();      // sc

    // ---- softmax statistics of the chunk: wave w takes the heads w, w + 4.  SCALED: a lane's four keys lane + 64 j bring their K scale,
    // which makes the score (dot * 2^ek) * scale = the dense cache's dot * scale, and their V scale, which goes into the weight left in sc
    if (wave < nh) {
        float sk[4], sv[4];
        if constexpr (Src::SCALED) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int key = chunk * DEC_SPLIT_CHUNK + lane + 64 * j;
                src.scales(key, src.template visible<MASKED>(key), sk[j], sv[j]);
            }
        }
        for (int h = wave; h < nh; h += 4) {
            float s[4], m = -INFINITY;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                s[j] = sc[h][lane + 64 * j];
                if constexpr (Src::SCALED) s[j] = s[j] == -INFINITY ? s[j] : (s[j] * sk[j]) * scale;
                m = fmaxf(m, s[j]);
            }
            for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
#pragma unroll
            for (int j = 0; j < 4; j++) {
                s[j] = s[j] == -INFINITY ? 0.f : expf(s[j] - m);      // (an invisible key: exactly 0, also when the chunk has no visible key)
                if constexpr (Src::SCALED) sc[h][lane + 64 * j] = s[j] * sv[j];
                else sc[h][lane + 64 * j] = s[j];
            }
            const float l = group_sum<64>((s[0] + s[1]) + (s[2] + s[3]));
            if (lane == 0) {
                float* ml = ws + (int64_t)rows * nq * nc * HD + (((int64_t)r * nq + head0 + h) * nc + chunk) * 2;
                ml[0] = m;
                ml[1] = l;
            }
        }
    }
    __syncthreads();      // sc = weights (SCALED: x V scales)

    // ---- O: per head, the lane's rows in ascending order, then the wave's row slots, then (below) the four waves
    for (int h = 0; h < nh; h++) {
        float acc[EPL];
#pragma unroll
        for (int e = 0; e < EPL; e++) acc[e] = 0.f;
#pragma unroll
        for (int i = 0; i < NI; i++) {
            const float p = sc[h][kl0 + i * RPI];
            float vf[EPL];
            Src::widen(reg[i], vf);
#pragma unroll
            for (int e = 0; e < EPL; e++) acc[e] = fmaf(p, vf[e], acc[e]);
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

template <typename T, int HD, bool MASKED>
__global__ __launch_bounds__(256) void llm_decode_attn_split_kernel(const T* __restrict__ q, const T* __restrict__ kc, const T* __restrict__ vc,
                                                                    float* __restrict__ ws, const int64_t* __restrict__ pos_p,
                                                                    const uint8_t* __restrict__ key_valid, int B, int nq, int nkv, int tmax,
                                                                    float scale) {
    decode_attn_pass1<MASKED>(DenseKV<T, HD>(kc, vc, pos_p, key_valid, nkv, tmax), q, ws, B, nq, nkv, tmax, scale);
}

template <int HD, bool MASKED>
__global__ __launch_bounds__(256) void llm_decode_attn_split_fp8_kernel(const bf16_t* __restrict__ q, const uint8_t* __restrict__ kc8,
                                                                        const uint8_t* __restrict__ vc8, const float* __restrict__ ks,
                                                                        const float* __restrict__ vs, float* __restrict__ ws,
                                                                        const int64_t* __restrict__ pos_p, const uint8_t* __restrict__ key_valid,
                                                                        int B, int nq, int nkv, int tmax, float scale) {
    decode_attn_pass1<MASKED>(Fp8KV<HD>(kc8, vc8, ks, vs, pos_p, key_valid, nkv, tmax), q, ws, B, nq, nkv, tmax, scale);
}

template <typename T, int HD, bool MASKED>
__global__ __launch_bounds__(256) void llm_decode_attn_beam_kernel(const T* __restrict__ q, const T* __restrict__ kp, const T* __restrict__ vp,
                                                                   const T* __restrict__ kg, const T* __restrict__ vg,
                                                                   const int32_t* __restrict__ src_row, float* __restrict__ ws,
                                                                   const int64_t* __restrict__ np_p, const int64_t* __restrict__ pos_p,
                                                                   const uint8_t* __restrict__ key_valid, int R, int K, int nq, int nkv, int tmax_p,
                                                                   int tmax_g, float scale) {
    decode_attn_pass1<MASKED>(BeamKV<T, HD>(kp, vp, kg, vg, src_row, np_p, pos_p, key_valid, R, K, nkv, tmax_p, tmax_g), q, ws, R, nq, nkv,
                              tmax_p + tmax_g, scale);
}

template <int HD, bool MASKED>
__global__ __launch_bounds__(256) void llm_decode_attn_beam_fp8_kernel(const vtgb_llm_decode_attention_beam_fp8_args a) {
    const bf16_t* __restrict__ q = (const bf16_t*)a.q;
    float* __restrict__ ws = (float*)a.workspace;
    decode_attn_pass1<MASKED>(BeamFp8KV<HD>(a), q, ws, a.R, a.nq, a.nkv, a.tmax_p + a.tmax_g, a.scale);
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

// ---- host.  Pass 1 (``masked`` where there is a key_valid, else ``plain``, with the kernel's own arguments ``args``) and pass 2 on
// stream s.  ``args`` repeats rows / nq / nkv / tmax / pos / workspace in the order its kernel takes them: the two must agree.
template <typename T, typename... KArgs, typename... Args>
static int launch_decode_attn(void (*masked)(KArgs...), void (*plain)(KArgs...), const uint8_t* key_valid, int rows, int nq, int nkv, int hd, int tmax,
                              const int64_t* pos, void* workspace, void* out, hipStream_t s, Args... args) {
    const int group = nq / nkv, nhb = (group + DEC_SPLIT_HEADS - 1) / DEC_SPLIT_HEADS, nc = (tmax + DEC_SPLIT_CHUNK - 1) / DEC_SPLIT_CHUNK;
    hipLaunchKernelGGL(key_valid ? masked : plain, dim3(nc, nkv * nhb, rows), dim3(256), 0, s, args...);
    VTGB_HIP(hipGetLastError());
    hipLaunchKernelGGL(llm_decode_attn_combine_kernel<T>, dim3((unsigned)((int64_t)rows * nq)), dim3(hd), 0, s, (const float*)workspace, (T*)out, pos,
                       (int64_t)rows * nq, hd, tmax);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

// What every entry requires of its heads, cache lengths (tmax_g = 0: one cache of tmax), grid and pointers, reported under the entry's name.
struct DecodeAttnShape {
    const char* entry;
    const char* rows_name;
    int rows, nq, nkv, hd, tmax, tmax_g;
};

static int check_decode_attn(const DecodeAttnShape& g, std::initializer_list<const void*> align16, std::initializer_list<const void*> align4,
                             const char* alignment) {
    VTGB_REQUIRE(g.nq % g.nkv == 0, VTGB_EINVAL, "%s: nq=%d is not a multiple of nkv=%d", g.entry, g.nq, g.nkv);
    VTGB_REQUIRE(g.hd == 64 || g.hd == 128, VTGB_EUNSUPPORTED, "%s: hd=%d, built for 64 and 128", g.entry, g.hd);
    const bool lengths_ok = g.tmax % 64 == 0 && g.tmax_g % 64 == 0 && (int64_t)g.tmax + g.tmax_g <= DEC_SPLIT_MAX_T;
    if (g.tmax_g)
        VTGB_REQUIRE(lengths_ok, VTGB_EUNSUPPORTED, "%s: tmax_p=%d / tmax_g=%d are not multiples of 64 with a sum up to %d", g.entry, g.tmax, g.tmax_g,
                     DEC_SPLIT_MAX_T);
    VTGB_REQUIRE(lengths_ok, VTGB_EUNSUPPORTED, "%s: tmax=%d is not a multiple of 64 up to %d", g.entry, g.tmax, DEC_SPLIT_MAX_T);
    const int nhb = (g.nq / g.nkv + DEC_SPLIT_HEADS - 1) / DEC_SPLIT_HEADS;
    VTGB_REQUIRE(g.rows <= 65535 && (int64_t)g.nkv * nhb <= 65535, VTGB_EUNSUPPORTED, "%s: %s=%d / nq=%d exceed the grid", g.entry, g.rows_name, g.rows,
                 g.nq);
    bool aligned = true;
    for (const void* p : align16) aligned &= (reinterpret_cast<uintptr_t>(p) & 15) == 0;
    for (const void* p : align4) aligned &= (reinterpret_cast<uintptr_t>(p) & 3) == 0;
    VTGB_REQUIRE(aligned, VTGB_EUNSUPPORTED, "%s: %s", g.entry, alignment);
    return VTGB_OK;
}

extern "C" int64_t vtgb_llm_decode_attention_split_workspace_bytes(int32_t B, int32_t nq, int32_t hd, int32_t tmax) {
    if (B <= 0 || nq <= 0 || hd <= 0 || tmax <= 0) return 0;
    const int64_t nc = (tmax + DEC_SPLIT_CHUNK - 1) / DEC_SPLIT_CHUNK;
    return (int64_t)B * nq * nc * (hd + 2) * (int64_t)sizeof(float);
}

template <typename T, int HD>
static int launch_split(const void* q, const void* kc, const void* vc, void* out, const int64_t* pos, const uint8_t* key_valid, void* workspace,
                        int B, int nq, int nkv, int tmax, float scale, hipStream_t s) {
    return launch_decode_attn<T>(llm_decode_attn_split_kernel<T, HD, true>, llm_decode_attn_split_kernel<T, HD, false>, key_valid, B, nq, nkv, HD, tmax,
                                 pos, workspace, out, s, (const T*)q, (const T*)kc, (const T*)vc, (float*)workspace, pos, key_valid, B, nq, nkv, tmax, scale);
}

extern "C" int vtgb_llm_decode_attention_split(int dtype, const void* q, const void* kc, const void* vc, void* out, const int64_t* pos,
                                               const uint8_t* key_valid, void* workspace, int32_t B, int32_t nq, int32_t nkv, int32_t hd,
                                               int32_t tmax, float scale, vtgb_stream_t stream) {
    VTGB_REQUIRE(q && kc && vc && out && pos && workspace, VTGB_EINVAL, "llm_decode_attention_split: NULL operand");
    VTGB_REQUIRE((dtype == VTGB_BF16 || dtype == VTGB_F32) && B > 0 && nq > 0 && nkv > 0 && tmax > 0, VTGB_EINVAL,
                 "llm_decode_attention_split: bad argument");
    VTGB_TRY(check_decode_attn({"llm_decode_attention_split", "B", B, nq, nkv, hd, tmax, 0}, {q, kc, vc, out, workspace}, {},
                               "q / kc / vc / out / workspace need 16-byte alignment"));
    hipStream_t s = (hipStream_t)stream;
    if (dtype == VTGB_BF16)
        return hd == 128 ? launch_split<bf16_t, 128>(q, kc, vc, out, pos, key_valid, workspace, B, nq, nkv, tmax, scale, s)
                         : launch_split<bf16_t, 64>(q, kc, vc, out, pos, key_valid, workspace, B, nq, nkv, tmax, scale, s);
    return hd == 128 ? launch_split<float, 128>(q, kc, vc, out, pos, key_valid, workspace, B, nq, nkv, tmax, scale, s)
                     : launch_split<float, 64>(q, kc, vc, out, pos, key_valid, workspace, B, nq, nkv, tmax, scale, s);
}

template <int HD>
static int launch_split_fp8(const void* q, const uint8_t* kc8, const uint8_t* vc8, const float* ks, const float* vs, void* out, const int64_t* pos,
                            const uint8_t* key_valid, void* workspace, int B, int nq, int nkv, int tmax, float scale, hipStream_t s) {
    return launch_decode_attn<bf16_t>(llm_decode_attn_split_fp8_kernel<HD, true>, llm_decode_attn_split_fp8_kernel<HD, false>, key_valid, B, nq, nkv, HD, tmax,
                                      pos, workspace, out, s, (const bf16_t*)q, kc8, vc8, ks, vs, (float*)workspace, pos, key_valid, B, nq, nkv, tmax, scale);
}

extern "C" int vtgb_llm_decode_attention_split_fp8(int dtype, const void* q, const uint8_t* kc8, const uint8_t* vc8, const float* ks, const float* vs,
                                                   void* out, const int64_t* pos, const uint8_t* key_valid, void* workspace, int32_t B, int32_t nq,
                                                   int32_t nkv, int32_t hd, int32_t tmax, float scale, vtgb_stream_t stream) {
    VTGB_REQUIRE(q && kc8 && vc8 && ks && vs && out && pos && workspace, VTGB_EINVAL, "llm_decode_attention_split_fp8: NULL operand");
    VTGB_REQUIRE(dtype == VTGB_BF16 && B > 0 && nq > 0 && nkv > 0 && tmax > 0, VTGB_EINVAL,
                 "llm_decode_attention_split_fp8: bad argument (activations are VTGB_BF16)");
    VTGB_TRY(check_decode_attn({"llm_decode_attention_split_fp8", "B", B, nq, nkv, hd, tmax, 0}, {q, kc8, vc8, out, workspace}, {ks, vs},
                               "q / kc8 / vc8 / out / workspace need 16-byte, ks / vs 4-byte alignment"));
    hipStream_t s = (hipStream_t)stream;
    return hd == 128 ? launch_split_fp8<128>(q, kc8, vc8, ks, vs, out, pos, key_valid, workspace, B, nq, nkv, tmax, scale, s)
                     : launch_split_fp8<64>(q, kc8, vc8, ks, vs, out, pos, key_valid, workspace, B, nq, nkv, tmax, scale, s);
}

template <typename T, int HD>
static int launch_beam(const vtgb_llm_decode_attention_beam_args* a, hipStream_t s) {
    return launch_decode_attn<T>(llm_decode_attn_beam_kernel<T, HD, true>, llm_decode_attn_beam_kernel<T, HD, false>, a->key_valid, a->R, a->nq, a->nkv, HD,
                                 a->tmax_p + a->tmax_g, a->pos, a->workspace, a->out, s, (const T*)a->q, (const T*)a->kp, (const T*)a->vp, (const T*)a->kg,
                                 (const T*)a->vg, a->src_row, (float*)a->workspace, a->n_prompt, a->pos, a->key_valid, a->R, a->K, a->nq, a->nkv, a->tmax_p,
                                 a->tmax_g, a->scale);
}

extern "C" int vtgb_llm_decode_attention_beam(const vtgb_llm_decode_attention_beam_args* a, vtgb_stream_t stream) {
    VTGB_REQUIRE(a, VTGB_EINVAL, "llm_decode_attention_beam: NULL args");
    VTGB_REQUIRE(a->q && a->kp && a->vp && a->kg && a->vg && a->src_row && a->out && a->n_prompt && a->pos && a->workspace, VTGB_EINVAL,
                 "llm_decode_attention_beam: NULL operand");
    VTGB_REQUIRE((a->dtype == VTGB_BF16 || a->dtype == VTGB_F32) && a->R > 0 && a->K > 0 && a->nq > 0 && a->nkv > 0 && a->tmax_p > 0 && a->tmax_g > 0,
                 VTGB_EINVAL, "llm_decode_attention_beam: bad argument");
    VTGB_REQUIRE(a->R % a->K == 0, VTGB_EINVAL, "llm_decode_attention_beam: R=%d rows are not a multiple of K=%d beams", a->R, a->K);
    VTGB_TRY(check_decode_attn({"llm_decode_attention_beam", "R", a->R, a->nq, a->nkv, a->hd, a->tmax_p, a->tmax_g},
                               {a->q, a->kp, a->vp, a->kg, a->vg, a->out, a->workspace}, {a->src_row},
                               "q / kp / vp / kg / vg / out / workspace need 16-byte, src_row 4-byte alignment"));
    hipStream_t s = (hipStream_t)stream;
    if (a->dtype == VTGB_BF16) return a->hd == 128 ? launch_beam<bf16_t, 128>(a, s) : launch_beam<bf16_t, 64>(a, s);
    return a->hd == 128 ? launch_beam<float, 128>(a, s) : launch_beam<float, 64>(a, s);
}

template <int HD>
static int launch_beam_fp8(const vtgb_llm_decode_attention_beam_fp8_args* a, hipStream_t s) {
    return launch_decode_attn<bf16_t>(llm_decode_attn_beam_fp8_kernel<HD, true>, llm_decode_attn_beam_fp8_kernel<HD, false>, a->key_valid, a->R, a->nq, a->nkv,
                                      HD, a->tmax_p + a->tmax_g, a->pos, a->workspace, a->out, s, *a);
}

extern "C" int vtgb_llm_decode_attention_beam_fp8(const vtgb_llm_decode_attention_beam_fp8_args* a, vtgb_stream_t stream) {
    VTGB_REQUIRE(a, VTGB_EINVAL, "llm_decode_attention_beam_fp8: NULL args");
    VTGB_REQUIRE(a->q && a->kp8 && a->vp8 && a->kps && a->vps && a->kg8 && a->vg8 && a->kgs && a->vgs && a->src_row && a->out && a->n_prompt && a->pos &&
                     a->workspace,
                 VTGB_EINVAL, "llm_decode_attention_beam_fp8: NULL operand");
    VTGB_REQUIRE(a->dtype == VTGB_BF16 && a->R > 0 && a->K > 0 && a->nq > 0 && a->nkv > 0 && a->tmax_p > 0 && a->tmax_g > 0, VTGB_EINVAL,
                 "llm_decode_attention_beam_fp8: bad argument (activations are VTGB_BF16)");
    VTGB_REQUIRE(a->R % a->K == 0, VTGB_EINVAL, "llm_decode_attention_beam_fp8: R=%d rows are not a multiple of K=%d beams", a->R, a->K);
    VTGB_TRY(check_decode_attn({"llm_decode_attention_beam_fp8", "R", a->R, a->nq, a->nkv, a->hd, a->tmax_p, a->tmax_g},
                               {a->q, a->kp8, a->vp8, a->kg8, a->vg8, a->out, a->workspace}, {a->kps, a->vps, a->kgs, a->vgs, a->src_row},
                               "q / kp8 / vp8 / kg8 / vg8 / out / workspace need 16-byte, kps / vps / kgs / vgs / src_row 4-byte alignment"));
    hipStream_t s = (hipStream_t)stream;
    return a->hd == 128 ? launch_beam_fp8<128>(a, s) : launch_beam_fp8<64>(a, s);
}
