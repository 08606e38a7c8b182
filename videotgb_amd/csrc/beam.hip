// beam.hip -- the per-vocabulary half of one beam-search step (opt-in: beam_search="graph"): the logits [R = B * K, V] of the beam rows -> per
// batch item the 2 K best continuations (transformers' GenerationMixin._beam_search: log_softmax, RepetitionPenaltyLogitsProcessor and the
// eos block of the min-length processors on the log-probabilities, + the running beam scores, torch.topk over K * V).  Two launches:
//
// beam_row_kernel, one workgroup per beam row.  In fp32: m = max x, S = sum exp(x - m), lp = (x - m) - log S into the workspace row; then
// every DISTINCT id of seq[r, 0 .. *step) is penalised once (lp < 0 ? lp * p : lp / p), lp[eos] = -inf while *step < min_new (one id, or
// every id of a device list: vtgb_llm_beam_candidates_eos), and the row's
// 2 K best scores lp + running[r] are taken in descending order, equal scores in ascending token: every thread keeps the best of its own
// tokens (token % 256 == thread) that has not been taken, a round picks the workgroup's best and only its owner looks again.
// Which values share a partial sum and the order inside the sum depend on V alone (thread = token % 256, a thread's tokens ascending, then
// the lanes of a wave, then the four waves): a row's lp bits do not depend on B, K or the row's place.
//
// beam_merge_kernel, one workgroup per batch item: the K * 2 K row candidates -> rank of every candidate under (score descending, flat index
// k * V + token ascending) -- a total order, ranks are distinct --, ranks < 2 K written to cand_score / cand_idx.
#include "common.h"

#include <math.h>

#include <type_traits>

constexpr int BEAM_MAX_K = 16;
constexpr int BEAM_MAX_V = 1 << 20;
constexpr int BEAM_NO_TOKEN = 0x7fffffff;

__device__ __forceinline__ bool beam_better(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }

// the workgroup's best (value, index) under beam_better, on every thread
__device__ __forceinline__ void beam_block_best(float& v, int& i, float (*sv)[4], int (*si)[4], int slot) {
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(i, o);
        if (beam_better(ov, oi, v, i)) v = ov, i = oi;
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) sv[slot][wave] = v, si[slot][wave] = i;
    __syncthreads();
    v = sv[slot][0], i = si[slot][0];
#pragma unroll
    for (int w = 1; w < 4; w++)
        if (beam_better(sv[slot][w], si[slot][w], v, i)) v = sv[slot][w], i = si[slot][w];
}

// the eos operand of beam_row_kernel: one id by value (vtgb_llm_beam_candidates; < 0: none), or a device list (vtgb_llm_beam_candidates_eos).
// A second instantiation, not a branch: the one-id kernel's arguments and instructions are what they were before the list existed.
struct BeamEosList {
    const int* ids;
    int n;
};

template <typename T, typename E>
__global__ __launch_bounds__(256) void beam_row_kernel(const T* __restrict__ logits, const int64_t* __restrict__ seq, const int64_t* __restrict__ step_p,
                                                       const float* __restrict__ running, float* __restrict__ lp_ws, float* __restrict__ row_score,
                                                       int* __restrict__ row_idx, int K, int V, int N, E eos, int min_new, float penalty) {
    __shared__ float red[4];
    __shared__ float sv[2][4];
    __shared__ int si[2][4];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const T* x = logits + (int64_t)r * V;
    float* lp = lp_ws + (int64_t)r * V;
    const int64_t step64 = *step_p;
    const int step = (int)(step64 < 0 ? 0 : step64 > N ? N : step64);

    float m = -INFINITY;
    for (int v = tid; v < V; v += 256) m = fmaxf(m, (float)x[v]);
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float s = 0.f;
    for (int v = tid; v < V; v += 256) s += expf((float)x[v] - m);
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);      // (both lanes of a pair add the same two numbers)
    if (lane == 0) red[wave] = s;
    __syncthreads();
    const float lse = logf(((red[0] + red[1]) + red[2]) + red[3]);
    for (int v = tid; v < V; v += 256) lp[v] = ((float)x[v] - m) - lse;
    __syncthreads();      // lp (this workgroup's own global writes)

    if (penalty != 1.f) {      // (p == 1: lp * 1 and lp / 1 are lp)
        const int64_t* sq = seq + (int64_t)r * N;
        for (int j = tid; j < step; j += 256) {
            const int64_t id = sq[j];
            if (id < 0 || id >= V) continue;
            bool first = true;
            for (int j2 = 0; j2 < j; j2++) first = first && sq[j2] != id;
            if (first) {
                const float t = lp[id];
                lp[id] = t < 0.f ? t * penalty : t / penalty;
            }
        }
        __syncthreads();
    }
    if constexpr (std::is_same<E, int>::value) {
        if (eos >= 0 && eos < V && step64 < (int64_t)min_new) {
            if (tid == 0) lp[eos] = -INFINITY;
            __syncthreads();
        }
    } else {
        if (eos.n > 0 && step64 < (int64_t)min_new) {      // every listed id (a duplicate writes the same value twice)
            if (tid < eos.n) {
                const int id = eos.ids[tid];
                if (id >= 0 && id < V) lp[id] = -INFINITY;
            }
            __syncthreads();
        }
    }

    // ---- the row's 2 K best under (score descending, token ascending)
    const float run = running[r];
    auto scan = [&](float lastv, int lasti, float& bv, int& bi) {      // the thread's best token behind (lastv, lasti) in that order
        bv = -INFINITY, bi = BEAM_NO_TOKEN;
        for (int v = tid; v < V; v += 256) {
            const float t = lp[v] + run;
            if (lasti != BEAM_NO_TOKEN && !beam_better(lastv, lasti, t, v)) continue;      // taken before (or NaN)
            if (beam_better(t, v, bv, bi)) bv = t, bi = v;
        }
    };
    float bv;
    int bi;
    scan(0.f, BEAM_NO_TOKEN, bv, bi);
    const int k = r % K;
    for (int j = 0; j < 2 * K; j++) {
        float wv = bv;
        int wi = bi;
        beam_block_best(wv, wi, sv, si, j & 1);
        if (tid == 0) {
            const bool none = wi == BEAM_NO_TOKEN;      // (fewer than 2 K comparable scores: NaN logits, outside the contract)
            row_score[(int64_t)r * 2 * K + j] = none ? -INFINITY : wv;
            row_idx[(int64_t)r * 2 * K + j] = none ? k * V : k * V + wi;
        }
        if (wi != BEAM_NO_TOKEN && (wi & 255) == tid) scan(wv, wi, bv, bi);
    }
}

__global__ __launch_bounds__(512) void beam_merge_kernel(const float* __restrict__ row_score, const int* __restrict__ row_idx, float* __restrict__ cand_score,
                                                         int32_t* __restrict__ cand_idx, int K) {
    __shared__ float cs[2 * BEAM_MAX_K * BEAM_MAX_K];
    __shared__ int ci[2 * BEAM_MAX_K * BEAM_MAX_K];
    const int b = blockIdx.x, n = 2 * K * K, tid = threadIdx.x;
    if (tid < n) {
        cs[tid] = row_score[(int64_t)b * n + tid];
        ci[tid] = row_idx[(int64_t)b * n + tid];
    }
    __syncthreads();
    if (tid >= n) return;
    const float v = cs[tid];
    const int i = ci[tid];
    int rank = 0;
    for (int j = 0; j < n; j++) rank += (j != tid && (beam_better(cs[j], ci[j], v, i) || (cs[j] == v && ci[j] == i && j < tid))) ? 1 : 0;
    if (rank < 2 * K) {
        cand_score[(int64_t)b * 2 * K + rank] = v;
        cand_idx[(int64_t)b * 2 * K + rank] = i;
    }
}

template <typename E>
static int beam_candidates_launch(const vtgb_llm_beam_candidates_args* a, E eos, vtgb_stream_t stream) {
    VTGB_REQUIRE(a->logits && a->step && a->running && a->cand_score && a->cand_idx && a->workspace && (a->seq || a->N == 0), VTGB_EINVAL,
                 "llm_beam_candidates: NULL operand");
    VTGB_REQUIRE((a->dtype == VTGB_BF16 || a->dtype == VTGB_F32) && a->R > 0 && a->K > 0 && a->V > 0 && a->N >= 0 && a->penalty > 0.f, VTGB_EINVAL,
                 "llm_beam_candidates: bad argument");
    VTGB_REQUIRE(a->R % a->K == 0, VTGB_EINVAL, "llm_beam_candidates: R=%d rows are not a multiple of K=%d beams", a->R, a->K);
    VTGB_REQUIRE(a->K <= BEAM_MAX_K, VTGB_EUNSUPPORTED, "llm_beam_candidates: K=%d beams, built for up to %d", a->K, BEAM_MAX_K);
    VTGB_REQUIRE(a->V <= BEAM_MAX_V, VTGB_EUNSUPPORTED, "llm_beam_candidates: V=%d, built for up to %d", a->V, BEAM_MAX_V);
    VTGB_REQUIRE(2 * a->K <= a->V, VTGB_EUNSUPPORTED, "llm_beam_candidates: 2 K=%d candidates from V=%d tokens", 2 * a->K, a->V);
    const size_t lp_bytes = (size_t)a->R * a->V * sizeof(float), need = lp_bytes + (size_t)a->R * 2 * a->K * 8;
    VTGB_REQUIRE(a->workspace_bytes >= need && (reinterpret_cast<uintptr_t>(a->workspace) & 15) == 0, VTGB_EUNSUPPORTED,
                 "llm_beam_candidates: workspace of %zu bytes (16-byte aligned) needed, %zu given", need, a->workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
    float* lp = (float*)a->workspace;
    float* row_score = (float*)((char*)a->workspace + lp_bytes);
    int* row_idx = (int*)(row_score + (size_t)a->R * 2 * a->K);
    if (a->dtype == VTGB_BF16)
        hipLaunchKernelGGL((beam_row_kernel<bf16_t, E>), dim3(a->R), dim3(256), 0, s, (const bf16_t*)a->logits, a->seq, a->step, a->running, lp, row_score,
                           row_idx, a->K, a->V, a->N, eos, a->min_new, a->penalty);
    else
        hipLaunchKernelGGL((beam_row_kernel<float, E>), dim3(a->R), dim3(256), 0, s, (const float*)a->logits, a->seq, a->step, a->running, lp, row_score,
                           row_idx, a->K, a->V, a->N, eos, a->min_new, a->penalty);
    VTGB_HIP(hipGetLastError());
    hipLaunchKernelGGL(beam_merge_kernel, dim3(a->R / a->K), dim3(512), 0, s, (const float*)row_score, (const int*)row_idx, a->cand_score, a->cand_idx, a->K);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

extern "C" int vtgb_llm_beam_candidates(const vtgb_llm_beam_candidates_args* a, vtgb_stream_t stream) {
    VTGB_REQUIRE(a, VTGB_EINVAL, "llm_beam_candidates: NULL args");
    return beam_candidates_launch<int>(a, a->eos, stream);
}

// the same two launches with the list instantiation of beam_row_kernel; everything but the eos operand is checked by the shared launcher
extern "C" int vtgb_llm_beam_candidates_eos(const vtgb_llm_beam_candidates_eos_args* a, vtgb_stream_t stream) {
    VTGB_REQUIRE(a, VTGB_EINVAL, "llm_beam_candidates_eos: NULL args");
    VTGB_REQUIRE(a->n_eos >= 0 && a->n_eos <= VTGB_LLM_EOS_MAX, VTGB_EINVAL, "llm_beam_candidates_eos: n_eos=%d eos ids, 0 .. %d are taken", a->n_eos,
                 VTGB_LLM_EOS_MAX);
    VTGB_REQUIRE(a->eos_ids || a->n_eos == 0, VTGB_EINVAL, "llm_beam_candidates_eos: NULL operand");
    VTGB_REQUIRE((reinterpret_cast<uintptr_t>(a->eos_ids) & 3) == 0, VTGB_EUNSUPPORTED, "llm_beam_candidates_eos: eos_ids alignment (4 bytes)");
    vtgb_llm_beam_candidates_args c = {a->dtype, a->R, a->K, a->V, a->N, -1, a->min_new, a->penalty, a->logits, a->seq, a->step, a->running,
                                       a->cand_score, a->cand_idx, a->workspace, a->workspace_bytes};
    return beam_candidates_launch<BeamEosList>(&c, BeamEosList{a->eos_ids, a->n_eos}, stream);
}
