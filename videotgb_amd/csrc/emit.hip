// emit.hip -- the greedy emission of one decode step for a request with a SET of eos ids (opt-in: eos_sets="graph"): the logits [B, V] of the
// step -> the next token of every row, written to tok[b] and out[b, *step], and the row's finished flag.  One launch for what the captured
// step otherwise does in a chain of small torch ops (clone, masked write of the eos columns, argmax, two where, isin, logical_or_, copy_,
// index_copy_).
//
// pick_greedy_kernel, one workgroup per row.  Every thread keeps the best (value, index) of its own elements under (value descending, index
// ascending), then the lanes of a wave, then the four waves: the lowest index of the maximum, torch.argmax's rule, whatever the order the
// elements are visited in.  A row is read in three pieces: single elements up to the first 16-byte boundary, 16-byte loads, single elements
// behind the last whole 16 bytes -- rows of an odd V start 2 bytes off in bf16 and are never loaded wide from a misaligned address.
// While *step < min_new the listed ids count as -inf.  Thread 0 then applies the finished flag: a finished row emits pad and keeps its flag,
// another row's flag is set when its token is in the list.  An id outside [0, V) equals no index: it blocks nothing and ends nothing.
//
// repetition_penalty_kernel (opt-in: penalty_decode="graph"): HF's RepetitionPenaltyLogitsProcessor on one step's logits, for one-beam decoding.
// Grid (ceil(V / 8192), R): a workgroup owns one 8192-index chunk of one row.  It zeroes an 8 KB byte map of its chunk in LDS, marks the row's
// ids seq[r, 0 .. clamp(*step, 0, N)) and start_id that fall into the chunk with plain byte stores (duplicates store the same 1: no atomics,
// and the map is separate from the data, so "once whatever the repeats" holds by construction), and after a barrier streams the chunk:
// out = seen ? (x < 0 ? x * p : x / p) : x in fp32.  Loads follow pick_greedy_kernel's head / vector / tail split.
#include "common.h"

#include <math.h>

constexpr int PICK_NO_TOKEN = 0x7fffffff;

__device__ __forceinline__ bool pick_better(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }

template <typename T>
__global__ __launch_bounds__(256) void pick_greedy_kernel(const T* __restrict__ logits, const int64_t* __restrict__ step_p, const int* __restrict__ eos_ids,
                                                          uint8_t* __restrict__ fin, int64_t* __restrict__ tok, int64_t* __restrict__ out, int V, int N,
                                                          int n_eos, int min_new, int64_t pad) {
    constexpr int W = 16 / (int)sizeof(T);      // elements of one 16-byte load
    __shared__ float sv[4];
    __shared__ int si[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const T* x = logits + (int64_t)b * V;
    const int64_t step64 = *step_p;
    const bool blocked = n_eos > 0 && step64 < (int64_t)min_new;
    int eos[VTGB_LLM_EOS_MAX];      // (unrolled everywhere below: registers)
#pragma unroll
    for (int j = 0; j < VTGB_LLM_EOS_MAX; j++) eos[j] = j < n_eos ? eos_ids[j] : -1;      // (-1 equals no index)

    float bv = -INFINITY;
    int bi = PICK_NO_TOKEN;
    auto see = [&](float v, int i) {
        if (blocked) {
#pragma unroll
            for (int j = 0; j < VTGB_LLM_EOS_MAX; j++) v = eos[j] == i ? -INFINITY : v;
        }
        if (pick_better(v, i, bv, bi)) bv = v, bi = i;
    };
    // [0, head): up to the first 16-byte boundary; [head, head + W * nvec): whole aligned vectors; the rest single
    const uintptr_t addr = reinterpret_cast<uintptr_t>(x);
    int head = (int)(((16 - (addr & 15)) & 15) / sizeof(T));
    head = head < V ? head : V;
    const int nvec = (V - head) / W;
    for (int i = tid; i < head; i += 256) see((float)x[i], i);
    typedef T vec_t __attribute__((ext_vector_type(W)));
    const vec_t* xv = reinterpret_cast<const vec_t*>(x + head);
    for (int c = tid; c < nvec; c += 256) {
        const vec_t v = xv[c];
        const int i0 = head + c * W;
#pragma unroll
        for (int j = 0; j < W; j++) see((float)v[j], i0 + j);
    }
    for (int i = head + nvec * W + tid; i < V; i += 256) see((float)x[i], i);

    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (pick_better(ov, oi, bv, bi)) bv = ov, bi = oi;
    }
    if (lane == 0) sv[wave] = bv, si[wave] = bi;
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int w = 1; w < 4; w++)
        if (pick_better(sv[w], si[w], bv, bi)) bv = sv[w], bi = si[w];
    int64_t t = bi == PICK_NO_TOKEN ? 0 : bi;      // (no comparable value: NaN logits, outside the contract)
    if (fin[b]) {
        t = pad;
    } else {
        bool hit = false;
#pragma unroll
        for (int j = 0; j < VTGB_LLM_EOS_MAX; j++) hit = hit || (int64_t)eos[j] == t;
        if (hit) fin[b] = 1;
    }
    const int64_t col = step64 < 0 ? 0 : step64 > N - 1 ? N - 1 : step64;
    tok[b] = t;
    out[(int64_t)b * N + col] = t;
}

extern "C" int vtgb_llm_pick_greedy(const vtgb_llm_pick_greedy_args* a, vtgb_stream_t stream) {
    VTGB_REQUIRE(a, VTGB_EINVAL, "llm_pick_greedy: NULL args");
    VTGB_REQUIRE(a->logits && a->step && a->fin && a->tok && a->out && (a->eos_ids || a->n_eos == 0), VTGB_EINVAL, "llm_pick_greedy: NULL operand");
    VTGB_REQUIRE((a->dtype == VTGB_BF16 || a->dtype == VTGB_F32) && a->B > 0 && a->V > 0 && a->N > 0, VTGB_EINVAL, "llm_pick_greedy: bad argument");
    VTGB_REQUIRE(a->n_eos >= 0 && a->n_eos <= VTGB_LLM_EOS_MAX, VTGB_EINVAL, "llm_pick_greedy: n_eos=%d eos ids, 0 .. %d are taken", a->n_eos,
                 VTGB_LLM_EOS_MAX);
    auto at = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    VTGB_REQUIRE((at(a->logits) & 15) == 0 && (at(a->step) & 7) == 0 && (at(a->tok) & 7) == 0 && (at(a->out) & 7) == 0 && (at(a->eos_ids) & 3) == 0,
                 VTGB_EUNSUPPORTED, "llm_pick_greedy: operand alignment (logits 16 bytes; step, tok, out 8; eos_ids 4)");
    hipStream_t s = (hipStream_t)stream;
    if (a->dtype == VTGB_BF16)
        hipLaunchKernelGGL(pick_greedy_kernel<bf16_t>, dim3(a->B), dim3(256), 0, s, (const bf16_t*)a->logits, a->step, a->eos_ids, a->fin, a->tok, a->out,
                           a->V, a->N, a->n_eos, a->min_new, a->pad);
    else
        hipLaunchKernelGGL(pick_greedy_kernel<float>, dim3(a->B), dim3(256), 0, s, (const float*)a->logits, a->step, a->eos_ids, a->fin, a->tok, a->out,
                           a->V, a->N, a->n_eos, a->min_new, a->pad);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

constexpr int PEN_CHUNK = 8192;      // vocabulary indices per workgroup = bytes of its LDS map

template <typename T>
__global__ __launch_bounds__(256) void repetition_penalty_kernel(const T* __restrict__ logits, const int64_t* __restrict__ seq, const int64_t* __restrict__ step_p,
                                                                 float* __restrict__ out, int V, int N, float penalty, int start_id) {
    constexpr int W = 16 / (int)sizeof(T);      // elements of one 16-byte load
    __shared__ uint32_t seen32[PEN_CHUNK / 4];
    uint8_t* seen = reinterpret_cast<uint8_t*>(seen32);
    const int r = blockIdx.y, tid = threadIdx.x;
    const int c0 = blockIdx.x * PEN_CHUNK;
    const int len = V - c0 < PEN_CHUNK ? V - c0 : PEN_CHUNK;      // (> 0: the grid covers ceil(V / PEN_CHUNK) chunks)
    for (int i = tid; i < PEN_CHUNK / 4; i += 256) seen32[i] = 0u;
    __syncthreads();
    const int64_t step64 = *step_p;
    const int n = step64 < 0 ? 0 : step64 > N ? N : (int)step64;      // entries at or behind *step are never read
    const int64_t* ids = seq + (int64_t)r * N;
    for (int j = tid; j < n; j += 256) {
        const int64_t d = ids[j] - c0;      // an id outside [0, V) falls into no chunk
        if (d >= 0 && d < len) seen[d] = 1;
    }
    if (tid == 0 && start_id >= c0 && start_id - c0 < len) seen[start_id - c0] = 1;
    __syncthreads();

    const T* x = logits + (int64_t)r * V + c0;
    float* o = out + (int64_t)r * V + c0;
    auto pen = [&](float v, int i) { return seen[i] ? (v < 0.0f ? v * penalty : v / penalty) : v; };
    // [0, head): up to the first 16-byte boundary of the loads; [head, head + W * nvec): whole aligned vectors; the rest single
    int head = (int)(((16 - (reinterpret_cast<uintptr_t>(x) & 15)) & 15) / sizeof(T));
    head = head < len ? head : len;
    const int nvec = (len - head) / W;
    for (int i = tid; i < head; i += 256) o[i] = pen((float)x[i], i);
    typedef T vec_t __attribute__((ext_vector_type(W)));
    const vec_t* xv = reinterpret_cast<const vec_t*>(x + head);
    const bool wide = (reinterpret_cast<uintptr_t>(o + head) & 15) == 0;      // (uniform over the workgroup) the stores of a vector are 16-byte aligned too
    for (int c = tid; c < nvec; c += 256) {
        const vec_t v = xv[c];
        const int i0 = head + c * W;
        float y[W];
#pragma unroll
        for (int j = 0; j < W; j++) y[j] = pen((float)v[j], i0 + j);
        if (wide) {
#pragma unroll
            for (int j = 0; j < W; j += 4) *reinterpret_cast<float4*>(o + i0 + j) = make_float4(y[j], y[j + 1], y[j + 2], y[j + 3]);
        } else {
#pragma unroll
            for (int j = 0; j < W; j++) o[i0 + j] = y[j];
        }
    }
    for (int i = head + nvec * W + tid; i < len; i += 256) o[i] = pen((float)x[i], i);
}

extern "C" int vtgb_llm_repetition_penalty(const vtgb_llm_repetition_penalty_args* a, vtgb_stream_t stream) {
    VTGB_REQUIRE(a, VTGB_EINVAL, "llm_repetition_penalty: NULL args");
    VTGB_REQUIRE(a->logits && a->seq && a->step && a->out, VTGB_EINVAL, "llm_repetition_penalty: NULL operand");
    VTGB_REQUIRE((a->dtype == VTGB_BF16 || a->dtype == VTGB_F32) && a->R > 0 && a->V > 0 && a->N > 0, VTGB_EINVAL, "llm_repetition_penalty: bad argument");
    VTGB_REQUIRE(isfinite(a->penalty) && a->penalty > 0.0f, VTGB_EINVAL, "llm_repetition_penalty: penalty=%g, a finite positive number is taken",
                 (double)a->penalty);
    VTGB_REQUIRE(a->R <= 65535, VTGB_EUNSUPPORTED, "llm_repetition_penalty: R=%d rows, up to 65535 are taken", a->R);
    auto at = [](const void* p) { return reinterpret_cast<uintptr_t>(p); };
    VTGB_REQUIRE((at(a->logits) & 15) == 0 && (at(a->out) & 15) == 0 && (at(a->seq) & 7) == 0 && (at(a->step) & 7) == 0, VTGB_EUNSUPPORTED,
                 "llm_repetition_penalty: operand alignment (logits, out 16 bytes; seq, step 8)");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((a->V + PEN_CHUNK - 1) / PEN_CHUNK, a->R);
    if (a->dtype == VTGB_BF16)
        hipLaunchKernelGGL(repetition_penalty_kernel<bf16_t>, grid, dim3(256), 0, s, (const bf16_t*)a->logits, a->seq, a->step, a->out, a->V, a->N,
                           a->penalty, a->start_id);
    else
        hipLaunchKernelGGL(repetition_penalty_kernel<float>, grid, dim3(256), 0, s, (const float*)a->logits, a->seq, a->step, a->out, a->V, a->N,
                           a->penalty, a->start_id);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}
