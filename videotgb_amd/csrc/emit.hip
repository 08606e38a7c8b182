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
