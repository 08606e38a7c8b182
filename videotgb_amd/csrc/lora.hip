// lora.hip -- unmerged LoRA adapters on the language model's q / k / v projections (peft 0.4.0 tuners.lora.Linear in inference mode, as
// videotgb_amd.train.LoraLinear.forward states it): an in-place low-rank update of a projection's output,
//     y[m, col0 + j] = rnd(y[m, col0 + j] + rnd((sum_i B[j, i] * (sum_k A[i, k] * float(x[m, k]))) * scaling))        rnd = to y's dtype
// with fp32 adapters and fp32 accumulation, for up to four disjoint column segments of y (q | k | v of one fused projection) per launch.
//
// One kernel serves the decode step (<= 128 rows: launch latency and the A / B reads of a single workgroup are what cost) and the prefill
// (tens of thousands of rows).  A workgroup owns a tile of LORA_RT rows and a chunk of one segment's columns:
//   phase 1  t[m, i] = A[i, :] . x[m, :] for the tile's rows, EIGHT ranks at a time: thread `tid` adds k = 4 tid + {0, 1, 2, 3}, then the same
//            + 1024, + 2048, ... (in that order, one fmaf chain per (m, i)); the 64 lanes of a wave are added by an xor butterfly (32, 16, ..
//            1), the four waves in wave order.  A is read once per row tile (and column chunk), not once per row.
//   phase 2  u = fmaf chain over i = 0 .. r-1 of B[j, i] * t[m, i]; d = rnd(u * scaling); y = rnd(y + d).
// Every column chunk recomputes t: the host spreads the columns over workgroups until the grid fills the device, which changes nothing in
// the arithmetic.  The order of every sum depends on (K, r) alone -- not on rows, on which rows share a tile, or on the grid -- so a row's
// bits do not depend on the batch (tests/test_gpu_scale.py's rule).  No atomics, plain vector loads and stores, no matrix cores.
//
// vtgb_llm_lora_parts (llm_lora_parts_kernel, below) is the same update on a projection whose split-K reduce was deferred: it adds the
// vtgb_gemm_skinny fragments itself and writes y without reading it.  Both kernels call the same device functions for phase 1 and for
// phase 2's sum, so the two forms agree bit for bit.
#include "common.h"

#define LORA_RT 8        // rows per workgroup
#define LORA_RC 8        // ranks per pass over K
#define LORA_THREADS 256

template <typename T> struct LoraT;
template <> struct LoraT<float> {
    static __device__ __forceinline__ float rnd(float v) { return v; }
    static __device__ __forceinline__ void load4(const float* p, float (&o)[4]) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p);
        o[0] = v[0], o[1] = v[1], o[2] = v[2], o[3] = v[3];
    }
    static __device__ __forceinline__ float load(const float* p) { return *p; }
    static __device__ __forceinline__ void store(float* p, float v) { *p = v; }
};
template <> struct LoraT<bf16_t> {
    static __device__ __forceinline__ float rnd(float v) { return bf16_round(v); }
    static __device__ __forceinline__ void load4(const bf16_t* p, float (&o)[4]) {
        const bf16x4 v = *reinterpret_cast<const bf16x4*>(p);
        o[0] = (float)v[0], o[1] = (float)v[1], o[2] = (float)v[2], o[3] = (float)v[3];
    }
    static __device__ __forceinline__ float load(const bf16_t* p) { return (float)*p; }
    static __device__ __forceinline__ void store(bf16_t* p, float v) { *p = (bf16_t)v; }      // (v is a bf16 number already)
};

struct LoraLaunch {
    vtgb_llm_lora_args a;
    int32_t chunk_cols;          // columns per workgroup (a multiple of 64)
    int32_t chunk_first[5];      // blockIdx.y of segment s's first chunk; [n_seg] = the grid's y extent
};

// ---- phase 1 (both kernels): t_s[m][i] = A[i, :] . x[m, :] for the tile's nr rows, LORA_RC ranks per pass.  Ends behind a barrier.
template <typename T>
__device__ __forceinline__ void lora_phase1(const T* __restrict__ x, int64_t ldx, const float* __restrict__ A, int K, int r, int nr,
                                            float (&red)[LORA_THREADS / 64][LORA_RT][LORA_RC], float (&t_s)[LORA_RT][64]) {
#pragma clang fp contract(off)      // (the sums are explicit fmaf chains)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i0 = 0; i0 < r; i0 += LORA_RC) {
        const int ni = min(LORA_RC, r - i0);
        float acc[LORA_RT][LORA_RC];
#pragma unroll
        for (int m = 0; m < LORA_RT; m++)
#pragma unroll
            for (int i = 0; i < LORA_RC; i++) acc[m][i] = 0.f;
        for (int k = tid * 4; k < K; k += LORA_THREADS * 4) {
            float av[LORA_RC][4];
#pragma unroll
            for (int i = 0; i < LORA_RC; i++)
                if (i < ni) LoraT<float>::load4(A + (int64_t)(i0 + i) * K + k, av[i]);
#pragma unroll
            for (int m = 0; m < LORA_RT; m++) {
                if (m < nr) {      // (uniform over the workgroup)
                    float xv[4];
                    LoraT<T>::load4(x + (int64_t)m * ldx + k, xv);
#pragma unroll
                    for (int i = 0; i < LORA_RC; i++)
                        if (i < ni) {
#pragma unroll
                            for (int e = 0; e < 4; e++) acc[m][i] = fmaf(av[i][e], xv[e], acc[m][i]);
                        }
                }
            }
        }
#pragma unroll
        for (int m = 0; m < LORA_RT; m++)
#pragma unroll
            for (int i = 0; i < LORA_RC; i++) {
                float v = acc[m][i];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
                if (lane == 0) red[wave][m][i] = v;
            }
        __syncthreads();
        if (tid < LORA_RT * LORA_RC) {
            const int m = tid / LORA_RC, i = tid % LORA_RC;
            if (i < ni) t_s[m][i0 + i] = ((red[0][m][i] + red[1][m][i]) + red[2][m][i]) + red[3][m][i];
        }
        __syncthreads();
    }
}

// ---- phase 2's sum (both kernels): u[m] = fmaf chain over i = 0 .. r-1 of B[j, i] * t[m, i]
__device__ __forceinline__ void lora_u(const float* __restrict__ bj, int r, const float (&t_s)[LORA_RT][64], float (&u)[LORA_RT]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int m = 0; m < LORA_RT; m++) u[m] = 0.f;
    for (int i = 0; i < r; i++) {
        const float b = bj[i];
#pragma unroll
        for (int m = 0; m < LORA_RT; m++) u[m] = fmaf(b, t_s[m][i], u[m]);      // (rows >= nr: stale t, never stored)
    }
}

template <typename T>
__global__ __launch_bounds__(LORA_THREADS) void llm_lora_kernel(const LoraLaunch p) {
#pragma clang fp contract(off)      // (u * scaling and y + d are single operations)
    __shared__ float red[LORA_THREADS / 64][LORA_RT][LORA_RC];
    __shared__ float t_s[LORA_RT][64];
    const vtgb_llm_lora_args& a = p.a;
    const int tid = threadIdx.x;
    int s = 0;
    while (s + 1 < a.n_seg && (int)blockIdx.y >= p.chunk_first[s + 1]) s++;
    const vtgb_llm_lora_seg sg = a.seg[s];
    const int c_beg = ((int)blockIdx.y - p.chunk_first[s]) * p.chunk_cols;
    const int c_end = min(c_beg + p.chunk_cols, sg.n);
    const int64_t row0 = (int64_t)blockIdx.x * LORA_RT;
    const int nr = (int)min((int64_t)LORA_RT, a.rows - row0);      // rows of this tile: 1 .. LORA_RT
    const int r = sg.r;
    lora_phase1<T>((const T*)a.x + row0 * a.ldx, a.ldx, sg.A, a.K, r, nr, red, t_s);

    // ---- phase 2: the tile's rows x this chunk's columns
    T* __restrict__ y = (T*)a.y + row0 * a.ldy + sg.col0;
    const float* __restrict__ Bw = sg.B;
    const float scaling = sg.scaling;
    for (int j = c_beg + tid; j < c_end; j += LORA_THREADS) {
        float u[LORA_RT];
        lora_u(Bw + (int64_t)j * r, r, t_s, u);
#pragma unroll
        for (int m = 0; m < LORA_RT; m++) {
            if (m < nr) {
                T* yp = y + (int64_t)m * a.ldy + j;
                const float d = LoraT<T>::rnd(u[m] * scaling);
                LoraT<T>::store(yp, LoraT<T>::rnd(LoraT<T>::load(yp) + d));
            }
        }
    }
}

// ---- vtgb_llm_lora_parts: the K-split reduce of a deferred vtgb_gemm_skinny projection and the update, in one launch (bf16, rows <= 128).
// y's columns are cut into PIECES -- the segments and the gaps between them, in column order -- and every piece into chunks of chunk_cols
// columns; a workgroup owns LORA_RT rows x one chunk.  base = rnd(0 + part[split 0] + part[split 1] + ...) is gemm_skinny_reduce_kernel's
// sum; a gap chunk stores it, a segment chunk runs llm_lora_kernel's phase 1 and stores rnd(base + rnd(u * scaling)).  y is never read.
#define LORA_MAX_PIECES (2 * VTGB_LORA_MAX_SEGMENTS + 1)
struct LoraPartsLaunch {
    vtgb_llm_lora_args a;
    const float* part;
    int32_t n_splits, chunk_cols, n_piece;
    int32_t piece_col0[LORA_MAX_PIECES], piece_n[LORA_MAX_PIECES], piece_seg[LORA_MAX_PIECES];      // piece_seg: the segment, or -1 for a gap
    int32_t chunk_first[LORA_MAX_PIECES + 1];      // blockIdx.y of piece q's first chunk; [n_piece] = the grid's y extent
};

// the reduce launch's value of column c (tile c / 128) of row m: fragments added in split order onto 0, one rounding to bf16
__device__ __forceinline__ float lora_parts_base(const float* __restrict__ part, int S, int M, int64_t m, int c) {
    const float* p = part + ((int64_t)(c >> 7) * S * M + m) * 128 + (c & 127);
    float v = 0.f;
    for (int sp = 0; sp < S; sp++) v += p[(int64_t)sp * M * 128];
    return bf16_round(v);
}

__global__ __launch_bounds__(LORA_THREADS) void llm_lora_parts_kernel(const LoraPartsLaunch p) {
#pragma clang fp contract(off)
    __shared__ float red[LORA_THREADS / 64][LORA_RT][LORA_RC];
    __shared__ float t_s[LORA_RT][64];
    const vtgb_llm_lora_args& a = p.a;
    const int tid = threadIdx.x;
    int q = 0;
    while (q + 1 < p.n_piece && (int)blockIdx.y >= p.chunk_first[q + 1]) q++;
    const int c_beg = ((int)blockIdx.y - p.chunk_first[q]) * p.chunk_cols;
    const int c_end = min(c_beg + p.chunk_cols, p.piece_n[q]);
    const int col0 = p.piece_col0[q];
    const int64_t row0 = (int64_t)blockIdx.x * LORA_RT;
    const int nr = (int)min((int64_t)LORA_RT, a.rows - row0), M = (int)a.rows, S = p.n_splits;
    bf16_t* __restrict__ y = (bf16_t*)a.y + row0 * a.ldy + col0;
    if (p.piece_seg[q] < 0) {      // a gap (uniform over the workgroup): the plain reduce
        for (int j = c_beg + tid; j < c_end; j += LORA_THREADS)
            for (int m = 0; m < nr; m++) y[(int64_t)m * a.ldy + j] = (bf16_t)lora_parts_base(p.part, S, M, row0 + m, col0 + j);
        return;
    }
    const vtgb_llm_lora_seg sg = a.seg[p.piece_seg[q]];
    const int r = sg.r;
    lora_phase1<bf16_t>((const bf16_t*)a.x + row0 * a.ldx, a.ldx, sg.A, a.K, r, nr, red, t_s);
    const float scaling = sg.scaling;
    for (int j = c_beg + tid; j < c_end; j += LORA_THREADS) {
        float u[LORA_RT];
        lora_u(sg.B + (int64_t)j * r, r, t_s, u);
#pragma unroll
        for (int m = 0; m < LORA_RT; m++) {
            if (m < nr) {
                const float d = bf16_round(u[m] * scaling);
                y[(int64_t)m * a.ldy + j] = (bf16_t)bf16_round(lora_parts_base(p.part, S, M, row0 + m, col0 + j) + d);
            }
        }
    }
}

// the argument checks of both entry points; *total = the segments' columns
static int lora_check(const vtgb_llm_lora_args* a, int64_t* total_out) {
    VTGB_REQUIRE(a, VTGB_EINVAL, "llm_lora: NULL args");
    VTGB_REQUIRE(a->dtype == VTGB_BF16 || a->dtype == VTGB_F32, VTGB_EINVAL, "llm_lora: dtype %d (VTGB_F32 or VTGB_BF16)", a->dtype);
    VTGB_REQUIRE(a->x && a->y, VTGB_EINVAL, "llm_lora: NULL x or y");
    VTGB_REQUIRE(a->n_seg >= 1 && a->n_seg <= VTGB_LORA_MAX_SEGMENTS, VTGB_EINVAL, "llm_lora: n_seg=%d outside 1..%d", a->n_seg, VTGB_LORA_MAX_SEGMENTS);
    VTGB_REQUIRE(a->rows > 0 && a->rows <= (int64_t)LORA_RT * 0x7FFFFFFF && a->K > 0 && a->n_cols > 0, VTGB_EINVAL,
                 "llm_lora: rows=%lld K=%d n_cols=%d must be positive", (long long)a->rows, a->K, a->n_cols);
    VTGB_REQUIRE(a->ldx >= a->K && a->ldy >= a->n_cols, VTGB_EINVAL, "llm_lora: row stride below the width (ldx=%lld K=%d, ldy=%lld n_cols=%d)",
                 (long long)a->ldx, a->K, (long long)a->ldy, a->n_cols);
    const size_t es = dtype_size(a->dtype);
    int64_t total = 0;
    for (int s = 0; s < a->n_seg; s++) {
        const vtgb_llm_lora_seg& g = a->seg[s];
        VTGB_REQUIRE(g.A && g.B, VTGB_EINVAL, "llm_lora: segment %d: NULL A or B", s);
        VTGB_REQUIRE(g.r >= 1 && g.r <= VTGB_LORA_MAX_RANK, VTGB_EINVAL, "llm_lora: segment %d: r=%d outside 1..%d", s, g.r, VTGB_LORA_MAX_RANK);
        VTGB_REQUIRE(g.n >= 1 && g.col0 >= 0 && (int64_t)g.col0 + g.n <= a->n_cols, VTGB_EINVAL,
                     "llm_lora: segment %d: columns [%d, %lld) past y's %d columns", s, g.col0, (long long)g.col0 + g.n, a->n_cols);
        for (int q = 0; q < s; q++)
            VTGB_REQUIRE(g.col0 >= a->seg[q].col0 + a->seg[q].n || a->seg[q].col0 >= g.col0 + g.n, VTGB_EINVAL,
                         "llm_lora: segments %d and %d overlap", q, s);
        VTGB_REQUIRE((uintptr_t)g.A % 16 == 0 && (uintptr_t)g.B % 4 == 0, VTGB_EUNSUPPORTED,
                     "llm_lora: segment %d: A must be 16-byte and B 4-byte aligned", s);
        total += g.n;
    }
    // phase 1 reads four consecutive k per lane
    VTGB_REQUIRE(a->K % 4 == 0 && a->ldx % 4 == 0, VTGB_EUNSUPPORTED, "llm_lora: K=%d and ldx=%lld must be multiples of 4", a->K, (long long)a->ldx);
    VTGB_REQUIRE((uintptr_t)a->x % (4 * es) == 0 && (uintptr_t)a->y % es == 0, VTGB_EUNSUPPORTED,
                 "llm_lora: x must be aligned to four elements and y to one");
    *total_out = total;
    return VTGB_OK;
}

// columns per workgroup over `total` columns: enough workgroups to fill the device at the decode step, one chunk per segment at the prefill
static int32_t lora_chunk_cols(int64_t total, int64_t row_tiles) {
    const int64_t want = (4 * (int64_t)cu_count() + row_tiles - 1) / row_tiles;
    int64_t cc = (total + want - 1) / want;
    cc = (cc + 127) / 128 * 128;
    return (int32_t)(cc > 0x40000000 ? 0x40000000 : cc);
}

extern "C" int vtgb_llm_lora(const vtgb_llm_lora_args* a, vtgb_stream_t stream) {
    int64_t total = 0;
    VTGB_TRY(lora_check(a, &total));
    LoraLaunch p;
    p.a = *a;
    const int64_t row_tiles = (a->rows + LORA_RT - 1) / LORA_RT;
    p.chunk_cols = lora_chunk_cols(total, row_tiles);
    int32_t first = 0;
    for (int s = 0; s < a->n_seg; s++) {
        p.chunk_first[s] = first;
        first += (a->seg[s].n + p.chunk_cols - 1) / p.chunk_cols;
    }
    for (int s = a->n_seg; s <= VTGB_LORA_MAX_SEGMENTS; s++) p.chunk_first[s] = first;
    VTGB_REQUIRE(first <= 65535, VTGB_EUNSUPPORTED, "llm_lora: %d column chunks", first);
    const dim3 grid((unsigned)row_tiles, (unsigned)first);
    if (a->dtype == VTGB_BF16)
        hipLaunchKernelGGL(llm_lora_kernel<bf16_t>, grid, dim3(LORA_THREADS), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(llm_lora_kernel<float>, grid, dim3(LORA_THREADS), 0, (hipStream_t)stream, p);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}

extern "C" int vtgb_llm_lora_parts(const vtgb_llm_lora_args* a, const float* part, int32_t n_splits, vtgb_stream_t stream) {
    int64_t total = 0;
    VTGB_TRY(lora_check(a, &total));
    VTGB_REQUIRE(a->dtype == VTGB_BF16, VTGB_EINVAL, "llm_lora_parts: dtype %d (VTGB_BF16: the fragments of a bf16 projection)", a->dtype);
    VTGB_REQUIRE(a->rows <= 128, VTGB_EINVAL, "llm_lora_parts: rows=%lld (<= 128, vtgb_gemm_skinny's M)", (long long)a->rows);
    VTGB_REQUIRE(n_splits >= 2 && n_splits <= 64, VTGB_EINVAL, "llm_lora_parts: n_splits=%d outside 2..64", n_splits);
    VTGB_REQUIRE(part, VTGB_EINVAL, "llm_lora_parts: NULL part");
    VTGB_REQUIRE((uintptr_t)part % 4 == 0, VTGB_EUNSUPPORTED, "llm_lora_parts: part must be 4-byte aligned");

    LoraPartsLaunch p;
    p.a = *a;
    p.part = part;
    p.n_splits = n_splits;
    const int64_t row_tiles = (a->rows + LORA_RT - 1) / LORA_RT;
    p.chunk_cols = lora_chunk_cols(a->n_cols, row_tiles);
    // the pieces: segments by column (they are disjoint), a gap wherever the next one starts behind the last one's end
    int order[VTGB_LORA_MAX_SEGMENTS];
    for (int s = 0; s < a->n_seg; s++) {
        int q = s;
        for (; q > 0 && a->seg[order[q - 1]].col0 > a->seg[s].col0; q--) order[q] = order[q - 1];
        order[q] = s;
    }
    int32_t first = 0, col = 0;
    p.n_piece = 0;
    const auto piece = [&](int32_t col0, int32_t n, int32_t seg) {
        p.piece_col0[p.n_piece] = col0, p.piece_n[p.n_piece] = n, p.piece_seg[p.n_piece] = seg;
        p.chunk_first[p.n_piece++] = first;
        first += (n + p.chunk_cols - 1) / p.chunk_cols;
    };
    for (int s = 0; s < a->n_seg; s++) {
        const vtgb_llm_lora_seg& g = a->seg[order[s]];
        if (g.col0 > col) piece(col, g.col0 - col, -1);
        piece(g.col0, g.n, order[s]);
        col = g.col0 + g.n;
    }
    if (a->n_cols > col) piece(col, a->n_cols - col, -1);
    for (int q = p.n_piece; q < LORA_MAX_PIECES; q++) p.piece_col0[q] = p.piece_n[q] = 0, p.piece_seg[q] = -1;
    for (int q = p.n_piece; q <= LORA_MAX_PIECES; q++) p.chunk_first[q] = first;
    VTGB_REQUIRE(first <= 65535, VTGB_EUNSUPPORTED, "llm_lora_parts: %d column chunks", first);
    hipLaunchKernelGGL(llm_lora_parts_kernel, dim3((unsigned)row_tiles, (unsigned)first), dim3(LORA_THREADS), 0, (hipStream_t)stream, p);
    VTGB_HIP(hipGetLastError());
    return VTGB_OK;
}
