"""The GEMM reference harness (tests/gemm_ref.py) checked on the CPU with a stand-in for the kernel: torch's fp32 matmul on the strided views.

(a) the bound accepts the correct stand-in in every epilogue at K = 64, 1408 and 11008, and fp32 accumulation of bf16-valued operands stays more
    than 10 x inside its accumulator term;
(b) the bound rejects each planted fault on >= 99 % of the elements the fault touches.  The 99 % is a condition: where a fault hides behind the
    bf16 OUTPUT rounding (2**-8 |ref|, which no test of a bf16 store can see below), the case says so and uses the inputs at which it cannot hide;
(c) run_gemm's own guards fire: writes outside out[:M, :N], reads of poison, elements never written."""
import pytest
import torch
import torch.nn.functional as F

import gemm_ref as R
from gemm_ref import EPI_GELU, EPI_RESID_F32, EPI_STORE, EPI_STORE_F32

ALL_EPI = [EPI_STORE, EPI_GELU, EPI_RESID_F32, EPI_STORE_F32]
F32_EPI = [EPI_RESID_F32, EPI_STORE_F32]


def test_epilogue_codes_match_the_library():
    from videotgb_amd import _lib as L
    assert (L.EPI_STORE, L.EPI_GELU, L.EPI_RESID_F32, L.EPI_STORE_F32) == (EPI_STORE, EPI_GELU, EPI_RESID_F32, EPI_STORE_F32)
    assert (L.BF16, L.F32) == (R.DT_BF16, R.DT_F32)


def operands(M, N, K, seed, bias=True, dtype=torch.bfloat16):
    """The distribution of the device tests: A ~ N(0, 1), W ~ 0.05 N(0, 1), bias and residual ~ N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g).to(dtype)
    W = (torch.randn(N, K, generator=g) * 0.05).to(dtype)
    b = torch.randn(N, generator=g) if bias else None
    r = torch.randn(M, N, generator=g)
    return A, W, b, r


def run(A, W, b, r, epi, kernel=R.standin_gemm, **kw):
    return R.run_gemm(A, W, b, epi, r if epi == EPI_RESID_F32 else None, kernel=kernel, **kw)


# ----------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("K", [64, 1408, 11008])
@pytest.mark.parametrize("epi", ALL_EPI, ids=lambda e: R.EPI_NAMES[e])
def test_bound_accepts_the_correct_standin(K, epi):
    A, W, b, r = operands(300, 200, K, seed=K + epi)
    for bias in (b, None):
        for kw in ({}, dict(a_off=8, a_pad=16, w_off=64, w_pad=64, o_pad=6), dict(inplace=True) if epi == EPI_RESID_F32 else dict(o_pad=2)):
            res = run(A, W, bias, r, epi, **kw)
            ex = R.excess(res)
            print(f"[standin {R.EPI_NAMES[epi]} K={K} bias={bias is not None} {kw}] max excess {ex.max().item():.3f}")
            assert ex.max() <= 1.0


@pytest.mark.parametrize("K", [64, 320, 1408, 4096, 6144, 11008])
def test_fp32_accumulation_is_ten_times_inside_the_accumulator_term(K):
    """torch's own fp32 order and a strict 32-deep chunked order (one MFMA's depth at a time, sequentially): both <= 2e-7 * sum |a||w|."""
    A, W, _, _ = operands(96, 80, K, seed=K)
    ref = R.ref64(A, W)
    s = A.double().abs() @ W.double().abs().t()
    own = A.float() @ W.float().t()
    chunked = torch.zeros(96, 80)
    for k0 in range(0, K, 32):
        chunked = chunked + A[:, k0:k0 + 32].float() @ W[:, k0:k0 + 32].float().t()
    for name, got in (("torch", own), ("32-deep", chunked)):
        ratio = ((got.double() - ref).abs() / s).max().item()
        print(f"[fp32 accumulation K={K} {name}] max |err| / sum|a||w| = {ratio:.3e}")
        assert ratio <= R.ACC_REL / 10


def test_gelu_lipschitz_constant():
    x = torch.linspace(-10, 10, 2_000_001, dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(F.gelu(x).sum(), x)
    assert 1.12 < g.abs().max().item() <= R.GELU_LIP


# ----------------------------------------------------------------------------- (b) planted faults
def faulty(fault):
    """A stand-in kernel with one fault planted, and the mask of the elements it touches."""
    def kernel(code, M, N, K, epi, A, lda, W, ldw, bias, resid, out, ldo):
        A32, W32 = A.float(), W.float()
        if fault == "dropped_k_tile":
            acc = A32[:, :K - 64] @ W32[:, :K - 64].t()
        else:
            acc = A32 @ W32.t()
        if fault == "rows_swapped":          # rows 37 and 201 of the second 256-row tile
            acc[[256 + 37, 256 + 201]] = acc[[256 + 201, 256 + 37]]
        if fault == "block_transposed":      # the 16 x 16 accumulator block at (272, 48)
            acc[272:288, 48:64] = acc[272:288, 48:64].t().clone()
        if bias is not None:
            acc = acc + (torch.roll(bias, -4) if fault == "bias_shifted" else bias)
        if epi == EPI_RESID_F32:
            acc = acc + (torch.roll(resid, -1, 0) if fault == "resid_wrong_row" else resid)
        if epi == EPI_GELU:
            acc = F.gelu(acc)
        out.copy_(acc.to(out.dtype))
    return kernel


def touched(fault, M, N):
    t = torch.zeros(M, N, dtype=torch.bool)
    if fault == "rows_swapped":
        t[[256 + 37, 256 + 201]] = True
    elif fault == "block_transposed":
        t[272:288, 48:64] = ~torch.eye(16, dtype=torch.bool)      # (the diagonal of a transposed block stays where it was)
    else:
        t[:] = True
    return t


# Where each fault is planted.  A bf16 store cannot show a difference below 2**-8 |ref|: a fault whose effect d has spread sd is missed on about
# 2 * 2**-8 E|ref| / (sqrt(2 pi) sd) of its elements.  Row swaps, transposition and the bias shift move an element by sd ~ 1.4 x its own spread
# (0.2 ... 0.5 % missed: inside the condition); a dropped 64-deep k-tile moves it by 0.05 * 8 = 0.4 whatever K is, so behind a bf16 store it is
# planted at K = 128 without bias (E|ref| = 0.45: 0.35 %), where at K = 11008 (E|ref| = 4.2) 3 % would hide: the depth K = 11008 is checked at
# the fp32 epilogues, where the bound is the accumulator term alone (7e-4 against 0.4: < 0.2 %).  GELU maps everything below -3.7 to less than
# 1e-4, where no fault shows: the bias shift is planted under it at K = 64 (pre-activations ~ N(0, 1.1): 0.03 % down there), not at K = 1408 (~ N(0,
# 2.1): 4 %).
FAULT_CASES = [
    ("dropped_k_tile", 11008, EPI_STORE_F32, True), ("dropped_k_tile", 11008, EPI_RESID_F32, True), ("dropped_k_tile", 1408, EPI_STORE_F32, False),
    ("dropped_k_tile", 128, EPI_STORE, False), ("dropped_k_tile", 128, EPI_GELU, False),
    ("rows_swapped", 64, EPI_STORE_F32, True), ("rows_swapped", 1408, EPI_STORE, True), ("rows_swapped", 1408, EPI_GELU, False),
    ("rows_swapped", 64, EPI_RESID_F32, True),
    ("bias_shifted", 64, EPI_STORE_F32, True), ("bias_shifted", 64, EPI_STORE, True), ("bias_shifted", 64, EPI_GELU, True),
    ("bias_shifted", 64, EPI_RESID_F32, True),
    ("block_transposed", 64, EPI_STORE_F32, True), ("block_transposed", 64, EPI_RESID_F32, False), ("block_transposed", 1408, EPI_STORE, False),
    ("resid_wrong_row", 64, EPI_RESID_F32, True), ("resid_wrong_row", 11008, EPI_RESID_F32, False),
]


@pytest.mark.parametrize("fault,K,epi,bias", FAULT_CASES, ids=[f"{f}-K{k}-{R.EPI_NAMES[e]}-{'bias' if b else 'nobias'}" for f, k, e, b in FAULT_CASES])
def test_bound_rejects_planted_fault(fault, K, epi, bias):
    M, N = 600, 2048 if fault == "rows_swapped" else 320      # (two rows are few elements: wide rows, so that 1 % of them is a number)
    A, W, b, r = operands(M, N, K, seed=7 * K + epi, bias=bias)
    assert R.excess(run(A, W, b, r, epi, o_pad=8)).max() <= 1.0          # the same inputs pass without the fault
    ex = R.excess(run(A, W, b, r, epi, kernel=faulty(fault), o_pad=8))
    t = touched(fault, M, N)
    rejected = (ex[t] > 1.0).double().mean().item()
    print(f"[{fault} K={K} {R.EPI_NAMES[epi]}] rejected on {100 * rejected:.2f} % of {int(t.sum())} touched elements; untouched max excess "
          f"{ex[~t].max().item() if (~t).any() else 0.0:.3f}")
    assert rejected >= 0.99
    assert not (~t).any() or ex[~t].max() <= 1.0


# ----------------------------------------------------------------------------- (c) the guards
def test_guards_catch_stray_writes_poison_reads_and_unwritten_elements():
    A, W, b, r = operands(40, 24, 64, seed=1)

    def writes_pad(code, M, N, K, epi, A, lda, W, ldw, bias, resid, out, ldo):
        R.standin_gemm(code, M, N, K, epi, A, lda, W, ldw, bias, resid, out, ldo)
        out.as_strided((M, ldo), (ldo, 1))[3, N] = 0.0

    def writes_behind(code, M, N, K, epi, A, lda, W, ldw, bias, resid, out, ldo):
        R.standin_gemm(code, M, N, K, epi, A, lda, W, ldw, bias, resid, out, ldo)
        out.as_strided((M + 1, N), (ldo, 1))[M, 0] = 0.0

    def reads_pad(code, M, N, K, epi, A, lda, W, ldw, bias, resid, out, ldo):
        R.standin_gemm(code, M, N, K, epi, A.as_strided((M, K), (lda, 1), A.storage_offset() + 1), lda, W, ldw, bias, resid, out, ldo)

    def reads_behind_w(code, M, N, K, epi, A, lda, W, ldw, bias, resid, out, ldo):
        R.standin_gemm(code, M, N, K, epi, A, lda, W.as_strided((N, K), (ldw, 1), W.storage_offset() + ldw), ldw, bias, resid, out, ldo)

    def skips_a_row(code, M, N, K, epi, A, lda, W, ldw, bias, resid, out, ldo):
        R.standin_gemm(code, M - 1, N, K, epi, A[:-1], lda, W, ldw, bias, resid, out[:-1], ldo)

    for epi in (EPI_STORE, EPI_STORE_F32):
        run(A, W, b, r, epi, a_pad=8, w_pad=8, o_pad=2)
        for k, msg in ((writes_pad, "pad columns"), (writes_behind, "behind row"), (reads_pad, "NaN"), (reads_behind_w, "NaN"), (skips_a_row, "unwritten")):
            with pytest.raises(AssertionError, match=msg):
                run(A, W, b, r, epi, a_pad=8, w_pad=8, o_pad=2, kernel=k)
