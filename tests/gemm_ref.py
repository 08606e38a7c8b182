"""Reference harness for vtgb_gemm (tests/test_gemm_ref.py checks it on the CPU, tests/test_gpu_gemm_large.py uses it on the device).

run_gemm   calls vtgb_gemm (or a stand-in with the same signature) on operands that are views into larger, poisoned buffers, with
           lda / ldw / ldo of the caller's choice, and checks the guards afterwards
ref64      the same operation in float64 from the operands as stored
bound      the element-wise error a correct kernel may show against ref64
kernels_run  the names of the device kernels a call launched (torch.profiler)

The bound.  Products of bf16 values are exact in fp32, so an fp32-accumulating kernel differs from float64 by its summation order only:
2e-6 * (|A| @ |W|^T + |bias| + |resid| + 1), the figure tests/test_gpu_train.py::test_gemm_train_reads_operands_in_place uses.  fp32 accumulation
of bf16-valued operands -- torch's own order and a strict 32-deep chunked order -- measures <= 1.4e-7 * sum |a||w| against float64 for K = 64 ...
11008 (test_gemm_ref.py asserts the torch figure), more than 10 x inside.  The bf16 epilogues add 2**-8 * |ref| for the output rounding (8
significant bits: half an ulp is 2**-8 of the value at the bottom of a binade); GELU is 1-Lipschitz up to 1.13 (max |gelu'| = 1.129 at x = 1.41),
so the accumulator term carries through it multiplied by 1.13."""
import ctypes as C
from dataclasses import dataclass
from typing import Callable, List, Optional

import torch
import torch.nn.functional as F

EPI_STORE, EPI_GELU, EPI_RESID_F32, EPI_STORE_F32 = 0, 1, 2, 3       # videotgb_amd._lib's codes (asserted in test_gemm_ref.py)
EPI_NAMES = {EPI_STORE: "store", EPI_GELU: "gelu", EPI_RESID_F32: "resid_f32", EPI_STORE_F32: "store_f32"}
DT_F32, DT_BF16 = 0, 1                                                  # videotgb_amd._lib.F32 / BF16
GUARD_ROWS = 256                                                       # rows behind every matrix: one whole tile of the largest kernel
ACC_REL = 2e-6
OUT_REL = 2.0 ** -8
GELU_LIP = 1.13
_PATTERN = {2: 0x5A5B, 4: 0x5A5B5C5D}                                  # the guard bit pattern of `out` per element size
_INT = {2: torch.int16, 4: torch.int32}


@dataclass
class GemmRun:
    """What one run_gemm call saw: the operand views as stored, the residual as it was BEFORE the call, and out[:M, :N]."""
    A: torch.Tensor
    W: torch.Tensor
    bias: Optional[torch.Tensor]
    resid: Optional[torch.Tensor]
    out: torch.Tensor
    epilogue: int
    lda: int
    ldw: int
    ldo: int


def lib_gemm(code, M, N, K, epilogue, A, lda, W, ldw, bias, resid, out, ldo):
    """The production entry: vtgb_gemm through the C ABI on the current stream."""
    from videotgb_amd import _lib as L
    a = L.GemmArgs(code, M, N, K, epilogue, A.data_ptr(), lda, W.data_ptr(), ldw, None if bias is None else bias.data_ptr(),
                   None if resid is None else resid.data_ptr(), out.data_ptr(), ldo)
    L.check(L.lib().vtgb_gemm(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)))


def standin_gemm(code, M, N, K, epilogue, A, lda, W, ldw, bias, resid, out, ldo):
    """CPU stand-in with vtgb_gemm's signature: torch's fp32 matmul on the strided views, the epilogue in fp32, one rounding to the output type.
    (resid has out's leading dimension, as in the C ABI; in place when it is out itself.)"""
    acc = A.float() @ W.float().t()
    if bias is not None:
        acc = acc + bias
    if epilogue == EPI_RESID_F32:
        acc = acc + resid
    if epilogue == EPI_GELU:
        acc = F.gelu(acc)
    out.copy_(acc.to(out.dtype))


def _poisoned(rows, cols, dtype, device):
    return torch.full((rows, cols), float("nan"), dtype=dtype, device=device)


def _patterned(rows, cols, dtype, device):
    es = torch.empty((), dtype=dtype).element_size()
    return torch.full((rows, cols), _PATTERN[es], dtype=_INT[es], device=device).view(dtype)


def run_gemm(A: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], epilogue: int, resid: Optional[torch.Tensor] = None, *,
             inplace: bool = False, a_off: int = 0, a_pad: int = 0, w_off: int = 0, w_pad: int = 0, o_pad: int = 0,
             kernel: Callable = None) -> GemmRun:
    """out[:M, :N] = epilogue(A @ W^T + bias (+ resid)) by `kernel` (default: vtgb_gemm), A [M, K] and W [N, K] in bf16 or fp32.

    A is stored as columns a_off .. a_off + K of a [M + 256, K + a_pad] buffer (lda = K + a_pad), W likewise, out as the first N columns of a
    [M + 256, N + o_pad] buffer (ldo = N + o_pad); the residual has out's layout (the C ABI gives it out's leading dimension), or IS out with
    inplace=True.  Everything outside the views is poison: NaN behind row M - 1 of A, behind row N - 1 of W and in their pad columns (and the
    residual's), a fixed bit pattern in out's pad columns and in the 256 rows behind it.  After the call the pattern must be unchanged, compared
    as integers, and out[:M, :N] must hold no NaN (and no trace of the pattern where the kernel had to write)."""
    kernel = kernel or lib_gemm
    dev, dt = A.device, A.dtype
    assert dt in (torch.bfloat16, torch.float32) and W.dtype == dt and A.dim() == 2 and W.dim() == 2
    M, K = A.shape
    N = W.shape[0]
    assert W.shape[1] == K and 0 <= a_off <= a_pad and 0 <= w_off <= w_pad
    lda, ldw, ldo = K + a_pad, K + w_pad, N + o_pad
    abuf = _poisoned(M + GUARD_ROWS, lda, dt, dev)
    wbuf = _poisoned(N + GUARD_ROWS, ldw, dt, dev)
    abuf[:M, a_off:a_off + K] = A
    wbuf[:N, w_off:w_off + K] = W
    Av, Wv = abuf[:M, a_off:a_off + K], wbuf[:N, w_off:w_off + K]
    odt = torch.float32 if epilogue in (EPI_RESID_F32, EPI_STORE_F32) else dt
    obuf = _patterned(M + GUARD_ROWS, ldo, odt, dev)
    Ov = obuf[:M, :N]
    es = obuf.element_size()
    rv = r0 = None
    if epilogue == EPI_RESID_F32:
        assert resid is not None and resid.shape == (M, N) and resid.dtype == torch.float32
        r0 = resid.clone()
        if inplace:
            Ov.copy_(resid)
            rv = Ov
        else:
            rbuf = _poisoned(M + GUARD_ROWS, ldo, torch.float32, dev)
            rbuf[:M, :N] = resid
            rv = rbuf[:M, :N]
    else:
        assert resid is None and not inplace
    before = obuf.view(_INT[es]).clone()
    code = DT_BF16 if dt == torch.bfloat16 else DT_F32
    kernel(code, M, N, K, epilogue, Av, lda, Wv, ldw, bias, rv, Ov, ldo)
    after = obuf.view(_INT[es])
    assert torch.equal(after[M:], before[M:]), "the kernel wrote behind row M - 1 of out"
    assert torch.equal(after[:M, N:], before[:M, N:]), "the kernel wrote into out's pad columns"
    got = Ov.clone()
    assert not torch.isnan(got).any(), "NaN in out[:M, :N]: the kernel read poison (rows behind A / W, or pad columns)"
    if not inplace:
        # bf16 0x5A5B = 1.54e16, fp32 0x5A5B5C5D = 1.54e16: no test operand reaches it, so an element still holding it was never written
        assert not (after[:M, :N] == _PATTERN[es]).any(), "out[:M, :N] holds unwritten elements"
    if rv is not None and not inplace:
        assert torch.equal(rv, r0), "the kernel wrote into a separate residual"
    return GemmRun(Av, Wv, bias, r0, got, epilogue, lda, ldw, ldo)


def ref64(A, W, bias=None, resid=None, epilogue=EPI_STORE_F32) -> torch.Tensor:
    """The operation in float64 from the operands as stored (bf16 and fp32 values are exact in float64); erf-GELU."""
    r = A.double() @ W.double().t()
    if bias is not None:
        r = r + bias.double()
    if epilogue == EPI_RESID_F32:
        r = r + resid.double()
    if epilogue == EPI_GELU:
        r = F.gelu(r)
    return r


def bound(A, W, bias=None, resid=None, epilogue=EPI_STORE_F32, ref=None, out_dtype=None) -> torch.Tensor:
    """Element-wise |out - ref64| a correct kernel may show (module docstring).  out_dtype: the type out[:M, :N] is stored in (default: what
    the epilogue stores for bf16 operands)."""
    s = A.double().abs() @ W.double().abs().t() + 1.0
    if bias is not None:
        s = s + bias.double().abs()
    if epilogue == EPI_RESID_F32:
        s = s + resid.double().abs()
    b = ACC_REL * s
    if epilogue == EPI_GELU:
        b = GELU_LIP * b
    if out_dtype is None:
        out_dtype = torch.bfloat16 if epilogue in (EPI_STORE, EPI_GELU) else torch.float32
    if out_dtype == torch.bfloat16:
        if ref is None:
            ref = ref64(A, W, bias, resid, epilogue)
        b = b + OUT_REL * ref.abs()
    return b


def ref_and_bound(run: GemmRun):
    ref = ref64(run.A, run.W, run.bias, run.resid, run.epilogue)
    return ref, bound(run.A, run.W, run.bias, run.resid, run.epilogue, ref, run.out.dtype)


def excess(run: GemmRun) -> torch.Tensor:
    """|out - ref64| / bound per element: a correct kernel stays <= 1 everywhere."""
    ref, b = ref_and_bound(run)
    return (run.out.double() - ref).abs() / b


def kernels_run(fn: Callable[[], None]) -> List[str]:
    """Names of the device kernels fn() launched."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.key for e in prof.key_averages() if e.device_time_total > 0]
