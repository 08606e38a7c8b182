"""Tensor-level wrappers over the C ABI (include/vtgb.h).  PyTorch is plumbing here: it owns
device memory and the stream; all arithmetic of the hot path happens inside libvtgb.so.

Every function takes CUDA(=HIP) tensors, launches asynchronously on the current stream and
returns fresh tensors on the same device.  Nothing here falls back to torch ops."""
from __future__ import annotations

import ctypes as C
import logging
import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib as L
from ._lib import BF16, BF16X3, F16C8, F32

_log = logging.getLogger("videotgb_amd")
_ws_logged = set()


def _log_workspace(what: str, need: int, detail: str) -> None:
    """the split-operand RAFT modes take several times the scratch memory of the bf16 mode -- say so once per (stage, size class) at INFO
    level (logging.getLogger('videotgb_amd')), and as a WARNING when a single call asks for more than 64 GB."""
    key = (what, need >> 30)
    if key in _ws_logged:
        return
    _ws_logged.add(key)
    _log.log(logging.WARNING if need > (64 << 30) else logging.INFO, "%s: %.2f GB of workspace (%s)", what, need / 2 ** 30, detail)

Tensor = torch.Tensor


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _need_cuda(*ts: Tensor) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            raise L.VtgbError("videotgb_amd ops need device tensors: the hot path has no CPU implementation")


def dtype_code(dtype) -> int:
    if dtype in (BF16, "bf16", torch.bfloat16):
        return BF16
    if dtype in (F32, "f32", "fp32", torch.float32):
        return F32
    raise ValueError(f"unsupported compute dtype {dtype!r}")


def raft_dtype_code(dtype) -> int:
    """RAFT's modes: "bf16" (bf16 MFMA, a reduced-precision mode the reference does not have), "bf16x3" (split-bf16 operands: fp32
    accuracy on the bf16 matrix cores) and "f32" (fp32 FMAs in the reference's order, the exactness mode)."""
    if dtype in (BF16X3, "bf16x3", "x3"):
        return BF16X3
    if dtype in (F16C8, "f16c8"):
        return F16C8
    return dtype_code(dtype)


def raft_stage_code(code: int) -> int:
    """The mode of RAFT's correlation volume next to an update block at ``code``: at f16c8 the correlation (and the encoders' stem, stride-2 / 1x1
    convolutions and head, include/vtgb.h) runs at bf16x3."""
    return BF16X3 if code == F16C8 else code


def act_dtype(code: int) -> torch.dtype:
    return torch.bfloat16 if code == BF16 else torch.float32


class _Workspace:
    """Scratch buffer handed to the library, one per (device, stream) -- calls on different streams never share scratch, so
    the wrappers are as re-entrant across streams as the C ABI underneath (grown on demand, never shrunk)."""

    def __init__(self, zero: bool = False):
        self.bufs: Dict[Tuple[int, int], Tensor] = {}
        self.zero = zero

    def get(self, nbytes: int, device) -> Tensor:
        idx = device.index if device.index is not None else torch.cuda.current_device()
        key = (idx, torch.cuda.current_stream(idx).cuda_stream)
        b = self.bufs.get(key)
        if b is None or b.numel() < nbytes:
            self.bufs[key] = b = (torch.zeros if self.zero else torch.empty)(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        return b


_ws = _Workspace()


def pack_weight(w: Tensor, code: int, cols_pad: Optional[int] = None) -> Tensor:
    """GEMM weight in the dtype the kernels consume: fp32 -> as is; bf16 -> one-time vtgb_pack_bf16."""
    _need_cuda(w)
    w2 = w.reshape(w.shape[0], -1).contiguous().float()
    if code == F32:
        return w2
    if code == BF16X3:
        raise ValueError("pack_weight: bf16x3 weights are expanded per convolution (split3_k)")
    rows, cols = w2.shape
    if cols_pad is None and cols % 8:
        raise NotImplementedError(f"bf16 GEMM weights need in_features % 8 == 0 (got {cols})")
    cp = cols_pad or cols
    out = torch.empty(rows, cp, dtype=torch.bfloat16, device=w.device)
    L.check(L.lib().vtgb_pack_bf16(w2.data_ptr(), out.data_ptr(), rows, cols, cp, _stream()))
    return out


# ----------------------------------------------------------------------------- K16-K18
def span_select(logits: Tensor, noise: Tensor, tau: float = 0.5) -> Tensor:
    """logits [B, L, 2] fp32, noise [draws, 2B, L] fp32 -> idx [draws, 2B] int64."""
    _need_cuda(logits, noise)
    logits, noise = logits.contiguous().float(), noise.contiguous().float()
    B, Lf, two = logits.shape
    draws = noise.shape[0]
    if two != 2 or tuple(noise.shape) != (draws, 2 * B, Lf):
        raise ValueError(f"span_select: logits {tuple(logits.shape)} / noise {tuple(noise.shape)} mismatch")
    idx = torch.empty(draws, 2 * B, dtype=torch.int64, device=logits.device)
    a = L.SpanSelectArgs(logits.data_ptr(), noise.data_ptr(), idx.data_ptr(), B, Lf, draws, float(tau))
    L.check(L.lib().vtgb_span_select(C.byref(a), _stream()))
    return idx


def span_to_frames(sel: Tensor, V, N: int, nframe: int, variant: str) -> Tensor:
    """sel [draws, 2B] int64; V int or int32 tensor [B] -> frame_idx [B, nframe] int64."""
    _need_cuda(sel)
    sel = sel.contiguous()
    draws, twoB = sel.shape
    B = twoB // 2
    out = torch.empty(B, nframe, dtype=torch.int64, device=sel.device)
    vt = None
    if isinstance(V, Tensor):
        vt = V.to(device=sel.device, dtype=torch.int32).contiguous()
    a = L.SpanToFramesArgs(sel.data_ptr(), _ptr(vt), out.data_ptr(), B, draws, 0 if vt is not None else int(V), N, nframe,
                           {"A": L.MAP_A, "B": L.MAP_B}[variant])
    L.check(L.lib().vtgb_span_to_frames(C.byref(a), _stream()))
    return out


def gather_frames(pixel_values: Tensor, frame_idx: Tensor) -> Tensor:
    """pixel_values [B, N, ...] fp32, frame_idx [B, nframe] int64 -> [B, nframe, ...] fp32."""
    _need_cuda(pixel_values, frame_idx)
    pv = pixel_values.contiguous().float()
    fi = frame_idx.contiguous()
    B, N = pv.shape[:2]
    nframe = fi.shape[1]
    out = torch.empty((B, nframe) + tuple(pv.shape[2:]), dtype=torch.float32, device=pv.device)
    a = L.GatherFramesArgs(pv.data_ptr(), fi.data_ptr(), out.data_ptr(), B, N, nframe, pv[0, 0].numel())
    L.check(L.lib().vtgb_gather_frames(C.byref(a), _stream()))
    return out


CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def preprocess_frames(raw: Tensor, frame_idx: Optional[Tensor] = None, size: int = 224, mean=CLIP_MEAN, std=CLIP_STD) -> Tensor:
    """raw [T, H0, W0, 3] uint8 decoded frames -> [n_out, 3, size, size] fp32: bilinear resize, truncation to uint8, /255,
    (x - mean) / std (get_frames, eval/utils/builder_utils.py:117-128); frame_idx [n_out] int64 picks source frames."""
    _need_cuda(raw)
    if raw.dtype != torch.uint8 or raw.dim() != 4 or raw.shape[-1] != 3:
        raise TypeError("clip tensor should have data type uint8 and shape [T, H, W, 3]. Got %s %s" % (raw.dtype, tuple(raw.shape)))
    raw = raw.contiguous()
    T, H0, W0, _ = raw.shape
    fi = None if frame_idx is None else frame_idx.to(device=raw.device, dtype=torch.int64).contiguous()
    n_out = T if fi is None else fi.numel()
    out = torch.empty(n_out, 3, size, size, dtype=torch.float32, device=raw.device)
    a = L.PreprocessArgs(raw.data_ptr(), None if fi is None else fi.data_ptr(), out.data_ptr(), T, H0, W0, n_out, size,
                         (C.c_float * 3)(*mean), (C.c_float * 3)(*std))
    L.check(L.lib().vtgb_preprocess_frames(C.byref(a), _stream()))
    return out


# ----------------------------------------------------------------------------- building blocks
def gemm(A: Tensor, W: Tensor, bias: Optional[Tensor] = None, epilogue: int = L.EPI_STORE, resid: Optional[Tensor] = None,
         K: Optional[int] = None) -> Tensor:
    """A [M, K] and W [N, K] in bf16 or fp32 -> out [M, N]."""
    _need_cuda(A, W)
    code = dtype_code(A.dtype)
    M, Ka = A.shape
    N = W.shape[0]
    K = K or Ka
    out_dtype = torch.float32 if epilogue in (L.EPI_RESID_F32, L.EPI_STORE_F32) else A.dtype
    out = torch.empty(M, N, dtype=out_dtype, device=A.device)
    a = L.GemmArgs(code, M, N, K, epilogue, A.data_ptr(), A.stride(0), W.data_ptr(), W.stride(0), _ptr(bias), _ptr(resid),
                   out.data_ptr(), N)
    L.check(L.lib().vtgb_gemm(C.byref(a), _stream()))
    return out


def _skinny_stream_init(self, w: Tensor, nbytes_of, finite: bool = False) -> Tensor:
    """What SkinnyWeight and SkinnyWeightFp8 share: the checks of nn.Linear.weight [N, K] (bf16), ``N``, ``K`` and the allocation of ``data`` (the
    re-laid weight stream, ``nbytes_of(N, K)`` bytes).  Returns the detached weight for the caller's pack call."""
    _need_cuda(w)
    w = w.detach()
    assert w.dtype == torch.bfloat16 and w.dim() == 2 and w.stride(1) == 1
    name = type(self).__name__
    if finite and not bool(torch.isfinite(w).all()):
        raise ValueError(f"{name}: the weights hold Inf or NaN")
    self.N, self.K = w.shape
    nbytes = nbytes_of(self.N, self.K)
    if nbytes == 0:
        raise NotImplementedError(f"{name}: K={self.K} must be a multiple of 64")
    self.data = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    return w


class SkinnyWeight:
    """nn.Linear.weight [N, K] (bf16) re-laid for vtgb_gemm_skinny's weight stream (vtgb_pack_skinny_weight; one-time)."""

    def __init__(self, w: Tensor):
        w = _skinny_stream_init(self, w, L.lib().vtgb_pack_skinny_weight_bytes)
        L.check(L.lib().vtgb_pack_skinny_weight(w.data_ptr(), w.stride(0), self.N, self.K, self.data.data_ptr(), _stream()))


FP8_MAX = 448.0      # largest finite OCP e4m3fn value


def quantize_fp8_rows(w: Tensor) -> Tuple[Tensor, Tensor]:
    """nn.Linear.weight [N, K] -> (q [N, K] torch.float8_e4m3fn, scale [N] fp32): THE definition of the fp8 weight format (decode_weights="fp8";
    vtgb_pack_skinny_weight_fp8 computes the same on the device, bit for bit).  Per output row n: e[n] = the smallest integer with
    amax[n] * 2^-e <= 448 (from the binary exponent: exact; 0 for a zero row), scale[n] = 2^e[n], q[n, :] = w[n, :] * 2^-e rounded to nearest
    even.  The scale is a power of two so that q * scale is exactly representable in bf16: the fp8 model is an ordinary bf16 model whose
    weights are ``dequantize_fp8_rows(q, scale)``.  Runs on any device; a non-finite weight raises ValueError."""
    if w.dim() != 2 or not w.is_floating_point():
        raise ValueError(f"quantize_fp8_rows: a floating-point [N, K] matrix, got {w.dtype} {tuple(w.shape)}")
    wf = w.detach().float()
    if not bool(torch.isfinite(wf).all()):
        raise ValueError("quantize_fp8_rows: the weights hold Inf or NaN")
    amax = wf.abs().amax(dim=1)
    m, x = torch.frexp(amax)                                     # amax = m * 2^x with 0.5 <= m < 1; 448 = 0.875 * 2^9
    e = torch.where(amax > 0, x - 9 + (m > 0.875).to(x.dtype), torch.zeros_like(x))
    q = torch.ldexp(wf, -e[:, None]).to(torch.float8_e4m3fn)
    return q, torch.ldexp(torch.ones_like(amax), e)


def dequantize_fp8_rows(q: Tensor, scale: Tensor, dtype: torch.dtype = torch.bfloat16) -> Tensor:
    """q * scale [N, K]: exact in bf16 (and so in fp32) for the pairs ``quantize_fp8_rows`` returns."""
    return (q.float() * scale.float()[:, None]).to(dtype)


class SkinnyWeightFp8:
    """nn.Linear.weight [N, K] (bf16) quantised per row to e4m3 and re-laid for vtgb_gemm_skinny_fp8's weight stream
    (vtgb_pack_skinny_weight_fp8; one-time): ``data`` = the codes, half the bytes of SkinnyWeight's; ``scale`` [N] fp32 powers of two."""

    def __init__(self, w: Tensor):
        w = _skinny_stream_init(self, w, L.lib().vtgb_pack_skinny_weight_fp8_bytes, finite=True)
        self.scale = torch.empty(self.N, dtype=torch.float32, device=w.device)
        L.check(L.lib().vtgb_pack_skinny_weight_fp8(w.data_ptr(), w.stride(0), self.N, self.K, self.data.data_ptr(), self.scale.data_ptr(), _stream()))

    def codes(self) -> Tensor:
        """q [N, K] float8_e4m3fn, un-tiled (tests): the inverse of the stream's layout -- [tile][k-tile][row][slot g][half][8 codes]."""
        nt, nk = (self.N + 127) // 128, self.K // 64
        t = self.data.view(nt, nk, 128, 4, 2, 8).permute(0, 2, 1, 4, 3, 5).reshape(nt * 128, self.K)
        return t[: self.N].contiguous().view(torch.float8_e4m3fn)


MXFP4_BLOCK = 32                                   # weights along K that share one E8M0 scale
MXFP4_EMIN, MXFP4_EMAX = -120, 125                 # the clamp of the block exponent e (scale byte = e + 127)
_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)   # magnitude of code c & 7; bit 3 is the sign


def _pow2(e: Tensor) -> Tensor:
    """2^e in fp32 for integer e in [-126, 127], built in the exponent field (exact on every backend)."""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


def quantize_mxfp4_rows(w: Tensor) -> Tuple[Tensor, Tensor]:
    """nn.Linear.weight [N, K] -> (codes [N, K / 2] uint8, scales [N, K / 32] uint8): THE definition of the MXFP4 weight format (decode_weights="mxfp4";
    vtgb_pack_skinny_weight_mxfp4 computes the same on the device, bit for bit).  OCP Microscaling v1.0, MXFP4: along K every block of 32
    consecutive weights of a row shares one E8M0 scale 2^e, e = floor(log2(amax of the block)) - 2 (from the binary exponent: exact; 0 for an
    all-zero block), clamped to [-120, 125] and stored as the byte e + 127.  An element is w * 2^-e rounded to the nearest e2m1 number (sign;
    magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6 = codes 0 .. 7), ties to the even code, saturating at +-6; the sign bit (code bit 3) is the weight's
    own, so a weight that rounds to zero keeps its sign.  Two codes per byte, the lower k in the low nibble.  Two properties follow.  Exactness:
    code * 2^e has at most two mantissa bits and an exponent within [-121, 127], so it is exactly a normal (finite) bf16 number, and the mxfp4
    model is an ordinary bf16 model whose weights are ``dequantize_mxfp4_rows(codes, scales)``.  Idempotence: the largest element of a block
    scales into [4, 8) and rounds to 4 or 6, which gives the same e again, so quantising the dequantised matrix returns the same codes and scale
    bytes (the decoder re-packs from its dequantised copy).  The one exception is a block under the lower clamp whose every element rounds to
    zero (amax <= 2^-122, bf16 subnormals among them): its byte is 7 (e = -120), and the all-zero block it dequantises to has byte 127 -- the
    same (zero) values.  The ids of the mode are the quantised model's, not the reference's, and answer quality on a trained checkpoint is not
    measured by this project.  Runs on any device; a non-finite weight and a non-2-D input raise ValueError, K % 64 != 0 NotImplementedError
    (the weight streams' k-tile)."""
    if w.dim() != 2 or not w.is_floating_point():
        raise ValueError(f"quantize_mxfp4_rows: a floating-point [N, K] matrix, got {w.dtype} {tuple(w.shape)}")
    N, K = w.shape
    if K == 0 or K % 64 != 0:
        raise NotImplementedError(f"quantize_mxfp4_rows: K={K} must be a multiple of 64")
    wf = w.detach().float()
    if not bool(torch.isfinite(wf).all()):
        raise ValueError("quantize_mxfp4_rows: the weights hold Inf or NaN")
    a = wf.abs().view(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    amax = a.amax(dim=2)
    _, x = torch.frexp(amax)                                     # amax = m * 2^x with 0.5 <= m < 1: floor(log2(amax)) = x - 1
    e = torch.where(amax > 0, x - 3, torch.zeros_like(x)).clamp_(MXFP4_EMIN, MXFP4_EMAX)
    v = a * _pow2(-e)[:, :, None]                                # exact (or below 2^-126, where the code is 0 either way)
    mag = ((v > 0.25).to(torch.uint8) + (v >= 0.75).to(torch.uint8) + (v > 1.25).to(torch.uint8) + (v >= 1.75).to(torch.uint8)
           + (v > 2.5).to(torch.uint8) + (v >= 3.5).to(torch.uint8) + (v > 5.0).to(torch.uint8))      # midpoints go to the even code
    c = (mag | (torch.signbit(wf).view_as(mag).to(torch.uint8) << 3)).view(N, K // 2, 2)
    return (c[:, :, 0] | (c[:, :, 1] << 4)).contiguous(), (e + 127).to(torch.uint8)


def dequantize_mxfp4_rows(codes: Tensor, scales: Tensor, dtype: torch.dtype = torch.bfloat16) -> Tensor:
    """code * 2^e [N, K]: exact in bf16 (and so in fp32) for the pairs ``quantize_mxfp4_rows`` returns."""
    N, K = codes.shape[0], codes.shape[1] * 2
    c = torch.stack((codes & 15, codes >> 4), dim=2).view(N, K).long()
    mag = torch.tensor(_E2M1, dtype=torch.float32, device=codes.device)[c & 7]
    val = torch.where((c & 8) != 0, -mag, mag).view(N, K // MXFP4_BLOCK, MXFP4_BLOCK) * _pow2(scales.to(torch.int32) - 127)[:, :, None]
    return val.view(N, K).to(dtype)


class SkinnyWeightMxfp4:
    """nn.Linear.weight [N, K] (bf16) quantised to MXFP4 (``quantize_mxfp4_rows``) and re-laid for vtgb_gemm_skinny_mxfp4's weight stream
    (vtgb_pack_skinny_weight_mxfp4; one-time): ``data`` = per (128-row tile, 64-deep k-tile) 4 KiB of codes and 256 scale bytes, 17 / 32 of
    SkinnyWeightFp8's bytes."""

    def __init__(self, w: Tensor):
        w = _skinny_stream_init(self, w, L.lib().vtgb_pack_skinny_weight_mxfp4_bytes, finite=True)
        L.check(L.lib().vtgb_pack_skinny_weight_mxfp4(w.data_ptr(), w.stride(0), self.N, self.K, self.data.data_ptr(), _stream()))

    def _blocks(self) -> Tensor:
        return self.data.view((self.N + 127) // 128, self.K // 64, 4096 + 256)

    def codes(self) -> Tensor:
        """codes [N, K / 2] uint8, un-tiled (tests): the inverse of the stream's layout -- [tile][k-tile][wave][row & 15][k chunk][fragment][half][4 bytes]."""
        nt, nk = (self.N + 127) // 128, self.K // 64
        t = self._blocks()[:, :, :4096].reshape(nt, nk, 4, 16, 4, 2, 2, 4).permute(0, 2, 5, 3, 1, 6, 4, 7).reshape(nt * 128, self.K // 2)
        return t[: self.N].contiguous()

    def scales(self) -> Tensor:
        """scale bytes [N, K / 32] uint8, un-tiled (tests): [tile][k-tile][wave][row & 15][fragment][half]."""
        nt, nk = (self.N + 127) // 128, self.K // 64
        t = self._blocks()[:, :, 4096:].reshape(nt, nk, 4, 16, 2, 2).permute(0, 2, 4, 3, 1, 5).reshape(nt * 128, self.K // 32)
        return t[: self.N].contiguous()


def gemm_skinny_workspace_bytes(M: int, N: int, K: int, n_splits: int = 0) -> int:
    a = L.GemmSkinnyArgs(M, N, K, n_splits, None, K, None, K, None, N, BF16, 0, None, 0)
    return int(L.lib().vtgb_gemm_skinny_workspace_bytes(C.byref(a)))


def gemm_skinny(x: Tensor, w: Tensor, out: Optional[Tensor] = None, n_splits: int = 0, out_dtype: Optional[torch.dtype] = None,
                workspace: Optional[Tensor] = None, defer_reduce: bool = False, bias: Optional[Tensor] = None):
    """``defer_reduce``: returns (out, n_splits, workspace) and leaves the K-split fragments to the consumer (see below).
    x [M <= 128, K] bf16, w [N, K] bf16 (nn.Linear.weight, or its SkinnyWeight) -> x @ w.T [M, N]: the decode step's projections (vtgb_gemm_skinny:
    the weights stream once, K split over workgroups, fp32 partials added in a fixed order).  A ``SkinnyWeightFp8`` streams e4m3 codes instead
    (vtgb_gemm_skinny_fp8): the result is that of the bf16 weights ``dequantize_fp8_rows(*quantize_fp8_rows(w))``, bit for bit; a ``SkinnyWeightMxfp4``
    streams MXFP4 codes and block scales (vtgb_gemm_skinny_mxfp4), likewise equal to the bf16 kernel on ``dequantize_mxfp4_rows(*quantize_mxfp4_rows(w))``.  ``out`` may be a preallocated
    [M, N] tensor and ``workspace`` a preallocated uint8 scratch (hipGraph capture: fixed addresses, no allocation).  ``bias`` [N] fp32 (a projection
    bias; never quantised): x @ w.T + bias through vtgb_gemm_skinny_bias, either stream -- added in fp32 to K split 0, so the fragments a
    ``defer_reduce`` call leaves already hold it (the mxfp4 entry takes it itself); None takes the entries above, unchanged."""
    fp8, mxfp4 = isinstance(w, SkinnyWeightFp8), isinstance(w, SkinnyWeightMxfp4)
    tiled = fp8 or mxfp4 or isinstance(w, SkinnyWeight)
    _need_cuda(x, w.data if tiled else w)
    assert x.dtype == torch.bfloat16 and x.stride(1) == 1 and (tiled or (w.dtype == torch.bfloat16 and w.stride(1) == 1))
    M, K = x.shape
    N = w.N if tiled else w.shape[0]
    assert not tiled or w.K == K
    if out is None:
        out = torch.empty(M, N, dtype=out_dtype or x.dtype, device=x.device)
    a = L.GemmSkinnyArgs(M, N, K, n_splits, x.data_ptr(), x.stride(0), w.data.data_ptr() if tiled else w.data_ptr(), K if tiled else w.stride(0),
                         out.data_ptr(), out.stride(0), dtype_code(out.dtype), 1 if tiled else 0, None, 0, 1 if defer_reduce else 0)
    need = L.lib().vtgb_gemm_skinny_workspace_bytes(C.byref(a))      # 0: no K split (or bad arguments, which the call reports)
    if need:
        ws = workspace if workspace is not None else _ws.get(need, x.device)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    if bias is not None:
        _need_cuda(bias)
        assert bias.dtype == torch.float32 and tuple(bias.shape) == (N,) and bias.stride(0) == 1
    if mxfp4:
        L.check(L.lib().vtgb_gemm_skinny_mxfp4(C.byref(a), _ptr(bias), _stream()))
    elif bias is not None:
        L.check(L.lib().vtgb_gemm_skinny_bias(C.byref(a), w.scale.data_ptr() if fp8 else None, bias.data_ptr(), _stream()))
    elif fp8:
        L.check(L.lib().vtgb_gemm_skinny_fp8(C.byref(a), w.scale.data_ptr(), _stream()))
    else:
        L.check(L.lib().vtgb_gemm_skinny(C.byref(a), _stream()))
    if defer_reduce:
        # (out, n_splits, fragments): n_splits > 1 -> `out` is NOT written; the consumer (vtgb_llm_rmsnorm_parts / vtgb_llm_rope_cache_parts) adds the
        # fragments left in the workspace
        S = int(L.lib().vtgb_gemm_skinny_splits(C.byref(a))) if need else 1
        return out, S, (ws if need else None)
    return out


# keys one (batch, head) of vtgb_attention's bf16 kernel holds in LDS, by head_dim (attn.hip's ladder); past them the tiled kernel takes over
_SINGLE_PASS_KEYS = {128: 288, 64: 512}


def attention(q: Tensor, k: Tensor, v: Tensor, heads: int, scale: float, key_mask: Optional[Tensor] = None,
              rope_q: Optional[Tensor] = None, rope_k: Optional[Tensor] = None, causal: bool = False,
              kv_heads: Optional[int] = None) -> Tensor:
    """q [B, Sq, H*hd], k/v [B, Skv, H*hd] (any token/batch strides, unit channel stride) -> [B, Sq, H*hd].
    ``causal``: query q attends keys <= q + (Skv - Sq).  ``kv_heads`` (grouped-query attention): k/v are [B, Skv, kv_heads*hd] and
    query head h reads K/V head h // (heads // kv_heads).  bf16 causal calls without rotary tables whose keys exceed the single-pass
    kernel's LDS (288 at head_dim 128, 512 at 64) or whose ``kv_heads`` differs from ``heads`` run on the tiled kernel
    (``attention_tiled``); every other call is vtgb_attention, which takes equal head counts only."""
    _need_cuda(q, k, v)
    hd = q.shape[2] // heads
    grouped = kv_heads is not None and kv_heads != heads
    if q.dtype == torch.bfloat16 and causal and rope_q is None and rope_k is None and hd in _SINGLE_PASS_KEYS and (
            grouped or k.shape[1] > _SINGLE_PASS_KEYS[hd]):
        return attention_tiled(q, k, v, heads, scale, kv_heads=kv_heads, key_mask=key_mask, causal=True)
    if grouped:
        raise NotImplementedError(f"ops.attention: kv_heads={kv_heads} != heads={heads} is implemented for bf16 causal calls without "
                                  f"rotary tables at head_dim 64 / 128 (the tiled kernel)")
    code = dtype_code(q.dtype)
    B, Sq, D = q.shape
    Skv = k.shape[1]
    assert k.stride() == v.stride() and q.stride(2) == 1 and k.stride(2) == 1
    out = torch.empty(B, Sq, D, dtype=q.dtype, device=q.device)
    a = L.AttentionArgs(code, B, heads, D // heads, Sq, Skv, q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(1), k.stride(1),
                        q.stride(0), k.stride(0), _ptr(key_mask), _ptr(rope_q), _ptr(rope_k), float(scale), out.data_ptr(),
                        out.stride(1), out.stride(0), int(causal))
    L.check(L.lib().vtgb_attention(C.byref(a), _stream()))
    return out


def attention_tiled(q: Tensor, k: Tensor, v: Tensor, heads: int, scale: float, kv_heads: Optional[int] = None,
                    key_mask: Optional[Tensor] = None, causal: bool = True) -> Tensor:
    """vtgb_attention_tiled: bf16 q [B, Sq, heads*hd], k/v [B, Skv <= 4096, kv_heads*hd] (hd 64 or 128) -> [B, Sq, heads*hd]; online
    softmax over 64-key tiles, K/V heads read in place.  ``key_mask`` [B, Skv] fp32: finfo(float32).min masks a key hard (weight
    exactly 0, its K/V rows never read), other values are added to the scaled score."""
    _need_cuda(q, k, v)
    assert q.dtype == k.dtype == v.dtype == torch.bfloat16, "attention_tiled is a bf16 kernel"
    kv_heads = heads if kv_heads is None else kv_heads
    B, Sq, D = q.shape
    Skv = k.shape[1]
    assert k.stride() == v.stride() and q.stride(2) == 1 and k.stride(2) == 1
    assert key_mask is None or (key_mask.dtype == torch.float32 and key_mask.shape == (B, Skv) and key_mask.is_contiguous())
    out = torch.empty(B, Sq, D, dtype=q.dtype, device=q.device)
    a = L.AttentionTiledArgs(B, heads, kv_heads, D // heads, Sq, Skv, q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(1), k.stride(1),
                             q.stride(0), k.stride(0), _ptr(key_mask), float(scale), int(causal), out.data_ptr(), out.stride(1), out.stride(0))
    L.check(L.lib().vtgb_attention_tiled(C.byref(a), _stream()))
    return out


ATTENTION_CACHED_MAX_KEYS = 16384


def attention_cached(q: Tensor, kc: Tensor, vc: Tensor, q0: int, heads: int, scale: float, key_valid: Optional[Tensor] = None,
                     scales: Optional[Tuple[Tensor, Tensor]] = None) -> Tensor:
    """vtgb_attention_cached: a chunk of queries over the decoder's KV cache.  q [B, Sq, heads*hd] bf16 (unit channel stride) are the
    positions q0 .. q0+Sq-1; kc / vc [B, kv_heads, tmax <= 16384, hd] (hd 64 or 128) contiguous, bf16 -- or, with ``scales`` = (ks, vs)
    [B, kv_heads, tmax] fp32, uint8 / float8_e4m3fn codes (``quantize_fp8_kv``) -> [B, Sq, heads*hd] bf16.  Query i sees cache rows
    0 .. q0+i; rows from q0+Sq on are never read.  ``key_valid`` [B, tmax] uint8: keys with 0 get weight exactly 0 and are never read.
    The bits are ``attention_tiled``'s on the same values with Skv = q0+Sq."""
    _need_cuda(q, kc, vc)
    B, Sq, D = q.shape
    assert kc.dim() == 4 and kc.shape[0] == B and vc.shape == kc.shape and kc.is_contiguous() and vc.is_contiguous()
    nkv, tmax, hd = kc.shape[1:]
    assert q.dtype == torch.bfloat16 and q.stride(2) == 1 and D == heads * hd, "attention_cached: q [B, Sq, heads*hd] bf16"
    ks = vs = None
    if scales is None:
        assert kc.dtype == vc.dtype == torch.bfloat16, "attention_cached: bf16 caches, or codes with scales=(ks, vs)"
    else:
        ks, vs = scales
        _need_cuda(ks, vs)
        assert kc.element_size() == 1 and vc.element_size() == 1, "attention_cached: with scales the caches hold e4m3 codes"
        assert ks.dtype == vs.dtype == torch.float32 and ks.shape == vs.shape == (B, nkv, tmax) and ks.is_contiguous() and vs.is_contiguous()
    assert key_valid is None or (key_valid.dtype == torch.uint8 and key_valid.shape == (B, tmax) and key_valid.is_contiguous())
    out = torch.empty(B, Sq, D, dtype=q.dtype, device=q.device)
    a = L.AttentionCachedArgs(B, heads, nkv, hd, Sq, int(q0), tmax, float(scale), q.data_ptr(), kc.data_ptr(), vc.data_ptr(), _ptr(ks), _ptr(vs),
                              _ptr(key_valid), q.stride(1), q.stride(0), out.data_ptr(), out.stride(1), out.stride(0))
    L.check(L.lib().vtgb_attention_cached(C.byref(a), _stream()))
    return out


# ---- single-query attention of the decode step.  Two kernels: vtgb_llm_decode_attention{,_masked} (one wave per (row, head), every score in
# LDS: caches up to 2048 slots, any head_dim <= 256) and vtgb_llm_decode_attention_split (256-key chunks over workgroups + a combine launch:
# caches up to 16384 slots, head_dim 64 / 128, K/V read once per group of query heads).  DECODE_SPLIT_MIN_KEYS: the cache length from which
# the split kernel is used where both apply.  2112 = only where the one-wave kernel refuses: the fallback of the routing rule, the two kernels
# have not been timed against each other yet ("Split-KV decode attention").
DECODE_SINGLE_MAX_KEYS = 2048
DECODE_SPLIT_MAX_KEYS = 16384
DECODE_SPLIT_CHUNK = 256
DECODE_SPLIT_MIN_KEYS = 2112


def decode_attention_route(tmax: int, hd: int, min_keys: Optional[int] = None) -> Optional[str]:
    """The kernel a cache of ``tmax`` slots and head_dim ``hd`` decodes on: "split", "single", or None where neither takes it."""
    min_keys = DECODE_SPLIT_MIN_KEYS if min_keys is None else min_keys
    split_ok = hd in (64, 128) and tmax % 64 == 0 and tmax <= DECODE_SPLIT_MAX_KEYS
    single_ok = tmax <= DECODE_SINGLE_MAX_KEYS and hd <= 256
    if split_ok and (tmax >= min_keys or not single_ok):
        return "split"
    return "single" if single_ok else None


def decode_attention_workspace_bytes(B: int, nq: int, hd: int, tmax: int) -> int:
    return int(L.lib().vtgb_llm_decode_attention_split_workspace_bytes(B, nq, hd, tmax))


def _decode_attention_buffers(what: str, q: Tensor, rows: int, nq: int, hd: int, ws_tmax: Optional[int], key_valid: Optional[Tensor], valid_shape,
                              out: Optional[Tensor], workspace: Optional[Tensor]) -> Tuple[Tensor, Optional[Tensor]]:
    """What the decode-attention entries share: the form of ``key_valid`` [valid_shape] uint8, ``out`` [rows, nq*hd] and the split-KV
    workspace for a cache of ``ws_tmax`` slots, both allocated here when None (``ws_tmax`` None: the one-wave kernel, no workspace)."""
    assert key_valid is None or (key_valid.dtype == torch.uint8 and key_valid.shape == valid_shape and key_valid.is_contiguous())
    if out is None:
        out = torch.empty(rows, nq * hd, dtype=q.dtype, device=q.device)
    if ws_tmax is not None:
        need = decode_attention_workspace_bytes(rows, nq, hd, ws_tmax)
        if workspace is None:
            workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=q.device)
        assert workspace.numel() * workspace.element_size() >= need, f"{what}: workspace too small"
    return out, workspace


def decode_attention(q: Tensor, kc: Tensor, vc: Tensor, pos: Tensor, scale: float, key_valid: Optional[Tensor] = None,
                     out: Optional[Tensor] = None, workspace: Optional[Tensor] = None, split: Optional[bool] = None) -> Tensor:
    """q [B, nq*hd], kc / vc [B, nkv, tmax, hd] (the static cache), pos: device int64 -> out [B, nq*hd] = softmax(scale q K[0..pos]^T) V[0..pos].
    ``key_valid`` [B, tmax] uint8: keys with 0 get no weight.  The one place that picks the kernel: ``split=None`` follows
    ``decode_attention_route``; True / False force one (False past 2048 keys raises what vtgb_llm_decode_attention raises).  The split
    kernel's ``workspace`` (uint8, ``decode_attention_workspace_bytes``) is allocated here when None."""
    _need_cuda(q, kc, vc, pos)
    B, nkv, tmax, hd = kc.shape
    nq = q.numel() // (B * hd)
    assert kc.is_contiguous() and vc.is_contiguous() and q.is_contiguous() and vc.shape == kc.shape and q.dtype == kc.dtype == vc.dtype
    assert pos.dtype == torch.int64
    if split is None:
        route = decode_attention_route(tmax, hd)
        split = route == "split" if route is not None else tmax > DECODE_SINGLE_MAX_KEYS      # (neither: the entry that refuses it names the reason)
    code = dtype_code(q.dtype)
    out, workspace = _decode_attention_buffers("decode_attention", q, B, nq, hd, tmax if split else None, key_valid, (B, tmax), out, workspace)
    lib = L.lib()
    if split:
        L.check(lib.vtgb_llm_decode_attention_split(code, _ptr(q), _ptr(kc), _ptr(vc), _ptr(out), _ptr(pos), _ptr(key_valid), _ptr(workspace), B, nq, nkv,
                                                    hd, tmax, float(scale), _stream()))
    elif key_valid is not None:
        L.check(lib.vtgb_llm_decode_attention_masked(code, _ptr(q), _ptr(kc), _ptr(vc), _ptr(out), _ptr(pos), _ptr(key_valid), B, nq, nkv, hd, tmax,
                                                     float(scale), _stream()))
    else:
        L.check(lib.vtgb_llm_decode_attention(code, _ptr(q), _ptr(kc), _ptr(vc), _ptr(out), _ptr(pos), B, nq, nkv, hd, tmax, float(scale), _stream()))
    return out


# ---- fp8 K/V cache (opt-in: kv_cache="fp8").  A cache row -- one token of one K/V head -- is e4m3 codes and one power-of-two scale.
KV_FP8_MIN_EXP = -100      # the scale's exponent is clamped here, so that code * scale stays a normal bf16 number (the smallest code is 2^-9)


def quantize_fp8_kv(x: Tensor) -> Tuple[Tensor, Tensor]:
    """x [..., hd] -> (codes [..., hd] torch.float8_e4m3fn, scale [...] fp32): THE definition of the fp8 K/V cache format (kv_cache="fp8";
    vtgb_llm_rope_cache_fp8 / _prefill_fp8 compute the same on the device, bit for bit).  ``quantize_fp8_rows``' rule on the last dimension:
    e = the smallest integer with amax * 2^-e <= 448 (from the binary exponent: exact; 0 for a zero row), clamped below at -100,
    scale = 2^e, codes = x * 2^-e rounded to nearest even.  codes * scale is exactly representable in bf16: the mode is an ordinary bf16
    model whose K and V pass through ``dequantize_fp8_kv(*quantize_fp8_kv(.))`` as they are produced.  Runs on any device (no host
    synchronisation: it may be captured); non-finite values are outside the contract, as they are for the bf16 cache."""
    xf = x.detach().float()
    amax = xf.abs().amax(dim=-1)
    m, ex = torch.frexp(amax)                                    # amax = m * 2^ex with 0.5 <= m < 1; 448 = 0.875 * 2^9
    e = torch.where(amax > 0, ex - 9 + (m > 0.875).to(ex.dtype), torch.zeros_like(ex)).clamp(min=KV_FP8_MIN_EXP)
    q = (xf * _pow2(-e)[..., None]).to(torch.float8_e4m3fn)
    return q, _pow2(e)


def _pow2(e: Tensor) -> Tensor:
    """2^e as fp32 for integer e in [-126, 127], built on the bits: exact on every device (a pow-based ldexp need not be)."""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


def dequantize_fp8_kv(q: Tensor, scale: Tensor, dtype: torch.dtype = torch.bfloat16) -> Tensor:
    """codes * scale [..., hd]: exact in bf16 (and so in fp32) for the pairs ``quantize_fp8_kv`` returns."""
    return (q.float() * scale.float()[..., None]).to(dtype)


def fp8_kv_round(x: Tensor) -> Tensor:
    """x [..., hd] as the fp8 K/V cache holds it: dequantize_fp8_kv(*quantize_fp8_kv(x)) in x's dtype."""
    return dequantize_fp8_kv(*quantize_fp8_kv(x), dtype=x.dtype)


def decode_attention_fp8_ok(tmax: int, hd: int) -> bool:
    """Whether vtgb_llm_decode_attention_split_fp8 takes a cache of ``tmax`` slots and head_dim ``hd`` (the split kernel's limits)."""
    return hd in (64, 128) and tmax > 0 and tmax % 64 == 0 and tmax <= DECODE_SPLIT_MAX_KEYS


def decode_attention_fp8(q: Tensor, kc8: Tensor, vc8: Tensor, ks: Tensor, vs: Tensor, pos: Tensor, scale: float, key_valid: Optional[Tensor] = None,
                         out: Optional[Tensor] = None, workspace: Optional[Tensor] = None) -> Tensor:
    """``decode_attention`` over an fp8 K/V cache: q [B, nq*hd] bf16, kc8 / vc8 [B, nkv, tmax, hd] uint8 (or float8_e4m3fn) codes, ks / vs
    [B, nkv, tmax] fp32 row scales (``quantize_fp8_kv``) -> out [B, nq*hd] bf16.  Always the split-KV kernel (vtgb_llm_decode_attention_split_fp8,
    caches from 64 slots up); the result is ``decode_attention(q, dq(kc8, ks), dq(vc8, vs), ..., split=True)``, bit for bit.  ``workspace``:
    ``decode_attention_workspace_bytes``, allocated here when None."""
    _need_cuda(q, kc8, vc8, ks, vs, pos)
    B, nkv, tmax, hd = kc8.shape
    nq = q.numel() // (B * hd)
    assert kc8.element_size() == 1 and vc8.element_size() == 1 and kc8.is_contiguous() and vc8.is_contiguous() and vc8.shape == kc8.shape
    assert ks.dtype == vs.dtype == torch.float32 and ks.shape == vs.shape == (B, nkv, tmax) and ks.is_contiguous() and vs.is_contiguous()
    assert q.is_contiguous() and pos.dtype == torch.int64
    out, workspace = _decode_attention_buffers("decode_attention_fp8", q, B, nq, hd, tmax, key_valid, (B, tmax), out, workspace)
    L.check(L.lib().vtgb_llm_decode_attention_split_fp8(dtype_code(q.dtype), _ptr(q), _ptr(kc8), _ptr(vc8), _ptr(ks), _ptr(vs), _ptr(out), _ptr(pos),
                                                        _ptr(key_valid), _ptr(workspace), B, nq, nkv, hd, tmax, float(scale), _stream()))
    return out


# ---- beam search on the Llama decode step (opt-in: beam_search="graph").  R = B * K beam rows, the beams of item b are rows b K .. b K + K - 1.
BEAM_MAX_BEAMS = 16
BEAM_MAX_VOCAB = 1 << 20


def decode_attention_beam_ok(tmax_p: int, tmax_g: int, hd: int) -> bool:
    """Whether vtgb_llm_decode_attention_beam takes these cache lengths and head_dim (the split kernel's limits on tmax_p + tmax_g)."""
    return hd in (64, 128) and tmax_p > 0 and tmax_g > 0 and tmax_p % 64 == 0 and tmax_g % 64 == 0 and tmax_p + tmax_g <= DECODE_SPLIT_MAX_KEYS


def decode_attention_beam(q: Tensor, kp: Tensor, vp: Tensor, kg: Tensor, vg: Tensor, src_row: Tensor, n_prompt: Tensor, pos: Tensor, scale: float,
                          key_valid: Optional[Tensor] = None, out: Optional[Tensor] = None, workspace: Optional[Tensor] = None) -> Tensor:
    """``decode_attention(split=True)`` for the R = B * K beam rows of a batch, over two K/V sources and without K/V copies: q [R, nq*hd];
    kp / vp [B, nkv, tmax_p, hd] the prompt cache (once per batch item); kg / vg [R, nkv, tmax_g, hd] what the beams generated, one slot per
    step; src_row [R, tmax_g] int32, the generated-cache row that holds row r's key of slot s.  Key t of row r is ``kp[r // K, :, t]`` for
    t < n_prompt, else ``kg[src_row[r, t - n_prompt], :, t - n_prompt]``; visible while t <= pos (n_prompt, pos: device int64) and, for
    prompt keys, ``key_valid`` [B, tmax_p] uint8 != 0.  The result equals ``decode_attention(q, K, V, pos, scale, split=True)`` on the caches
    K / V [R, nkv, T, hd] materialised by that gather, bit for bit.  ``workspace``: ``decode_attention_workspace_bytes(R, nq, hd, tmax_p + tmax_g)``."""
    _need_cuda(q, kp, vp, kg, vg, src_row, n_prompt, pos)
    B, nkv, tmax_p, hd = kp.shape
    R, _, tmax_g, _ = kg.shape
    nq = q.numel() // (R * hd)
    assert R % B == 0 and kg.shape == (R, nkv, tmax_g, hd) and vp.shape == kp.shape and vg.shape == kg.shape
    assert all(t.is_contiguous() for t in (q, kp, vp, kg, vg, src_row)) and q.dtype == kp.dtype == vp.dtype == kg.dtype == vg.dtype
    assert src_row.dtype == torch.int32 and src_row.shape == (R, tmax_g) and pos.dtype == torch.int64 and n_prompt.dtype == torch.int64
    out, workspace = _decode_attention_buffers("decode_attention_beam", q, R, nq, hd, tmax_p + tmax_g, key_valid, (B, tmax_p), out, workspace)
    a = L.LlmDecodeAttentionBeamArgs(dtype_code(q.dtype), R, R // B, nq, nkv, hd, tmax_p, tmax_g, float(scale), _ptr(q), _ptr(kp), _ptr(vp), _ptr(kg),
                                     _ptr(vg), _ptr(src_row), _ptr(out), _ptr(n_prompt), _ptr(pos), _ptr(key_valid), _ptr(workspace))
    L.check(L.lib().vtgb_llm_decode_attention_beam(C.byref(a), _stream()))
    return out


def decode_attention_beam_fp8_ok(tmax_p: int, tmax_g: int, hd: int) -> bool:
    """Whether vtgb_llm_decode_attention_beam_fp8 takes these cache lengths and head_dim (``decode_attention_beam_ok``: the same kernel body)."""
    return decode_attention_beam_ok(tmax_p, tmax_g, hd)


def decode_attention_beam_fp8(q: Tensor, kp8: Tensor, vp8: Tensor, kps: Tensor, vps: Tensor, kg8: Tensor, vg8: Tensor, kgs: Tensor, vgs: Tensor,
                              src_row: Tensor, n_prompt: Tensor, pos: Tensor, scale: float, key_valid: Optional[Tensor] = None,
                              out: Optional[Tensor] = None, workspace: Optional[Tensor] = None) -> Tensor:
    """``decode_attention_beam`` over fp8 K/V caches (vtgb_llm_decode_attention_beam_fp8): q [R, nq*hd] bf16; kp8 / vp8 [B, nkv, tmax_p, hd]
    uint8 (or float8_e4m3fn) codes with kps / vps [B, nkv, tmax_p] fp32 row scales, the prompt cache; kg8 / vg8 [R, nkv, tmax_g, hd] with
    kgs / vgs [R, nkv, tmax_g], what the beams generated; src_row, n_prompt, pos, key_valid as there.  The result is
    ``decode_attention_beam`` on the dequantised caches (``dequantize_fp8_kv``), bit for bit."""
    _need_cuda(q, kp8, vp8, kps, vps, kg8, vg8, kgs, vgs, src_row, n_prompt, pos)
    B, nkv, tmax_p, hd = kp8.shape
    R, _, tmax_g, _ = kg8.shape
    nq = q.numel() // (R * hd)
    assert R % B == 0 and kg8.shape == (R, nkv, tmax_g, hd) and vp8.shape == kp8.shape and vg8.shape == kg8.shape
    assert all(t.element_size() == 1 for t in (kp8, vp8, kg8, vg8)) and all(t.dtype == torch.float32 for t in (kps, vps, kgs, vgs))
    assert kps.shape == vps.shape == (B, nkv, tmax_p) and kgs.shape == vgs.shape == (R, nkv, tmax_g)
    assert all(t.is_contiguous() for t in (q, kp8, vp8, kps, vps, kg8, vg8, kgs, vgs, src_row))
    assert src_row.dtype == torch.int32 and src_row.shape == (R, tmax_g) and pos.dtype == torch.int64 and n_prompt.dtype == torch.int64
    out, workspace = _decode_attention_buffers("decode_attention_beam_fp8", q, R, nq, hd, tmax_p + tmax_g, key_valid, (B, tmax_p), out, workspace)
    a = L.LlmDecodeAttentionBeamFp8Args(dtype_code(q.dtype), R, R // B, nq, nkv, hd, tmax_p, tmax_g, float(scale), _ptr(q), _ptr(kp8), _ptr(vp8),
                                        _ptr(kps), _ptr(vps), _ptr(kg8), _ptr(vg8), _ptr(kgs), _ptr(vgs), _ptr(src_row), _ptr(out), _ptr(n_prompt),
                                        _ptr(pos), _ptr(key_valid), _ptr(workspace))
    L.check(L.lib().vtgb_llm_decode_attention_beam_fp8(C.byref(a), _stream()))
    return out


def beam_candidates_workspace_bytes(R: int, K: int, V: int) -> int:
    """vtgb_llm_beam_candidates' workspace: the rows' fp32 log-probabilities and their 2 K candidates each."""
    return R * V * 4 + R * 2 * K * 8


def beam_candidates(logits: Tensor, seq: Tensor, step: Tensor, running: Tensor, repetition_penalty: float = 1.0, eos: Optional[int] = None,
                    min_new: int = 0, out: Optional[Tuple[Tensor, Tensor]] = None, workspace: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """One beam-search step's candidates (vtgb_llm_beam_candidates): logits [B*K, V] bf16 / fp32, seq [B*K, N] int64 generated ids of which the
    first ``step`` (device int64) count, running [B, K] fp32 -> (cand_score [B, 2K] fp32, cand_idx [B, 2K] int32 = k * V + token): per batch
    item the 2K largest of ``log_softmax(logits.float())`` after HF's repetition penalty on the ids generated so far (each once), with
    ``eos`` at -inf while step < min_new, plus the running score of the row -- descending, equal scores in ascending index."""
    _need_cuda(logits, seq, step, running)
    R, V = logits.shape
    B, K = running.shape
    N = seq.shape[1]
    assert R == B * K and seq.shape == (R, N) and seq.dtype == torch.int64 and step.dtype == torch.int64 and running.dtype == torch.float32
    assert logits.is_contiguous() and seq.is_contiguous() and running.is_contiguous()
    if out is None:
        out = (torch.empty(B, 2 * K, dtype=torch.float32, device=logits.device), torch.empty(B, 2 * K, dtype=torch.int32, device=logits.device))
    need = beam_candidates_workspace_bytes(R, K, V)
    if workspace is None:
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=logits.device)
    a = L.LlmBeamCandidatesArgs(dtype_code(logits.dtype), R, K, V, N, -1 if eos is None else int(eos), int(min_new), float(repetition_penalty),
                                _ptr(logits), _ptr(seq) if N else None, _ptr(step), _ptr(running), _ptr(out[0]), _ptr(out[1]), _ptr(workspace),
                                workspace.numel() * workspace.element_size())
    L.check(L.lib().vtgb_llm_beam_candidates(C.byref(a), _stream()))
    return out


# ---- eos-id sets on the graph decoders (opt-in: eos_sets="graph").  A request's eos ids as a device int32 list of up to EOS_MAX entries
# (VTGB_LLM_EOS_MAX of include/vtgb.h), read by vtgb_llm_pick_greedy and vtgb_llm_beam_candidates_eos inside the captured step.
EOS_MAX = 8


def eos_list(ids, V: int, device) -> Tensor:
    """The device list the eos-set entries read: int32 [n], 0 <= n <= EOS_MAX, every id in [0, V) -- checked HERE, on the host, because the
    entries cannot read a device list (ValueError).  Duplicates are allowed.  Builds a tensor: call it outside any capture."""
    ids = [int(v) for v in ids]
    if len(ids) > EOS_MAX:
        raise ValueError(f"{len(ids)} eos ids: up to {EOS_MAX} are taken")
    if any(not 0 <= v < V for v in ids):
        raise ValueError(f"eos ids {ids}: every id has to be in [0, {V})")
    return torch.tensor(ids, dtype=torch.int32, device=device)


def pick_greedy(logits: Tensor, step: Tensor, eos_ids: Tensor, fin: Tensor, tok: Tensor, out: Tensor, min_new: int = 0, pad: int = 0) -> Tensor:
    """The greedy emission of one decode step in one launch (vtgb_llm_pick_greedy): logits [B, V] bf16 / fp32, ``step`` device int64,
    ``eos_ids`` device int32 [n <= EOS_MAX] (``eos_list``) -> per row the lowest index of the maximum (torch.argmax), the listed ids at -inf
    while step < min_new; a row with ``fin`` [B] bool set emits ``pad`` and keeps it, another row's ``fin`` is set when its token is listed.
    The token is written to ``tok`` [B] int64 and ``out[:, step]`` ([B, N] int64).  Every operand is the caller's: nothing is allocated, so
    the call can be captured.  Returns ``tok``."""
    _need_cuda(logits, step, eos_ids, fin, tok, out)
    B, V = logits.shape
    N = out.shape[1]
    assert fin.shape == (B,) and tok.shape == (B,) and out.shape == (B, N) and eos_ids.dim() == 1 and step.numel() == 1
    assert fin.dtype == torch.bool and tok.dtype == torch.int64 and out.dtype == torch.int64 and step.dtype == torch.int64 and eos_ids.dtype == torch.int32
    assert logits.is_contiguous() and out.is_contiguous() and tok.is_contiguous() and fin.is_contiguous() and eos_ids.is_contiguous()
    n = eos_ids.numel()
    a = L.LlmPickGreedyArgs(dtype_code(logits.dtype), B, V, N, int(min_new), n, int(pad), _ptr(logits), _ptr(step), _ptr(eos_ids) if n else None,
                            _ptr(fin), _ptr(tok), _ptr(out))
    L.check(L.lib().vtgb_llm_pick_greedy(C.byref(a), _stream()))
    return tok


def beam_candidates_eos(logits: Tensor, seq: Tensor, step: Tensor, running: Tensor, eos_ids: Tensor, repetition_penalty: float = 1.0,
                        min_new: int = 0, out: Optional[Tuple[Tensor, Tensor]] = None, workspace: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """``beam_candidates`` with a device list of eos ids (vtgb_llm_beam_candidates_eos; ``eos_ids`` int32 [n <= EOS_MAX], ``eos_list``): every
    listed id is at -inf while step < min_new.  The workspace is ``beam_candidates_workspace_bytes``; with a one-element list the result equals
    ``beam_candidates``' bit for bit."""
    _need_cuda(logits, seq, step, running, eos_ids)
    R, V = logits.shape
    B, K = running.shape
    N = seq.shape[1]
    assert R == B * K and seq.shape == (R, N) and seq.dtype == torch.int64 and step.dtype == torch.int64 and running.dtype == torch.float32
    assert logits.is_contiguous() and seq.is_contiguous() and running.is_contiguous()
    assert eos_ids.dim() == 1 and eos_ids.dtype == torch.int32 and eos_ids.is_contiguous()
    if out is None:
        out = (torch.empty(B, 2 * K, dtype=torch.float32, device=logits.device), torch.empty(B, 2 * K, dtype=torch.int32, device=logits.device))
    need = beam_candidates_workspace_bytes(R, K, V)
    if workspace is None:
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=logits.device)
    n = eos_ids.numel()
    a = L.LlmBeamCandidatesEosArgs(dtype_code(logits.dtype), R, K, V, N, n, int(min_new), float(repetition_penalty), _ptr(logits),
                                   _ptr(seq) if N else None, _ptr(step), _ptr(running), _ptr(eos_ids) if n else None, _ptr(out[0]), _ptr(out[1]),
                                   _ptr(workspace), workspace.numel() * workspace.element_size())
    L.check(L.lib().vtgb_llm_beam_candidates_eos(C.byref(a), _stream()))
    return out


# ---- repetition penalty on one beam (opt-in: penalty_decode="graph").
def repetition_penalty(logits: Tensor, seq: Tensor, step: Tensor, penalty: float, start_id: Optional[int] = None, out: Optional[Tensor] = None) -> Tensor:
    """HF's RepetitionPenaltyLogitsProcessor on one step's logits (vtgb_llm_repetition_penalty): logits [R, V] bf16 / fp32, ``seq`` [R, N]
    int64, ``step`` device int64 -> fp32 scores [R, V]: x < 0 ? x * penalty : x / penalty at every index among seq[r, :clamp(step, 0, N)] or
    equal to ``start_id`` (an id that is always seen -- T5's decoder start token; None / -1: none), once whatever the repeats, and
    float(logit) elsewhere.  Ids outside [0, V) match no index.  With ``out`` ([R, V] fp32, the caller's) nothing is allocated, so the call
    can be captured.  Returns ``out``."""
    _need_cuda(logits, seq, step, out)
    R, V = logits.shape
    N = seq.shape[1]
    assert seq.shape == (R, N) and seq.dtype == torch.int64 and step.dtype == torch.int64 and step.numel() == 1
    assert logits.is_contiguous() and seq.is_contiguous()
    if out is None:
        out = torch.empty(R, V, dtype=torch.float32, device=logits.device)
    assert out.shape == (R, V) and out.dtype == torch.float32 and out.is_contiguous() and out.data_ptr() != logits.data_ptr()
    a = L.LlmRepetitionPenaltyArgs(dtype_code(logits.dtype), R, V, N, -1 if start_id is None else int(start_id), float(penalty), _ptr(logits),
                                   _ptr(seq), _ptr(step), _ptr(out))
    L.check(L.lib().vtgb_llm_repetition_penalty(C.byref(a), _stream()))
    return out


# ---- beam search on the T5 decode step (opt-in: beam_search="graph+t5").  vtgb_llm_attention_rows_beam keeps its scores and the table rows of a
# (row, head) in LDS: the largest t_pad (= decoder positions of a state) it is launched with, VTGB_LLM_ATTN_ROWS_BEAM_MAX_T of include/vtgb.h.
ATTENTION_ROWS_BEAM_MAX_KEYS = 1920


def attention_rows_beam(q: Tensor, kc: Tensor, vc: Tensor, src_row: Tensor, pos: Tensor, scale: float, bias: Optional[Tensor] = None,
                        out: Optional[Tensor] = None) -> Tensor:
    """The T5 decoder's self-attention of R beam rows through an ancestry table (vtgb_llm_attention_rows_beam): q [R, H*dk]; kc / vc
    [R, H, N, dk], row r holding what beam row r appended; src_row [R, >= N] int32, the cache row that holds row r's key of slot t; keys
    [0, *pos] (device int64) with the bias row *pos of ``bias`` [H, N, N] (None: no bias).  Equals vtgb_llm_attention_rows on the gathered
    caches ``kc[src_row[r, t], :, t]`` bit for bit."""
    _need_cuda(q, kc, vc, src_row, pos)
    R, H, N, dk = kc.shape
    assert q.shape == (R, H * dk) and vc.shape == kc.shape and q.dtype == kc.dtype == vc.dtype and all(t.is_contiguous() for t in (q, kc, vc))
    assert src_row.dtype == torch.int32 and src_row.dim() == 2 and src_row.shape[0] == R and src_row.stride(1) == 1 and pos.dtype == torch.int64
    assert bias is None or (bias.shape == (H, N, N) and bias.dtype == q.dtype and bias.is_contiguous())
    if out is None:
        out = torch.empty(R, H * dk, dtype=q.dtype, device=q.device)
    a = L.LlmAttnRowsArgs(dtype_code(q.dtype), R, H, dk, 1, 0, N, float(scale), _ptr(q), H * dk, _ptr(kc), _ptr(vc), H * N * dk, N * dk, dk,
                          _ptr(bias), N, N * N, _ptr(pos), _ptr(out), H * dk)
    L.check(L.lib().vtgb_llm_attention_rows_beam(C.byref(a), _ptr(src_row), src_row.stride(0), R, _stream()))
    return out


def _lora_args(x: Tensor, y: Tensor, segments, name: str):
    """vtgb_llm_lora_args of both LoRA entries (the wrappers' own shape / dtype checks; the library checks the rest)."""
    _need_cuda(x, y, *(t for _, A, B, _ in segments for t in (A, B)))
    assert x.dim() == 2 and y.dim() == 2 and x.shape[0] == y.shape[0] and x.dtype == y.dtype, f"{name}: x [rows, K] and y [rows, n_cols] of one dtype"
    assert x.stride(1) == 1 and y.stride(1) == 1, f"{name}: unit column stride"
    a = L.LlmLoraArgs(dtype_code(y.dtype), x.shape[1], y.shape[1], len(segments), x.shape[0], x.stride(0), y.stride(0), _ptr(x), _ptr(y))
    for s, (col0, A, B, scaling) in enumerate(segments[:L.LORA_MAX_SEGMENTS]):
        assert A.dtype == B.dtype == torch.float32 and A.is_contiguous() and B.is_contiguous(), f"{name}: fp32 contiguous adapters"
        assert A.dim() == 2 and B.dim() == 2 and A.shape[1] == x.shape[1] and B.shape[1] == A.shape[0], f"{name}: A [r, K], B [n, r]"
        a.seg[s] = L.LlmLoraSeg(_ptr(A), _ptr(B), A.shape[0], B.shape[0], int(col0), float(scaling))
    return a


def lora_update(x: Tensor, y: Tensor, segments) -> Tensor:
    """Unmerged LoRA adapters on a projection's output, in place (vtgb_llm_lora): for every ``(col0, A, B, scaling)`` of ``segments`` (1 .. 4,
    disjoint column ranges), ``y[:, col0 : col0 + n] += ((x.float() @ A.T) @ B.T * scaling).to(y.dtype)`` -- train.LoraLinear.forward in eval
    mode, rounding for rounding.  x [rows, K] and y [rows, n_cols] bf16 or fp32 (the same), unit column stride, any row stride; A [r, K] and
    B [n, r] fp32 contiguous.  Returns ``y``.  The library checks the rest (include/vtgb.h) and raises through ``_lib.check``."""
    a = _lora_args(x, y, segments, "lora_update")
    L.check(L.lib().vtgb_llm_lora(C.byref(a), _stream()))
    return y


def lora_update_parts(x: Tensor, y: Tensor, segments, part: Tensor, n_splits: int) -> Tensor:
    """The K-split reduce of a deferred projection and ``lora_update`` in ONE launch (vtgb_llm_lora_parts): ``part`` and ``n_splits`` > 1 are
    the workspace and split count ``gemm_skinny(x, w, defer_reduce=True)`` returned for the [rows <= 128, n_cols] projection; ``y`` (bf16, as
    x) is written, not read.  Bit for bit ``lora_update(x, gemm_skinny(x, w, n_splits=n_splits), segments)``.  Returns ``y``."""
    a = _lora_args(x, y, segments, "lora_update_parts")
    _need_cuda(part)
    rows, n_cols = y.shape
    need = -(-n_cols // 128) * int(n_splits) * rows * 128 * 4
    assert part.is_contiguous() and part.numel() * part.element_size() >= need, f"lora_update_parts: fragments of {need} bytes"
    L.check(L.lib().vtgb_llm_lora_parts(C.byref(a), _ptr(part), int(n_splits), _stream()))
    return y


def layernorm(x: Tensor, gamma: Tensor, beta: Tensor, eps: float, out_dtype=torch.float32) -> Tensor:
    _need_cuda(x, gamma, beta)
    x = x.contiguous().float()
    M, D = x.numel() // x.shape[-1], x.shape[-1]
    out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    f32_out = out_dtype == torch.float32
    a = L.LayerNormArgs(BF16 if out_dtype == torch.bfloat16 else F32, M, D, float(eps), x.data_ptr(), gamma.data_ptr(),
                        beta.data_ptr(), out.data_ptr() if f32_out else None, None if f32_out else out.data_ptr())
    L.check(L.lib().vtgb_layernorm(C.byref(a), _stream()))
    return out


# ----------------------------------------------------------------------------- weight tables
class _WeightTable:
    """Keeps the (packed) device tensors of one stage alive next to the pointer array the ABI takes."""

    def __init__(self, code: int):
        self.code = code
        self.tensors: List[Optional[Tensor]] = []

    def add(self, t: Optional[Tensor], gemm_weight: bool = False, cols_pad: Optional[int] = None, force_f32: bool = False):
        if t is None:
            self.tensors.append(None)
        elif gemm_weight and not force_f32 and self.code in (BF16X3, F16C8):
            self.tensors.append(_bf16_exact(t.reshape(t.shape[0], -1).float()))      # (already split3: bf16 values)
        elif gemm_weight and not force_f32:
            self.tensors.append(pack_weight(t, self.code, cols_pad))
        else:
            self.tensors.append(t.detach().contiguous().float())

    def finish(self):
        self.array = (C.c_void_p * len(self.tensors))(*[_ptr(t) for t in self.tensors])
        return self

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.tensors if t is not None)


class VitWeights(_WeightTable):
    """model.vision_model.* -> the pointer table of vtgb_vit_forward (include/vtgb.h)."""

    def __init__(self, sd: Dict[str, Tensor], prefix: str, code: int, heads: int, eps: float = 1e-6, fold_ln: bool = True):
        super().__init__(code)
        p = prefix
        pw = sd[p + "embeddings.patch_embedding.weight"]
        self.hidden, _, self.patch, _ = pw.shape
        pos = sd[p + "embeddings.position_embedding"]
        self.tokens = pos.shape[1]
        self.image = int(round(math.sqrt(self.tokens - 1))) * self.patch
        self.heads, self.eps = heads, eps
        kpad = L.lib().vtgb_vit_patch_kpad(code, self.patch)
        self.add(pw, True, kpad)
        self.add(sd[p + "embeddings.patch_embedding.bias"])
        self.add(sd[p + "embeddings.class_embedding"].reshape(-1))
        self.add(pos.reshape(self.tokens, self.hidden))
        self.add(sd[p + "post_layernorm.weight"])
        self.add(sd[p + "post_layernorm.bias"])
        self.layers = 0
        while f"{p}encoder.layers.{self.layers}.self_attn.qkv.weight" in sd:
            lp = f"{p}encoder.layers.{self.layers}."
            folded = code == BF16 and fold_ln      # (then the unfolded qkv / fc1 weights are never read: not uploaded -- ADVICE r5)
            self.add(sd[lp + "layer_norm1.weight"]); self.add(sd[lp + "layer_norm1.bias"])
            self.add(None if folded else sd[lp + "self_attn.qkv.weight"], True); self.add(sd[lp + "self_attn.qkv.bias"])
            self.add(sd[lp + "self_attn.projection.weight"], True); self.add(sd[lp + "self_attn.projection.bias"])
            self.add(sd[lp + "layer_norm2.weight"]); self.add(sd[lp + "layer_norm2.bias"])
            self.add(None if folded else sd[lp + "mlp.fc1.weight"], True); self.add(sd[lp + "mlp.fc1.bias"])
            self.add(sd[lp + "mlp.fc2.weight"], True); self.add(sd[lp + "mlp.fc2.bias"])
            # bf16 mode: the two LayerNorms folded into the GEMMs that follow them (include/vtgb.h: +12 .. +17)
            for lnn, lin in (("layer_norm1", "self_attn.qkv"), ("layer_norm2", "mlp.fc1")):
                if code == BF16 and fold_ln:
                    wl, bl = sd[lp + lin + ".weight"].float(), sd[lp + lin + ".bias"].float()
                    gam, bet = sd[lp + lnn + ".weight"].float(), sd[lp + lnn + ".bias"].float()
                    wf = (wl * gam[None, :]).to(torch.bfloat16)
                    self.tensors.append(wf.contiguous())
                    self.add(wf.float().sum(1))
                    self.add((wl.double() @ bet.double() + bl.double()).float())
                else:
                    self.add(None); self.add(None); self.add(None)
            self.mlp = sd[lp + "mlp.fc1.weight"].shape[0]
            self.layers += 1
        self.finish()


class QFormerWeights(_WeightTable):
    """model.qformer.* (InstructBLIP with text branch, or BLIP-2) -> table of vtgb_qformer_forward."""

    def __init__(self, sd: Dict[str, Tensor], prefix: str, code: int, heads: int, cross_freq: int = 2, eps: float = 1e-12):
        super().__init__(code)
        p = prefix
        self.has_text = (p + "embeddings.word_embeddings.weight") in sd
        self.heads, self.cross_freq, self.eps = heads, cross_freq, eps
        if self.has_text:
            self.add(sd[p + "embeddings.word_embeddings.weight"]); self.add(sd[p + "embeddings.position_embeddings.weight"])
            self.add(sd[p + "embeddings.layernorm.weight"]); self.add(sd[p + "embeddings.layernorm.bias"])
        else:
            self.add(None); self.add(None)
            self.add(sd[p + "layernorm.weight"]); self.add(sd[p + "layernorm.bias"])

        def lin(name):
            w = sd.get(name + ".weight")
            self.add(w, True); self.add(sd.get(name + ".bias"))

        def lnp(name):
            self.add(sd.get(name + ".weight")); self.add(sd.get(name + ".bias"))

        self.layers = 0
        while f"{p}encoder.layer.{self.layers}.attention.attention.query.weight" in sd:
            lp = f"{p}encoder.layer.{self.layers}."
            for nm in ("query", "key", "value"):
                lin(f"{lp}attention.attention.{nm}")
            lin(lp + "attention.output.dense"); lnp(lp + "attention.output.LayerNorm")
            for nm in ("query", "key", "value"):
                lin(f"{lp}crossattention.attention.{nm}")
            lin(lp + "crossattention.output.dense"); lnp(lp + "crossattention.output.LayerNorm")
            lin(lp + "intermediate_query.dense"); lin(lp + "output_query.dense"); lnp(lp + "output_query.LayerNorm")
            lin(lp + "intermediate.dense"); lin(lp + "output.dense"); lnp(lp + "output.LayerNorm")
            self.hidden = sd[lp + "attention.attention.query.weight"].shape[0]
            self.ffn = sd[lp + "intermediate_query.dense.weight"].shape[0]
            if (lp + "crossattention.attention.key.weight") in sd:
                self.enc_hidden = sd[lp + "crossattention.attention.key.weight"].shape[1]
            self.layers += 1
        self.finish()


class TgbWeights(_WeightTable):
    """temporal_encoder.* -> table of vtgb_tgb_forward."""

    def __init__(self, sd: Dict[str, Tensor], prefix: str, code: int, heads: int, fusion_layer: int, eps: float = 1e-12):
        super().__init__(code)
        p = prefix
        self.heads, self.fusion_layer, self.eps = heads, fusion_layer, eps
        t = p + "temporal_embeddings."
        pw = sd[t + "projection.weight"]
        self.hidden, _, self.patch, _ = pw.shape
        self.image = int(round(math.sqrt(sd[t + "fc.weight"].shape[1]))) * self.patch
        self.add(sd[p + "embeddings.word_embeddings.weight"]); self.add(sd[p + "embeddings.token_type_embeddings.weight"])
        self.add(sd[p + "embeddings.LayerNorm.weight"]); self.add(sd[p + "embeddings.LayerNorm.bias"])
        self.add(sd[t + "bos"]); self.add(sd[t + "eos"])
        self.add(pw.reshape(self.hidden, -1)); self.add(sd[t + "projection.bias"])
        self.add(sd[t + "fc.weight"].reshape(-1)); self.add(sd[t + "fc.bias"])
        self.add(sd[t + "frame_pos_embed.weight"])
        self.add(sd[t + "ln.weight"]); self.add(sd[t + "ln.bias"])
        self.add(sd[p + "encoder.embed_positions.weight"]); self.add(sd[p + "encoder.c_embed_positions.weight"])
        self.add(sd[p + "mrc_head.weight"]); self.add(sd[p + "mrc_head.bias"])
        self.max_pos = sd[p + "encoder.embed_positions.weight"].shape[0]

        def lin(name):
            self.add(sd.get(name + ".weight"), True); self.add(sd.get(name + ".bias"))

        def lnp(name):
            self.add(sd.get(name + ".weight")); self.add(sd.get(name + ".bias"))

        self.layers = 0
        while f"{p}encoder.layer.{self.layers}.attention.self.query.weight" in sd:
            lp = f"{p}encoder.layer.{self.layers}."
            for att in ("attention", "crossattention"):
                for nm in ("query", "key", "value"):
                    lin(f"{lp}{att}.self.{nm}")
                lin(f"{lp}{att}.output.dense"); lnp(f"{lp}{att}.output.LayerNorm")
            lin(lp + "intermediate.dense"); lin(lp + "output.dense"); lnp(lp + "output.LayerNorm")
            self.ffn = sd[lp + "intermediate.dense.weight"].shape[0]
            self.layers += 1
        self.finish()


# ----------------------------------------------------------------------------- stages
def vit_forward(w: VitWeights, pixel_values: Tensor, want_f32: bool = True, want_act: bool = False):
    """pixel_values [n, 3, image, image] fp32 -> last_hidden_state [n, tokens, hidden] (fp32 and/or compute dtype)."""
    if pixel_values is None:
        raise ValueError("You have to specify pixel_values")
    _need_cuda(pixel_values)
    pv = pixel_values.contiguous().float()
    n = pv.shape[0]
    if tuple(pv.shape[1:]) != (3, w.image, w.image):
        raise ValueError(f"vit: pixel_values {tuple(pv.shape)} does not match image size {w.image}")
    dev = pv.device
    out32 = torch.empty(n, w.tokens, w.hidden, dtype=torch.float32, device=dev) if want_f32 else None
    outa = torch.empty(n, w.tokens, w.hidden, dtype=act_dtype(w.code), device=dev) if want_act else None
    a = L.VitArgs(w.code, n, w.image, w.patch, w.hidden, w.heads, w.mlp, w.layers, float(w.eps), pv.data_ptr(),
                  C.cast(w.array, C.POINTER(C.c_void_p)), _ptr(out32), _ptr(outa), None, 0)
    need = L.lib().vtgb_vit_workspace_bytes(C.byref(a))
    ws = _ws.get(need, dev)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    L.check(L.lib().vtgb_vit_forward(C.byref(a), _stream()))
    return out32, outa


def qformer_forward(w: QFormerWeights, query_tokens: Tensor, image_embeds: Tensor, text_ids: Optional[Tensor] = None,
                    text_mask: Optional[Tensor] = None, image_mask: Optional[Tensor] = None) -> Tensor:
    """image_embeds [n, tokens, enc_hidden] in the compute dtype -> query rows [n, n_query, hidden] fp32."""
    _need_cuda(image_embeds, query_tokens)
    ie = image_embeds.contiguous()
    if ie.dtype != act_dtype(w.code):
        ie = ie.to(act_dtype(w.code))
    n, enc_tokens, enc_hidden = ie.shape
    qt = query_tokens.reshape(-1, query_tokens.shape[-1]).contiguous().float()
    nq = qt.shape[0]
    nt = 0
    if w.has_text and text_ids is not None:
        text_ids = text_ids.contiguous().to(torch.int64)
        nt = text_ids.shape[1]
        if text_mask is not None:
            text_mask = text_mask.contiguous().to(torch.int64)
    else:
        text_ids = text_mask = None
    if image_mask is not None:
        image_mask = image_mask.contiguous().to(torch.int64)
    out = torch.empty(n, nq, w.hidden, dtype=torch.float32, device=ie.device)
    a = L.QFormerArgs(w.code, n, nq, nt, w.hidden, w.heads, w.ffn, w.layers, w.cross_freq, enc_tokens, enc_hidden,
                      1 if (w.has_text and nt > 0) else 0, float(w.eps), ie.data_ptr(), qt.data_ptr(), _ptr(text_ids),
                      _ptr(text_mask), _ptr(image_mask), C.cast(w.array, C.POINTER(C.c_void_p)), out.data_ptr(), None, 0)
    need = L.lib().vtgb_qformer_workspace_bytes(C.byref(a))
    ws = _ws.get(need, ie.device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    L.check(L.lib().vtgb_qformer_forward(C.byref(a), _stream()))
    return out


def pool_project(query_out: Tensor, widths: Sequence[int], proj_w: Tensor, proj_b: Tensor, mode: str, code: int) -> Tensor:
    """query_out [sum(widths), n_query, hidden] fp32; proj_w packed for `code` -> LLM prefix tokens (fp32)."""
    _need_cuda(query_out, proj_w)
    if mode not in ("mean", "concat"):
        raise ValueError(f"INVALID POOL MODE: {mode}")
    qo = query_out.contiguous().float()
    total, nq, hidden = qo.shape
    if sum(widths) != total:
        raise ValueError(f"pool_project: widths sum {sum(widths)} != {total} frames")
    n_clips = len(widths)
    out_dim = proj_w.shape[0]
    if mode == "mean":
        out = torch.empty(n_clips, nq, out_dim, dtype=torch.float32, device=qo.device)
    else:
        out = torch.empty(total * nq, out_dim, dtype=torch.float32, device=qo.device)
    wd = (C.c_int32 * n_clips)(*[int(x) for x in widths])
    a = L.PoolProjectArgs(code, n_clips, nq, hidden, out_dim, L.POOL_MEAN if mode == "mean" else L.POOL_CONCAT, qo.data_ptr(),
                          C.cast(wd, C.POINTER(C.c_int32)), proj_w.data_ptr(), proj_b.data_ptr(), out.data_ptr(), None, 0)
    need = L.lib().vtgb_pool_project_workspace_bytes(C.byref(a))
    ws = _ws.get(need, qo.device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    L.check(L.lib().vtgb_pool_project(C.byref(a), _stream()))
    if mode == "concat":
        if len(set(widths)) != 1:
            raise ValueError("concat pooling needs equal widths")
        out = out.reshape(n_clips, -1, out_dim)
    return out


def tgb_forward(w: TgbWeights, of: Tensor, of_mask: Tensor, text_ids: Tensor, text_mask: Tensor, mode: str):
    """of [B, L, 2, image, image] fp32 -> (sequence_output [B, L+2, hidden], logits [B, L, 2]) fp32."""
    if mode not in L.TGB_MODE:
        raise ValueError(f"INVALID MODE: {mode}")
    _need_cuda(of, of_mask, text_ids, text_mask)
    of = of.contiguous().float()
    B, Lf = of.shape[:2]
    if tuple(of.shape[2:]) != (2, w.image, w.image):
        raise ValueError(f"tgb: flow {tuple(of.shape)} does not match image size {w.image}")
    if Lf + 2 > w.max_pos:
        raise ValueError(f"tgb: {Lf} flow frames exceed the {w.max_pos} position table")
    of_mask = of_mask.contiguous().to(torch.int64)
    text_ids = text_ids.contiguous().to(torch.int64)
    text_mask = text_mask.contiguous().to(torch.int64)
    seq = torch.empty(B, Lf + 2, w.hidden, dtype=torch.float32, device=of.device)
    logits = torch.empty(B, Lf, 2, dtype=torch.float32, device=of.device)
    a = L.TgbArgs(w.code, B, Lf, text_ids.shape[1], w.hidden, w.heads, w.ffn, w.layers, w.fusion_layer, L.TGB_MODE[mode],
                  w.image, w.patch, float(w.eps), of.data_ptr(), of_mask.data_ptr(), text_ids.data_ptr(), text_mask.data_ptr(),
                  C.cast(w.array, C.POINTER(C.c_void_p)), seq.data_ptr(), logits.data_ptr(), None, 0)
    need = L.lib().vtgb_tgb_workspace_bytes(C.byref(a))
    ws = _ws.get(need, of.device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    L.check(L.lib().vtgb_tgb_forward(C.byref(a), _stream()))
    return seq, logits


class TgbTrunk:
    """One clip's question-independent TGB state (vtgb_tgb_trunk): the residual stream after the layers before the first cross-attention
    layer, fp32 ``H`` and its compute-dtype copy ``Hb`` [L+2, hidden]; ``of_mask`` [1, L+2] the clip's flow mask; ``mode`` / ``code`` the
    TGB mode and compute dtype it was built at (tgb_resume checks both)."""

    def __init__(self, H: Tensor, Hb: Tensor, of_mask: Tensor, mode: str, code: int):
        self.H, self.Hb, self.of_mask, self.mode, self.code = H, Hb, of_mask, mode, code

    @property
    def L(self) -> int:
        return self.H.shape[0] - 2


def _tgb_split_args(w: TgbWeights, B: int, Lf: int, n_text: int, mode: str) -> "L.TgbSplitArgs":
    return L.TgbSplitArgs(w.code, B, Lf, n_text, w.hidden, w.heads, w.ffn, w.layers, w.fusion_layer, L.TGB_MODE[mode], w.image, w.patch,
                          float(w.eps), None, None, None, None, C.cast(w.array, C.POINTER(C.c_void_p)), None, None, None, None, None, 0)


def tgb_trunk(w: TgbWeights, of: Tensor, of_mask: Tensor, mode: str) -> TgbTrunk:
    """of [1, L, 2, image, image] fp32 (one clip), of_mask [1, L+2] -> the clip's TgbTrunk (vtgb_tgb_trunk)."""
    if mode not in L.TGB_MODE:
        raise ValueError(f"INVALID MODE: {mode}")
    _need_cuda(of, of_mask)
    of = of.contiguous().float()
    if of.dim() != 5 or of.shape[0] != 1:
        raise ValueError(f"tgb_trunk: flow {tuple(of.shape)} is not one clip [1, L, 2, image, image]")
    Lf = of.shape[1]
    if tuple(of.shape[2:]) != (2, w.image, w.image):
        raise ValueError(f"tgb: flow {tuple(of.shape)} does not match image size {w.image}")
    if Lf + 2 > w.max_pos:
        raise ValueError(f"tgb: {Lf} flow frames exceed the {w.max_pos} position table")
    of_mask = of_mask.contiguous().to(torch.int64)
    if tuple(of_mask.shape) != (1, Lf + 2):
        raise ValueError(f"tgb_trunk: of_mask {tuple(of_mask.shape)} != (1, {Lf + 2})")
    H = torch.empty(Lf + 2, w.hidden, dtype=torch.float32, device=of.device)
    Hb = torch.empty(Lf + 2, w.hidden, dtype=act_dtype(w.code), device=of.device)
    a = _tgb_split_args(w, 1, Lf, 0, mode)
    a.of, a.of_mask, a.trunk, a.trunk_act = of.data_ptr(), of_mask.data_ptr(), H.data_ptr(), Hb.data_ptr()
    need = L.lib().vtgb_tgb_trunk_workspace_bytes(C.byref(a))
    ws = _ws.get(need, of.device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    L.check(L.lib().vtgb_tgb_trunk(C.byref(a), _stream()))
    return TgbTrunk(H, Hb, of_mask, mode, w.code)


def tgb_resume(w: TgbWeights, trunk: TgbTrunk, text_ids: Tensor, text_mask: Tensor):
    """B question rows against one clip's trunk (vtgb_tgb_resume) -> (sequence_output [B, L+2, hidden], logits [B, L, 2]) fp32, equal bit for
    bit to tgb_forward on the clip repeated B times."""
    if trunk.code != w.code:
        raise ValueError(f"tgb_resume: trunk built at compute dtype {trunk.code}, weights at {w.code}")
    _need_cuda(text_ids, text_mask)
    text_ids = text_ids.contiguous().to(torch.int64)
    text_mask = text_mask.contiguous().to(torch.int64)
    if text_ids.dim() != 2 or tuple(text_mask.shape) != tuple(text_ids.shape):
        raise ValueError(f"tgb_resume: text_ids {tuple(text_ids.shape)} / text_mask {tuple(text_mask.shape)} mismatch")
    B, Lf = text_ids.shape[0], trunk.L
    seq = torch.empty(B, Lf + 2, w.hidden, dtype=torch.float32, device=text_ids.device)
    logits = torch.empty(B, Lf, 2, dtype=torch.float32, device=text_ids.device)
    a = _tgb_split_args(w, B, Lf, text_ids.shape[1], trunk.mode)
    a.of_mask, a.text_ids, a.text_mask = trunk.of_mask.data_ptr(), text_ids.data_ptr(), text_mask.data_ptr()
    a.trunk, a.trunk_act, a.seq_out, a.logits = trunk.H.data_ptr(), trunk.Hb.data_ptr(), seq.data_ptr(), logits.data_ptr()
    need = L.lib().vtgb_tgb_resume_workspace_bytes(C.byref(a))
    ws = _ws.get(need, text_ids.device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    L.check(L.lib().vtgb_tgb_resume(C.byref(a), _stream()))
    return seq, logits


# ----------------------------------------------------------------------------- RAFT (a2 / f1)
def conv_k_order(w: Tensor) -> Tensor:
    """[co, kh, kw, ci] (ci % 64 == 0) -> [co, K] in the implicit-GEMM kernels' K order: 64-channel chunk major,
    tap minor (the taps of one channel slab are gathered back to back, see gemm.hip / conv_f32.hip)."""
    co, kh, kw, ci = w.shape
    return w.reshape(co, kh * kw, ci // 64, 64).permute(0, 2, 1, 3).reshape(co, -1).contiguous()


def _bf16_parts(w: Tensor) -> Tuple[Tensor, Tensor]:
    """w fp32 -> (hi, lo) as fp32 tensors holding bf16 values: hi = bf16(w), lo = bf16(w - hi)."""
    hi = w.to(torch.bfloat16).float()
    return hi, (w - hi).to(torch.bfloat16).float()


def split3(w: Tensor, sources: Optional[Sequence[int]] = None) -> Tensor:
    """[co, kh, kw, ci] fp32 -> [co, kh, kw, 3 ci] for the bf16x3 contraction: per source of the (virtual) channel concatenation the
    channel blocks [Wh | Wh | Wl], which meet the activation pair read as [hi | lo | hi] (GemmDesc::conv_wrap)."""
    ci = w.shape[-1]
    out, c0 = [], 0
    for c in (sources or [ci]):
        hi, lo = _bf16_parts(w[..., c0:c0 + c])
        out += [hi, hi, lo]
        c0 += c
    assert c0 == ci
    return torch.cat(out, -1)


H8_LO_SCALE = 2048.0      # csrc/pair_h8.h


def h8_weight_scale(w: Tensor) -> Tuple[float, int]:
    """(sw, E8M0 byte of 2^-11 / sw): sw = the largest power of two with max |w| sw <= 448 (e4m3's largest finite value)."""
    import math
    m = float(w.abs().max())
    e = 0 if m == 0.0 else math.floor(math.log2(448.0 / m))
    e = max(min(e, 100), -100)
    return 2.0 ** e, 127 - 11 - e


def h8_conv_pack(w: Tensor, sw: float, sources: Optional[Sequence[int]] = None) -> Tensor:
    """[co, kh, kw, ci] fp32 -> [co, K] bf16-typed 16-bit units for the f16c8 contraction (csrc/pair_h8.h, gemm_h8.hip): per source of the (virtual)
    channel concatenation the K order is [fp16(w): taps x C | correction bytes: taps x C], each half 64-channel chunk major / tap minor; the
    correction bytes of channels 4g .. 4g+3 are (Wh8 x 4, Wl' x 4) -- under the activations' (xl' x 4, xh8 x 4)."""
    co, kh, kw, ci = w.shape
    out, c0 = [], 0
    for c in (sources or [ci]):
        ws = w[..., c0:c0 + c].float()
        wh = ws.to(torch.float16)
        wl = ws - wh.float()
        h8 = (ws * sw).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)                      # [co, kh, kw, c]
        l8 = (wl * (sw * H8_LO_SCALE)).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
        corr = torch.stack([h8.reshape(co, kh, kw, c // 4, 4), l8.reshape(co, kh, kw, c // 4, 4)], -2)      # [.., c/4, {Wh8, Wl'}, 4]
        corr16 = corr.reshape(co, kh, kw, 2 * c).contiguous().view(torch.int16)                             # [co, kh, kw, c] 16-bit units
        out += [conv_k_order(wh.view(torch.int16)), conv_k_order(corr16)]
        c0 += c
    assert c0 == ci
    return torch.cat(out, 1).contiguous().view(torch.bfloat16)


def flow_tail_pack(w2: Tensor) -> Tensor:
    """FlowHead.conv2 as the 1x1 tail of conv1's f16c8 launch: w2 [32 (tap * 2 + c, zero-padded), 256] fp32 -> [wn 4][i 4][lane 64][e 4][ob 2] fp32 with
    the value W2[channel = 64 wn + 16 i + 4 (lane >> 4) + e][out = 16 ob + (lane & 15)] -- eight consecutive floats per (wn, i, lane)."""
    t = w2.float().t().contiguous()                                    # [256 channels, 32 outs]
    t = t.reshape(4, 4, 4, 4, 2, 16)                                   # [wn, i, fg, e, ob, fr]
    return t.permute(0, 1, 2, 5, 3, 4).contiguous().reshape(-1)        # [wn, i, fg, fr, e, ob]


def _bf16_exact(w: Tensor) -> Tensor:
    """fp32 holding bf16 values -> bf16 (exact)."""
    return w.contiguous().to(torch.bfloat16)


def pair_pack(x: Tensor, fmt: int = F16C8, ld_pair: Optional[int] = None) -> Tensor:
    """x [M, C] fp32 -> pair rows (include/vtgb.h vtgb_pair_pack) as an int16 tensor [M, 2 * ld_pair]."""
    _need_cuda(x)
    x = x.contiguous().float()
    M, Cc = x.shape
    ld = ld_pair or Cc
    out = torch.empty(M, 2 * ld, dtype=torch.int16, device=x.device)
    L.check(L.lib().vtgb_pair_pack(fmt, x.data_ptr(), out.data_ptr(), M, Cc, ld, _stream()))
    return out


def pair_unpack(rows: Tensor, C_: int, fmt: int = F16C8) -> Tensor:
    """The fp32 values pair rows stand for where they are read back element-wise: f16c8 xh + xl' 2^-11 (csrc/pair_h8.h), bf16x3 hi + lo."""
    M, two_ld = rows.shape
    ld = two_ld // 2
    if fmt == BF16X3:
        v = rows.view(torch.bfloat16).float()
        return v[:, :C_] + v[:, ld:ld + C_]
    hi = rows[:, :C_].contiguous().view(torch.float16).float()
    lo = rows[:, ld:].contiguous().view(torch.uint8).reshape(M, ld // 4, 2, 4)[:, :, 0].reshape(M, ld)[:, :C_].contiguous()
    return hi + lo.view(torch.float8_e5m2).float() / H8_LO_SCALE


def pair_conv(a: Tensor, w: Tensor, sw: float, H: int, W: int, a2: Optional[Tensor] = None, bias: Optional[Tensor] = None, relu: bool = False,
              out_fmt: int = F16C8, ld_out: Optional[int] = None, resid: Optional[Tensor] = None, tail_w: Optional[Tensor] = None,
              out_f32: bool = False) -> Tensor:
    """One 'same' convolution over f16c8 pair rows (include/vtgb.h vtgb_pair_conv / vtgb_pair_conv_ex): a [M, 2 C1] int16 pair rows (pair_pack),
    w [co, kh, kw, ci] fp32 with ci = C1 (x 2 with a2), sw from h8_weight_scale(w) -> pair rows [M, 2 * ld_out] int16.  resid (f16c8 pair rows of the
    output's layout): the ResidualBlock tail relu(resid + act(conv)); tail_w ([32, 256] fp32, co == 256): returns the [M, 32] fp32 products with it
    instead; out_f32: returns fp32 rows [M, ld_out] instead."""
    _need_cuda(a, w)
    co, kh, kw, ci = w.shape
    C1 = a.shape[1] // 2
    assert ci == C1 * (2 if a2 is not None else 1)
    _, byte = h8_weight_scale(w)
    packed = h8_conv_pack(w, sw, [C1, C1] if a2 is not None else None)
    scale = torch.tensor([byte], dtype=torch.int32, device=a.device)
    ld = ld_out or ((co + 3) // 4 * 4)
    out = torch.zeros(a.shape[0], 2 * ld, dtype=torch.int16, device=a.device)
    bias_t = None if bias is None else bias.contiguous().float()
    args = L.PairConvArgs(a.shape[0], co, H, W, kh, kw, C1, a.data_ptr(), _ptr(a2), packed.data_ptr(), scale.data_ptr(), _ptr(bias_t),
                          1 if relu else 0, out_fmt, out.data_ptr(), ld)
    if resid is None and tail_w is None and not out_f32:
        L.check(L.lib().vtgb_pair_conv(C.byref(args), _stream()))
        torch.cuda.current_stream().synchronize()      # (packed / scale are temporaries of this call)
        return out
    tail_p = tail_out = f32 = None
    if tail_w is not None:
        tail_p = flow_tail_pack(tail_w.to(a.device))
        tail_out = torch.zeros(a.shape[0], 32, dtype=torch.float32, device=a.device)
    if out_f32:
        f32 = torch.zeros(a.shape[0], ld, dtype=torch.float32, device=a.device)
    ex = L.PairConvExArgs(args, _ptr(resid), ld, _ptr(tail_p), _ptr(tail_out), _ptr(f32), ld)
    L.check(L.lib().vtgb_pair_conv_ex(C.byref(ex), _stream()))
    torch.cuda.current_stream().synchronize()
    return tail_out if tail_w is not None else f32 if out_f32 else out


def raft_lookup_convc1(pyramid: Sequence[Tensor], flow: Tensor, w: Tensor, bias: Tensor, H8: int, W8: int, variant: int = 1,
                       want_occupancy: bool = False):
    """vtgb_raft_update's fused f16c8 launch alone (include/vtgb.h vtgb_raft_lookup_convc1): pyramid = 4 fp32 levels [M, H8 >> l, W8 >> l], flow [M, 2]
    fp32, w [256, 324] fp32 (convc1), bias [256] -> c1 as f16c8 pair rows [M, 512] int16 (pair_unpack(., 256) gives the values).  variant 1: the
    split-K tile of the product; 0: the whole-K tile it replaced.  want_occupancy: returns (rows, resident workgroups per CU of that instantiation)."""
    _need_cuda(flow, *pyramid)
    M = flow.shape[0]
    assert M % (H8 * W8) == 0 and flow.shape == (M, 2) and w.shape == (256, 324) and len(pyramid) == 4
    lv = [p.contiguous().float() for p in pyramid]
    for l, p in enumerate(lv):
        assert p.numel() == M * (H8 >> l) * (W8 >> l)
    wk = torch.zeros(256, 1, 1, 384, dtype=torch.float32, device=flow.device)
    wk[:, 0, 0, :324] = w.to(flow.device).float()
    sw, byte = h8_weight_scale(wk)
    packed = h8_conv_pack(wk, sw)
    scale = torch.tensor([byte], dtype=torch.int32, device=flow.device)
    fl, bias_t = flow.contiguous().float(), bias.to(flow.device).contiguous().float()
    out = torch.zeros(M, 512, dtype=torch.int16, device=flow.device)
    occ = L.i32(0)
    args = L.RaftLookupConvc1Args(M // (H8 * W8), H8, W8, variant, (L.vp * 4)(*[p.data_ptr() for p in lv]), fl.data_ptr(), packed.data_ptr(), scale.data_ptr(),
                                  bias_t.data_ptr(), out.data_ptr(), C.pointer(occ) if want_occupancy else None)
    L.check(L.lib().vtgb_raft_lookup_convc1(C.byref(args), _stream()))
    torch.cuda.current_stream().synchronize()      # (packed / scale are temporaries of this call)
    return (out, occ.value) if want_occupancy else out


def raft_gru_half(fmt: int, h: Tensor, x: Tensor, start_zr: Optional[Tensor], start_q: Optional[Tensor], w_zr: Optional[Tensor], w_q: Optional[Tensor],
                  H8: int, W8: int, half: int, stage: int = 2, rh: Optional[Tensor] = None, z: Optional[Tensor] = None, h_q: Optional[Tensor] = None):
    """One SepConvGRU half-step of vtgb_raft_update's refinement loop alone (include/vtgb.h vtgb_raft_gru_half; fmt F16C8 or BF16X3): h, x = [motion | flow]
    pair rows [M, 256] int16 (pair_pack), start maps fp32 [M, 256] / [M, 128], w_zr [256, kh, kw, 256] / w_q [128, kh, kw, 256] fp32 over the input
    channels [h | x] with (kh, kw) = (1, 5) for half 0, (5, 1) for half 1 -- packed here the way RaftWeights packs the table.  stage 0: the z | r launch
    writes z (fp32 [M, 128]) and rh (pair rows); stage 1: the q launch reads them and updates h_q IN PLACE (default: h itself, as the loop does);
    stage 2: both.  Returns (z, rh, h_q); operands of a launch that does not run may be None."""
    _need_cuda(h, x)
    M, dev = h.shape[0], h.device
    assert M % (H8 * W8) == 0 and h.shape == (M, 256) and x.shape == (M, 256) and h.dtype == torch.int16 and x.dtype == torch.int16
    assert h.is_contiguous() and x.is_contiguous()
    kh, kw = (1, 5) if half == 0 else (5, 1)
    keep = []

    def pack(w, co):
        if w is None:
            return None, None
        assert tuple(w.shape) == (co, kh, kw, 256)
        w = w.to(dev).float()
        if fmt == F16C8:
            sw, byte = h8_weight_scale(w)
            keep.append(torch.tensor([byte], dtype=torch.int32, device=dev))
            keep.append(h8_conv_pack(w, sw, [128, 128]))
            return keep[-1], keep[-2]
        keep.append(_bf16_exact(conv_k_order(split3(w, [128, 128]))))
        return keep[-1], None

    pzr, szr = pack(w_zr, 256)
    pq, sq = pack(w_q, 128)
    rh = torch.zeros(M, 256, dtype=torch.int16, device=dev) if rh is None else rh
    z = torch.zeros(M, 128, dtype=torch.float32, device=dev) if z is None else z
    h_q = h if h_q is None else h_q
    for t, shape, dt in ((rh, (M, 256), torch.int16), (z, (M, 128), torch.float32), (h_q, (M, 256), torch.int16), (start_zr, (M, 256), torch.float32),
                         (start_q, (M, 128), torch.float32)):
        assert t is None or (tuple(t.shape) == shape and t.dtype == dt and t.is_contiguous() and t.device == dev)
    args = L.RaftGruHalfArgs(fmt, M // (H8 * W8), H8, W8, half, stage, h.data_ptr(), h_q.data_ptr(), x.data_ptr(), rh.data_ptr(), z.data_ptr(), _ptr(start_zr),
                             _ptr(start_q), _ptr(pzr), _ptr(pq), _ptr(szr), _ptr(sq))
    L.check(L.lib().vtgb_raft_gru_half(C.byref(args), _stream()))
    torch.cuda.current_stream().synchronize()      # (the packed weights / scales are temporaries of this call)
    return z, rh, h_q


def conv_launch(code: int, a: Tensor, w: Tensor, n_images: int, H: int, W: int, a2: Optional[Tensor] = None, bias: Optional[Tensor] = None, act: int = 0,
                stride: int = 1, in_hw: Optional[Tuple[int, int]] = None, site: int = L.CONV_SITE_UPDATE, out_kind: int = L.CONV_OUT_F32,
                ld_out: Optional[int] = None, out: Optional[Tensor] = None, moments: bool = False, resid: Optional[Tensor] = None, post_relu: bool = False,
                tail_w: Optional[Tensor] = None, out_scale: float = 0.0):
    """One implicit-GEMM convolution launch of RAFT at ``code`` = BF16X3 / BF16 / F32 alone (include/vtgb.h vtgb_conv_launch), on the H x W output grid of
    n_images images.  a (and a2, a virtual channel concatenation): contiguous rows of the input grid ``in_hw`` (default the output grid) -- int16 pair rows
    [M_in, 2 C] (pair_pack(., BF16X3)) at BF16X3, bf16 [M_in, C] at BF16, fp32 at F32.  w [co, kh, kw, ci] fp32, packed here the way the production tables
    pack it (conv_k_order; split3 per source at BF16X3).  site: L.CONV_SITE_ENCODER / L.CONV_SITE_UPDATE = whose descriptor builder runs.  out_kind
    CONV_OUT_F32 -> fp32 rows [M, ld_out]; CONV_OUT_PAIR_BF16 / CONV_OUT_PAIR_F16C8 -> int16 pair rows [M, 2 ld_out] (pair_unpack); CONV_OUT_BF16 -> bf16
    rows.  ``out``: write into this 2-D tensor (unit column stride; its row stride is ld_out) instead of a fresh one.  moments: also returns the
    [n_images, co, 2] per-image (sum, sum of squares).  resid (bf16 rows) / post_relu: the ResidualBlock tail; tail_w [32, 256] fp32: returns the fused
    1x1 tail's [M, 32] fp32 instead."""
    _need_cuda(a, a2)
    dev = a.device
    co, kh, kw, ci = w.shape
    width = {BF16X3: 2, BF16: 1, F32: 1}[code]
    adt = {BF16X3: torch.int16, BF16: torch.bfloat16, F32: torch.float32}[code]
    C1 = a.shape[1] // width
    C2 = 0 if a2 is None else a2.shape[1] // width
    Hi, Wi = in_hw or (H, W)
    M = n_images * H * W
    for t in (a, a2):
        assert t is None or (t.dtype == adt and t.is_contiguous() and t.shape[0] == n_images * Hi * Wi)
    assert ci == C1 + C2
    w = w.to(dev).float()
    if code == BF16X3:
        packed = _bf16_exact(conv_k_order(split3(w, [C1, C2] if a2 is not None else None)))
    else:
        packed = conv_k_order(w).to(act_dtype(code)).contiguous()
    bias_t = None if bias is None else bias.to(dev).contiguous().float()
    pair = out_kind in (L.CONV_OUT_PAIR_BF16, L.CONV_OUT_PAIR_F16C8)
    if out is None:
        ld = ld_out or ((co + 7) // 8 * 8)
        odt = torch.int16 if pair else torch.bfloat16 if out_kind == L.CONV_OUT_BF16 else torch.float32
        out = torch.zeros(M, (2 if pair else 1) * ld, dtype=odt, device=dev)
    else:
        assert out.dim() == 2 and out.shape[0] == M and out.stride(1) == 1 and out.shape[1] >= co and not pair
        ld = out.stride(0)
    mom = part = None
    if moments:
        mom = torch.zeros(n_images, co, 2, dtype=torch.float32, device=dev)
        part = torch.zeros((M // 256 + 2) * 128 * 4, dtype=torch.float32, device=dev)
    tail_p = tail_out = None
    if tail_w is not None:
        tail_p = tail_w.to(dev).to(torch.bfloat16).contiguous()
        assert tuple(tail_p.shape) == (32, 256)
        tail_out = torch.zeros(M, 32, dtype=torch.float32, device=dev)
    if resid is not None:
        assert resid.dtype == torch.bfloat16 and resid.dim() == 2 and resid.shape[0] == M and resid.stride(1) == 1
    args = L.ConvLaunchArgs(code, out_kind, site, n_images, H, W, kh, kw, stride, Hi, Wi, C1, C2, co, act, 1 if post_relu else 0, out_scale, a.data_ptr(),
                            _ptr(a2), packed.data_ptr(), _ptr(bias_t), out.data_ptr(), ld, _ptr(mom), _ptr(part), 0 if part is None else part.numel(),
                            _ptr(resid), 0 if resid is None else resid.stride(0), _ptr(tail_p), _ptr(tail_out))
    L.check(L.lib().vtgb_conv_launch(C.byref(args), _stream()))
    torch.cuda.current_stream().synchronize()      # (the packed weights are temporaries of this call)
    res = tail_out if tail_w is not None else out
    return (res, mom) if moments else res


class RaftWeights(_WeightTable):
    """of_extractor.update_block.* -> the packed table of vtgb_raft_update ([C_out, KH, KW, C_in] in the compute dtype)."""

    def __init__(self, sd: Dict[str, Tensor], prefix: str = "update_block.", code: int = BF16, hoist_inp: Optional[bool] = None):
        super().__init__(code)
        p = prefix
        if code in (BF16X3, F16C8):
            self._init_x3(sd, p, h8=(code == F16C8))
            return
        # bf16 mode: split the loop-invariant `inp` channels (128..255) out of the GRU convolutions (include/vtgb.h [26..29])
        self.hoist_inp = (code == BF16) if hoist_inp is None else (hoist_inp and code == BF16)

        def conv(name, cin_pad=None, channels=None):
            w = sd[p + name + ".weight"].float()
            if channels is not None:
                w = w[:, channels]
            co, ci, kh, kw = w.shape
            w = w.permute(0, 2, 3, 1)                       # [co, kh, kw, ci]
            if cin_pad and cin_pad != ci:
                w = torch.nn.functional.pad(w, (0, cin_pad - ci))
            return conv_k_order(w)

        def add_conv(name, cin_pad=None):
            self.add(conv(name, cin_pad), True)
            self.add(sd[p + name + ".bias"])

        add_conv("encoder.convc1", 384)
        add_conv("encoder.convc2")
        if code == BF16:
            # convf1 on the matrix cores: k = tap * 4 + {x, y, x, y} (flow head | flow remainder), 49 taps padded to 56
            wf = sd[p + "encoder.convf1.weight"].float().reshape(128, 2, 49).permute(0, 2, 1)         # [co, tap, c]
            wf = torch.nn.functional.pad(torch.cat([wf, wf], 2), (0, 0, 0, 7))                        # [co, 56, 4]
            self.add(wf.reshape(128, 224).contiguous(), True)
        else:
            # exactness mode: plain fp32 FMAs over the 98 taps; [98, 128], k = c * 49 + ky * 7 + kx
            self.add(sd[p + "encoder.convf1.weight"].float().reshape(128, 98).t().contiguous(), True)
        self.add(sd[p + "encoder.convf1.bias"])
        add_conv("encoder.convf2")
        add_conv("encoder.conv")
        dyn = (list(range(0, 128)) + list(range(256, 384))) if self.hoist_inp else None     # [h | motion + flow]
        for sfx in ("1", "2"):
            self.add(torch.cat([conv("gru.convz" + sfx, channels=dyn), conv("gru.convr" + sfx, channels=dyn)], 0), True)
            self.add(torch.cat([sd[p + "gru.convz" + sfx + ".bias"], sd[p + "gru.convr" + sfx + ".bias"]], 0))
            self.add(conv("gru.convq" + sfx, channels=dyn), True)
            self.add(sd[p + "gru.convq" + sfx + ".bias"])
        add_conv("flow_head.conv1")
        # flow_head.conv2 as a GEMM with the taps on the output side: row tap*2 + o = w[o, :, ky, kx]; 18 rows padded to 32
        w2 = sd[p + "flow_head.conv2.weight"].float().permute(2, 3, 0, 1).reshape(18, 256)
        self.add(torch.nn.functional.pad(w2, (0, 0, 0, 14)).contiguous(), True)
        self.add(sd[p + "flow_head.conv2.bias"])
        add_conv("mask.0")
        add_conv("mask.2")
        inp = list(range(128, 256))
        for sfx in ("1", "2"):
            if self.hoist_inp:
                self.add(torch.cat([conv("gru.convz" + sfx, channels=inp), conv("gru.convr" + sfx, channels=inp)], 0), True)
                self.add(conv("gru.convq" + sfx, channels=inp), True)
            else:
                self.add(None); self.add(None)
        self.finish()

    def _init_x3(self, sd: Dict[str, Tensor], p: str, h8: bool = False) -> None:
        """The bf16x3 table (raft_x3.hip): every MFMA convolution as [C_out, taps, 3 C_in] in the kernels' K order with the channel blocks
        [Wh | Wh | Wl] per source; convf1 as in the fp32 mode; the mask head's 0.25 (update.py:143) folded into mask.2 (a power of two: exact).
        ``h8`` (VTGB_F16C8): the nine large convolutions and convf2 in the f16c8 operand format instead (h8_conv_pack) and entry [30] = their scale bytes."""
        self.hoist_inp = True
        scales = []

        def raw(name, cin_pad=None, scale=1.0, channels=None):
            w = sd[p + name + ".weight"].float() * scale
            if channels is not None:
                w = w[:, channels]
            co, ci, kh, kw = w.shape
            w = w.permute(0, 2, 3, 1)
            if cin_pad and cin_pad != ci:
                w = torch.nn.functional.pad(w, (0, cin_pad - ci))
            return w

        def conv(name, cin_pad=None, sources=None, scale=1.0, channels=None):
            return _bf16_exact(conv_k_order(split3(raw(name, cin_pad, scale, channels), sources)))

        def big(ws, sources=None):
            """one large convolution (the rows of `ws` stacked along C_out) in the mode's operand format"""
            if not h8:
                return torch.cat([_bf16_exact(conv_k_order(split3(w, sources))) for w in ws], 0).contiguous()
            sw, byte = h8_weight_scale(torch.cat([w.reshape(-1) for w in ws]))
            scales.append(byte)
            return torch.cat([h8_conv_pack(w, sw, sources) for w in ws], 0).contiguous()

        def add_big(name, cin_pad=None):
            self.tensors.append(big([raw(name, cin_pad)]))
            self.add(sd[p + name + ".bias"].float())

        def add_conv(name, cin_pad=None, scale=1.0):
            self.tensors.append(conv(name, cin_pad, scale=scale))
            self.add(sd[p + name + ".bias"].float() * scale)

        add_big("encoder.convc1", 384)
        add_big("encoder.convc2")
        self.add(sd[p + "encoder.convf1.weight"].float().reshape(128, 98).t().contiguous())
        self.add(sd[p + "encoder.convf1.bias"])
        late_scales = []
        if h8:      # (round 6, later: convf2 joins the f16c8 convolutions; its scale byte is entry [9] of the table's scale vector)
            wf2 = raw("encoder.convf2")
            sw, byte = h8_weight_scale(wf2)
            late_scales.append(byte)
            self.tensors.append(h8_conv_pack(wf2, sw))
            self.add(sd[p + "encoder.convf2.bias"].float())
        else:
            add_conv("encoder.convf2")
        add_big("encoder.conv")
        dyn = list(range(0, 128)) + list(range(256, 384))     # [h | motion + flow]: two pair sources of 128 channels
        for sfx in ("1", "2"):
            self.tensors.append(big([raw("gru.convz" + sfx, channels=dyn), raw("gru.convr" + sfx, channels=dyn)], sources=[128, 128]))
            self.add(torch.cat([sd[p + "gru.convz" + sfx + ".bias"], sd[p + "gru.convr" + sfx + ".bias"]], 0))
            self.tensors.append(big([raw("gru.convq" + sfx, channels=dyn)], sources=[128, 128]))
            self.add(sd[p + "gru.convq" + sfx + ".bias"])
        add_big("flow_head.conv1")
        w2 = sd[p + "flow_head.conv2.weight"].float().permute(2, 3, 0, 1).reshape(18, 256)
        w2 = torch.nn.functional.pad(w2, (0, 0, 0, 14)).reshape(32, 1, 1, 256)
        if h8:      # (round 6, later) fp32, in the order the flow-head epilogue's lanes read it (csrc/gemm_h8.hip EPI_FTAIL)
            self.add(flow_tail_pack(w2.reshape(32, 256)))
        else:
            self.tensors.append(_bf16_exact(conv_k_order(split3(w2))))
        self.add(sd[p + "flow_head.conv2.bias"])
        add_big("mask.0")
        add_conv("mask.2", scale=0.25)
        inp = list(range(128, 256))                           # the loop-invariant third: start maps, once per call
        for sfx in ("1", "2"):
            self.tensors.append(torch.cat([conv("gru.convz" + sfx, channels=inp), conv("gru.convr" + sfx, channels=inp)], 0).contiguous())
            self.tensors.append(conv("gru.convq" + sfx, channels=inp))
        if h8:      # [30]: E8M0 bytes of 2^-11 / sw of convc1, convc2, conv, zr1, q1, zr2, q2, flow_head.conv1, mask.0, convf2 (include/vtgb.h)
            assert len(scales) == 9
            self.tensors.append(torch.tensor(scales + late_scales, dtype=torch.int32, device=self.tensors[0].device))
        self.finish()


def raft_update(w: RaftWeights, net: Optional[Tensor], inp: Optional[Tensor], pyramid: Sequence[Tensor], iters: int = 20,
                cnet_nhwc: Optional[Tensor] = None, hw: Optional[Tuple[int, int]] = None, flow_init: Optional[Tensor] = None) -> Tensor:
    """net/inp [n, 128, H8, W8] fp32 (tanh / relu applied) -- or ``cnet_nhwc`` [n, H8*W8, 256], the context encoder's
    pixel-major output, with ``hw=(H8, W8)`` (tanh / relu are then applied inside); pyramid: 4 levels
    [n*H8*W8, 1, h, w] fp32 or fp16 -> flow_up [n, 2, 8H8, 8W8].  ``flow_init`` [n, 2, H8, W8] as in xraft.py:131-132."""
    if cnet_nhwc is not None:
        _need_cuda(cnet_nhwc, *pyramid)
        cnet_nhwc = cnet_nhwc.contiguous().float()
        n, (H8, W8) = cnet_nhwc.shape[0], hw
    else:
        _need_cuda(net, inp, *pyramid)
        net, inp = net.contiguous().float(), inp.contiguous().float()
        n, _, H8, W8 = net.shape
    if len(pyramid) != 4:
        raise ValueError("raft_update: the correlation pyramid has 4 levels")
    half = all(t.dtype == torch.float16 for t in pyramid)
    lv = [t.contiguous() if half else t.contiguous().float() for t in pyramid]
    dev = lv[0].device
    if flow_init is not None:
        flow_init = flow_init.contiguous().float()
    out = torch.empty(n, 2, 8 * H8, 8 * W8, dtype=torch.float32, device=dev)
    a = L.RaftUpdateArgs(w.code, n, H8, W8, iters, None if net is None else net.data_ptr(), None if inp is None else inp.data_ptr(),
                         (C.c_void_p * 4)(*[t.data_ptr() for t in lv]), C.cast(w.array, C.POINTER(C.c_void_p)), out.data_ptr(), None, 0,
                         1 if half else 0, None if cnet_nhwc is None else cnet_nhwc.data_ptr(), _ptr(flow_init))
    need = L.lib().vtgb_raft_update_workspace_bytes(C.byref(a))
    _log_workspace("raft_update", need, f"{n} frame pairs of {H8} x {W8} coarse pixels, dtype code {w.code}; lower flow_clips_per_call to shrink it")
    ws = _ws.get(need, dev)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    L.check(L.lib().vtgb_raft_update(C.byref(a), _stream()))
    return out


def raft_corr(fmap: Tensor, n_pairs: int, H8: int, W8: int, pairs_per_clip: int, frames_per_clip: int, first_off: int, second_off: int,
              code: int = BF16) -> List[Tensor]:
    """CorrBlock.__init__ (corr.py:12-27, :52-60): fmap [n_images, H8*W8, 256] fp32 (raft_encoder layout) -> the 4-level pyramid,
    level l [n_pairs*H8*W8, 1, H8 >> l, W8 >> l] in fp16 (bf16 mode) or fp32 (exactness mode).  Pair n correlates images
    (n // pairs_per_clip) * frames_per_clip + n % pairs_per_clip + first_off / + second_off."""
    _need_cuda(fmap)
    fmap = fmap.contiguous().float()
    n_images = fmap.numel() // (H8 * W8 * 256)
    odt = torch.float16 if code == BF16 else torch.float32      # (bf16x3: split-bf16 products, fp32 levels)
    lv, h, w = [], H8, W8
    for _ in range(4):
        lv.append(torch.empty(n_pairs * H8 * W8, 1, h, w, dtype=odt, device=fmap.device))
        h, w = h // 2, w // 2
    done = 0
    while done < n_pairs:   # the kernel's grid takes at most 65535 pairs; chunks must start on a clip boundary
        per = n_pairs - done
        if per > 65535:
            per = max(65535 // pairs_per_clip, 1) * pairs_per_clip
            if per > 65535:
                raise NotImplementedError("raft_corr: more than 65535 pairs per clip")
        img0 = (done // pairs_per_clip) * frames_per_clip
        fm = fmap.view(n_images, -1)[img0:]
        lvs = [t[done * H8 * W8:] for t in lv]
        a = L.RaftCorrArgs(code, per, H8, W8, 256, pairs_per_clip, frames_per_clip, first_off, second_off, n_images - img0, 1.0 / 16.0,
                           fm.data_ptr(), (C.c_void_p * 4)(*[t.data_ptr() for t in lvs]), None, 0)
        need = L.lib().vtgb_raft_corr_workspace_bytes(C.byref(a))
        if need == 0:
            L.check(L.lib().vtgb_raft_corr(C.byref(a), _stream()))   # raises with the library's message
        ws = _ws.get(need, fmap.device)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
        L.check(L.lib().vtgb_raft_corr(C.byref(a), _stream()))
        done += per
    return lv


def raft_stem_pack(w: Tensor, code: int) -> Tensor:
    """The stem's weight [64, 3, 7, 7] fp32 (BatchNorm already folded for cnet) -> entry [0] of vtgb_raft_encoder's table as fp32 values [64, K]: the stem
    as a 4x1 convolution over the space-to-depth image (raft_enc.hip): [co][tY][dX, py, px, c | pad to 64], ky = 2 tY + py - 1, kx = 2 dX + px - 1.  fp32
    mode: the kernel packs 2*(x/255)-1 itself, weights as they are.  bf16 mode: the kernel packs x - 127.5 as a bf16 pair (hi | lo channel chunks), so
    w' = w * 2/255 in BOTH chunks.  bf16x3 / f16c8: w' as the blocks [Wh | Wh | Wl]."""
    w = w.float()
    if code != F32:
        w = w * (2.0 / 255.0)
    wp = torch.zeros(64, 4, 4, 2, 2, 3, dtype=torch.float32, device=w.device)
    for tY in range(4):
        for py in range(2):
            ky = 2 * tY + py - 1
            if ky < 0:
                continue
            for dX in range(4):
                for px in range(2):
                    kx = 2 * dX + px - 1
                    if kx >= 0:
                        wp[:, tY, dX, py, px, :] = w[:, :, ky, kx]
    wp = torch.nn.functional.pad(wp.reshape(64, 4, 48), (0, 16))                    # [co, tY, 64]
    if code == BF16:
        wp = torch.stack([wp, wp], 1)                                               # K order: 64-channel chunk major, tap minor
    if code in (BF16X3, F16C8):                                                     # [co, tY, 1, 64] -> blocks [Wh | Wh | Wl], K order
        wp = conv_k_order(split3(wp.reshape(64, 4, 1, 64)))
    return wp.reshape(64, -1).contiguous()


def raft_stem(images: Tensor, w: Tensor, bias: Tensor, variant: int = 1, out_kind: int = L.CONV_OUT_F32, out: Optional[Tensor] = None,
              workspace: Optional[Tensor] = None):
    """The encoders' stem at bf16x3 / f16c8 alone (include/vtgb.h vtgb_raft_stem): images [n, 3, H, W] fp32, w [64, 3, 7, 7] fp32 (packed here by
    raft_stem_pack, as the encoder table packs it), bias [64].  variant 1: the fused kernel, 0: pack + implicit GEMM, 2 (fp32 rows only): the fused kernel + the moments added in variant 0's order, what
    the encoder launches for fnet.  out_kind CONV_OUT_F32 -> (fp32 rows
    [n * H/2 * W/2, 64], moments [n, 64, 2]); CONV_OUT_PAIR_BF16 / CONV_OUT_PAIR_F16C8 -> relu(.) as int16 pair rows [., 128].  ``out``: write the rows into
    the head of this contiguous tensor instead of a fresh one; ``workspace``: a uint8 tensor to use as the scratch (at least the size the library asks for)."""
    _need_cuda(images)
    dev = images.device
    images = images.contiguous().float()
    n, _, H, W = images.shape
    M2 = n * (H // 2) * (W // 2)
    pair = out_kind != L.CONV_OUT_F32
    packed = _bf16_exact(raft_stem_pack(w.to(dev), BF16X3))
    bias_t = bias.to(dev).contiguous().float()
    if out is None:
        out = torch.empty(M2, 128, dtype=torch.int16, device=dev) if pair else torch.empty(M2, 64, dtype=torch.float32, device=dev)
    assert out.is_contiguous() and out.numel() >= M2 * (128 if pair else 64) and out.dtype == (torch.int16 if pair else torch.float32)
    moments = None if pair else torch.empty(n, 64, 2, dtype=torch.float32, device=dev)
    a = L.RaftStemArgs(n, H, W, variant, out_kind, images.data_ptr(), packed.data_ptr(), bias_t.data_ptr(), out.data_ptr(), _ptr(moments), None, 0)
    need = L.lib().vtgb_raft_stem_workspace_bytes(C.byref(a))
    if need == 0:
        L.check(L.lib().vtgb_raft_stem(C.byref(a), _stream()))   # raises with the library's message
    ws = workspace if workspace is not None else _ws.get(need, dev)
    assert ws.numel() >= need
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    L.check(L.lib().vtgb_raft_stem(C.byref(a), _stream()))
    torch.cuda.current_stream().synchronize()      # (packed / bias_t are temporaries of this call)
    return out if pair else (out, moments)


def raft_layer1_h8(x: Tensor, w: Tensor, bias: Tensor, n: int, H: int, W: int, variant: int = 1, out_kind: int = L.CONV_OUT_F32, resid: Optional[Tensor] = None,
                   moments: bool = False, out: Optional[Tensor] = None, workspace: Optional[Tensor] = None):
    """One layer1 convolution of the encoders at f16c8 alone (include/vtgb.h vtgb_raft_layer1_h8): x = f16c8 pair rows [n * H * W, 128] int16 (pair_pack),
    w [64, 3, 3, 64] fp32 (co, kh, kw, ci; packed here by h8_conv_pack with h8_weight_scale's scale, as the encoder table packs it), bias [64].
    variant 0: the implicit GEMM, 1: the row-resident kernel, 2 (fp32 rows + moments): the row-resident kernel + the moments in variant 0's order.
    out_kind CONV_OUT_F32 -> fp32 rows [M, 64] (with ``moments``: (rows, moments [n, 64, 2])); CONV_OUT_PAIR_F16C8 -> relu(.) or, with ``resid`` (f16c8 pair
    rows), relu(resid + relu(.)) as int16 pair rows [M, 128]; CONV_OUT_PAIR_BF16: that tail as a bf16 pair.  ``out``: write the rows into the head of this
    contiguous tensor; ``workspace``: a uint8 tensor to use as the scratch."""
    _need_cuda(x, w)
    dev = x.device
    M = n * H * W
    assert x.is_contiguous() and x.dtype == torch.int16 and tuple(x.shape) == (M, 128) and tuple(w.shape) == (64, 3, 3, 64)
    sw, byte = h8_weight_scale(w)
    packed = h8_conv_pack(w.to(dev), sw)
    scale = torch.tensor([byte], dtype=torch.int32, device=dev)
    bias_t = bias.to(dev).contiguous().float()
    pair = out_kind != L.CONV_OUT_F32
    if out is None:
        out = torch.empty(M, 128, dtype=torch.int16, device=dev) if pair else torch.empty(M, 64, dtype=torch.float32, device=dev)
    assert out.is_contiguous() and out.numel() >= M * (128 if pair else 64) and out.dtype == (torch.int16 if pair else torch.float32)
    mom = torch.empty(n, 64, 2, dtype=torch.float32, device=dev) if moments else None
    a = L.RaftLayer1H8Args(n, H, W, variant, out_kind, x.data_ptr(), packed.data_ptr(), bias_t.data_ptr(), scale.data_ptr(), _ptr(resid), out.data_ptr(), _ptr(mom),
                           None, 0)
    need = L.lib().vtgb_raft_layer1_h8_workspace_bytes(C.byref(a))
    if need == 0:
        L.check(L.lib().vtgb_raft_layer1_h8(C.byref(a), _stream()))   # raises with the library's message
    ws = workspace if workspace is not None else _ws.get(need, dev)
    assert ws.numel() >= need
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    L.check(L.lib().vtgb_raft_layer1_h8(C.byref(a), _stream()))
    torch.cuda.current_stream().synchronize()      # (packed / scale / bias_t are temporaries of this call)
    return (out, mom) if moments else out


class RaftEncoderWeights(_WeightTable):
    """of_extractor.{fnet,cnet}.* -> the packed table of vtgb_raft_encoder.  batch_norm=True folds the eval-mode
    BatchNorm2d that follows each convolution (extractor.py:20-24,124) into the convolution's weight and bias."""

    def __init__(self, sd: Dict[str, Tensor], prefix: str, batch_norm: bool, code: int = BF16):
        super().__init__(code)
        self.batch_norm = batch_norm
        p = prefix

        def folded(conv, bn):
            w, b = sd[p + conv + ".weight"].float(), sd[p + conv + ".bias"].float()
            if batch_norm:
                g = sd[p + bn + ".weight"].float() / torch.sqrt(sd[p + bn + ".running_var"].float() + 1e-5)
                w = w * g.view(-1, 1, 1, 1)
                b = (b - sd[p + bn + ".running_mean"].float()) * g + sd[p + bn + ".bias"].float()
            return w, b

        x3 = code in (BF16X3, F16C8)
        h8_scales = [0] * 12      # VTGB_F16C8: the stride-1 3x3 convolutions on f16c8 operands (csrc/raft_enc.hip), entry [40] = their scale bytes

        def packed(w, cin_pad, cout_pad=None, h8=None):
            co, ci, kh, kw = w.shape
            w = w.permute(0, 2, 3, 1)
            if cin_pad != ci:
                w = torch.nn.functional.pad(w, (0, cin_pad - ci))
            if h8 is not None:      # (slot of the scale byte: 2 * block + conv)
                if batch_norm and cout_pad and cout_pad != co:
                    w = torch.nn.functional.pad(w, (0, 0, 0, 0, 0, 0, 0, cout_pad - co))
                sw, byte = h8_weight_scale(w)
                h8_scales[h8] = byte
                return h8_conv_pack(w, sw)
            w = conv_k_order(split3(w) if x3 else w)
            if batch_norm and cout_pad and cout_pad != co:        # cnet stores activations straight from the GEMM: padded channels = 0
                w = torch.nn.functional.pad(w, (0, 0, 0, cout_pad - co))
            return w

        def pbias(b, cout_pad):
            return torch.nn.functional.pad(b, (0, cout_pad - b.numel())) if batch_norm and cout_pad != b.numel() else b

        # stem as a 4x1 convolution over the space-to-depth image (raft_enc.hip): [co][tY][dX, py, px, c | pad to 64],
        # ky = 2 tY + py - 1, kx = 2 dX + px - 1.  fp32 mode: the kernel packs 2*(x/255)-1 itself, weights as they are.
        # bf16 mode: the kernel packs x - 127.5 as a bf16 pair (hi | lo channel chunks), so w' = w * 2/255 in BOTH chunks, b' = b
        w, b = folded("conv1", "norm1")
        self.add(raft_stem_pack(w, code), True); self.add(b)
        cin_pad = 64
        for l, (li, c, cpad) in enumerate((("layer1", 64, 64), ("layer2", 96, 128), ("layer3", 128, 128))):
            for bi in range(2):
                bp = f"{li}.{bi}."
                blk = 2 * l + bi
                w1, b1 = folded(bp + "conv1", bp + "norm1")
                w2, b2 = folded(bp + "conv2", bp + "norm2")
                # f16c8: every stride-1 3x3 (raw 16-bit patterns: appended as they are); the stride-2 conv1 of layer2.0 / layer3.0 stays bf16x3
                if code == F16C8 and (l == 0 or bi == 1):
                    self.tensors.append(packed(w1, cin_pad, cpad, 2 * blk)); self.add(pbias(b1, cpad))
                else:
                    self.add(packed(w1, cin_pad, cpad), True); self.add(pbias(b1, cpad))
                if code == F16C8:
                    self.tensors.append(packed(w2, cpad, cpad, 2 * blk + 1)); self.add(pbias(b2, cpad))
                else:
                    self.add(packed(w2, cpad, cpad), True); self.add(pbias(b2, cpad))
                if (p + bp + "downsample.0.weight") in sd:
                    wd, bd = folded(bp + "downsample.0", bp + "norm3")
                    self.add(packed(wd, cin_pad, cpad), True); self.add(pbias(bd, cpad))
                else:
                    self.add(None); self.add(None)
                cin_pad = cpad
        wh = sd[p + "conv2.weight"].float().reshape(256, 128)
        self.add(conv_k_order(split3(wh.reshape(256, 1, 1, 128))) if x3 else wh.contiguous(), True)
        self.add(sd[p + "conv2.bias"])
        if code == F16C8:
            assert len(self.tensors) == 40
            self.tensors.append(torch.tensor(h8_scales, dtype=torch.int32, device=self.tensors[0].device))
        self.finish()


def raft_encoder(w: RaftEncoderWeights, images: Tensor, max_images: int = 384) -> Tensor:
    """images [n, 3, H, W] fp32 (RAFT's 0..255 convention) -> NHWC features [n, H/8 * W/8, 256] fp32."""
    _need_cuda(images)
    images = images.contiguous().float()
    n, _, H, W = images.shape
    out = torch.empty(n, (H // 8) * (W // 8), 256, dtype=torch.float32, device=images.device)
    # max_images frames per launch sequence.  Workspace per frame at 224 x 224: 7.2 MB at bf16, 14.4 MB at fp32 / bf16x3 / f16c8 (4 bytes per channel of
    # every activation: pairs) = 5.5 GB for 384 frames.  Larger chunks are faster (per frame, f16c8 fnet: 39.2 us at 96, 36.8 at 192, 35.3 at 384, 34.7 at
    # 768 frames -- the small late stages fill the 256 CUs better; a chunk that fits the 256 MB Infinity Cache is NOT: tools/exp/enc_chunk.py), so the
    # pair modes no longer halve the chunk (round 5 did, for memory; the fp32 exactness mode still does).
    if w.code == F32:
        max_images = max(max_images // 2, 1)
    for i0 in range(0, n, max_images):
        chunk = images[i0:i0 + max_images]
        a = L.RaftEncoderArgs(w.code, chunk.shape[0], H, W, 1 if w.batch_norm else 0, chunk.data_ptr(), C.cast(w.array, C.POINTER(C.c_void_p)),
                              out[i0:i0 + max_images].data_ptr(), None, 0)
        need = L.lib().vtgb_raft_encoder_workspace_bytes(C.byref(a))
        _log_workspace("raft_encoder", need, f"{chunk.shape[0]} frames of {H} x {W} per chunk, dtype code {w.code}; max_images sets the chunk")
        ws = _ws.get(need, images.device)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
        L.check(L.lib().vtgb_raft_encoder(C.byref(a), _stream()))
    return out
