"""CPU reference of ONE implicit-GEMM convolution launch of RAFT (include/vtgb.h vtgb_conv_launch; csrc/gemm.hip, gemm_pp.hip, conv_f32.hip) in fp64,
for tests/test_gpu_conv_launch.py (the device against it) and tests/test_conv_ref.py (this file against torch, no GPU).

The kernels' geometry: NHWC rows, output pixel (oy, ox) reads input pixel (oy * stride + ty - KH // 2, ox * stride + tx - KW // 2) for tap (ty, tx),
zeros outside the Hi x Wi input grid.  Odd kernels: the usual 'same' padding.  Even kernels (the 4 x 1 stem GEMM over the packed rows) pad KH // 2
before and KH - 1 - KH // 2 behind.  Everything here is a plain tap loop of fp64 matrix products, on whatever device the operands live."""
import torch

BF16X3, BF16, F32 = 2, 1, 0


def conv_ref(x, w, b=None, stride=1, act=0, resid=None, post_relu=False, tail_w=None, out_scale=1.0):
    """x [n, ci, Hi, Wi], w [co, ci, kh, kw], b [co] -> fp64 [n, co, Ho, Wo] with Ho = ceil(Hi / stride): out_scale * act(conv + b), then
    [relu](. + resid) (a ResidualBlock's tail, resid [n, co, Ho, Wo]), then -- tail_w [o, co] -- the 1 x 1 product with tail_w ([n, o, Ho, Wo])."""
    x, w = x.double(), w.double()
    n, ci, Hi, Wi = x.shape
    co, ci_w, kh, kw = w.shape
    assert ci == ci_w
    Ho, Wo = (Hi + stride - 1) // stride, (Wi + stride - 1) // stride
    xp = torch.nn.functional.pad(x, (kw // 2, kw - 1 - kw // 2 + stride, kh // 2, kh - 1 - kh // 2 + stride))
    out = torch.zeros(n, co, Ho, Wo, dtype=torch.float64, device=x.device)
    for ty in range(kh):
        for tx in range(kw):
            win = xp[:, :, ty:ty + stride * Ho:stride, tx:tx + stride * Wo:stride]
            out += torch.einsum("nchw,oc->nohw", win, w[:, :, ty, tx])
    if b is not None:
        out += b.double().view(1, -1, 1, 1)
    if act == 1:
        out = out.relu()
    elif act == 2:
        out = torch.sigmoid(out)
    out = out * out_scale
    if resid is not None:
        out = out + resid.double()
        if post_relu:
            out = out.relu()
    if tail_w is not None:
        out = torch.einsum("nchw,oc->nohw", out, tail_w.double())
    return out


def conv_bound(x, w, b=None, stride=1):
    """The magnitude an error is measured against: sum |x| |w| + |b| per output element."""
    return conv_ref(x.abs(), w.abs(), None if b is None else b.abs(), stride)


def rows(x):
    """[n, C, H, W] -> NHWC rows [n H W, C]."""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def unrows(r, n, H, W, C=None):
    """rows [n H W, >= C] -> [n, C, H, W] fp64."""
    C = C or r.shape[1]
    return r[:, :C].reshape(n, H, W, C).permute(0, 3, 1, 2).double()


def bf16r(x):
    """x rounded to bf16, as fp32."""
    return x.to(torch.bfloat16).float()


def pair_rows(x2d):
    """fp32 rows [M, C] -> the bf16 pair rows [hi(C) | lo(C)] as int16 [M, 2 C] (what vtgb_pair_pack(VTGB_BF16X3) writes), on the CPU."""
    hi = x2d.to(torch.bfloat16)
    lo = (x2d - hi.float()).to(torch.bfloat16)
    return torch.cat([hi, lo], 1).contiguous().view(torch.int16)


def inputs(g, n, C, H, W, spread=10.0):
    """post-ReLU-like activations (tests/test_gpu_h8.py _inputs): mostly positive, a wide range of magnitudes, a little signed noise."""
    x = torch.randn(n, C, H, W, generator=g) * (torch.rand(n, 1, H, W, generator=g) * spread + 0.1)
    return torch.relu(x) + 0.05 * torch.randn(n, C, H, W, generator=g)


# ---- the exact-pair construction: values v = a + b 2^-9, a in {+-1, +-2}, b in {-3 .. 3}, whose bf16 pair is exactly (a, b 2^-9).
# bf16 keeps 8 significant bits, so hi = bf16(v) stays at a only while |b| 2^-9 does not pass half a unit in the last place on that side of a (ties go
# to a: its mantissa is even): |a| = 1 takes b a >= 0 up to |b| = 2 and b a < 0 up to |b| = 1; |a| = 2 takes b a >= 0 up to 3 and b a < 0 up to 2.  A draw
# outside that (8 of the 28 (a, b) combinations) is folded back to b = sign(a) (|b| - 1), which is inside; every value of both sets still occurs.
EXACT_LO = 2.0 ** -9


def exact_parts(g, shape, lo=True):
    """(a, b) integer-valued fp32 tensors of `shape`; lo = False: b = 0 (the bf16 mode's operands)."""
    a = (torch.randint(0, 2, shape, generator=g) * 2 - 1) * (torch.randint(1, 3, shape, generator=g))
    b = torch.randint(-3, 4, shape, generator=g)
    same = (a * b) >= 0
    ok = torch.where(a.abs() == 1, torch.where(same, b.abs() <= 2, b.abs() <= 1), torch.where(same, b.abs() <= 3, b.abs() <= 2))
    b = torch.where(ok, b, torch.sign(a) * (b.abs() - 1))
    if not lo:
        b = torch.zeros_like(b)
    return a.float(), b.float()


def exact_value(a, b):
    return a + b * EXACT_LO          # exact in fp32: 12 significant bits


def exact_conv(xa, xb, wa, wb, stride=1):
    """What the three products hi.Wh + lo.Wh + hi.Wl give for x = (xa, xb 2^-9), w = (wa, wb 2^-9): sum a c + 2^-9 sum (a d + b c), the fp64 convolution
    minus the dropped 2^-18 sum b d.  fp64 [n, co, Ho, Wo]; a multiple of 2^-9 below 2^15 for K <= 3456 channels x taps, so exact in fp32 in any order."""
    return conv_ref(xa, wa, stride=stride) + EXACT_LO * (conv_ref(xa, wb, stride=stride) + conv_ref(xb, wa, stride=stride))
