"""TEST INFRASTRUCTURE (not collected by pytest, not product): the fused f16c8 "correlation lookup + convc1" launch (include/vtgb.h
vtgb_raft_lookup_convc1; csrc/raft.hip raft_lookup_convc1_h8_kernel) stated in fp64 on the CPU, and the inputs tests/test_gpu_lookup_split.py and
tests/test_lookup_split_abi.py share.

  taps    : per pixel and pyramid level l the 9 x 9 bilinear samples around (pixel + flow) / 2^l, zeros outside the level; tap (i along x, j along y) of
            level l is column l * 81 + i * 9 + j (corr.py:29-50)
  operands: csrc/pair_h8.h -- x = clamp(tap, +-57344): xh = fp16(x), xl' = e5m2((x - xh) 2^11), xh8 = e5m2(x); Wh = fp16(w), Wh8 = e4m3(w sw),
            Wl' = e4m3((w - Wh) sw 2^11)
  c1      : relu(xh . Wh + (xl' . Wh8 + xh8 . Wl') 2^-11 / sw + bias), products and sums in fp64
"""
import torch

from emul_f16c8 import e4m3, e5m2, f16

SHAPES = [(2, 9, 13), (5, 16, 16), (3, 28, 28)]      # (pairs, H8, W8)
FLOWS = ["zero", "uniform", "integer", "outside", "mix"]


def make_inputs(n, H8, W8, seed=0, extremes=False):
    """Pyramid (4 fp32 levels [M, H8 >> l, W8 >> l]), convc1 weight [256, 324], bias [256].  The levels are a common offset plus unit noise and every
    channel's weights sum to zero: the outputs are small differences of large products, which is where the two correction products show (the plain
    fp16 product is then far from the full one -- fp8_half_is_visible).  extremes: values beyond +-57344 (they saturate) and below 2^-14."""
    g = torch.Generator().manual_seed(seed)
    M = n * H8 * W8
    pyr = []
    for l in range(4):
        lv = 6.0 + torch.randn(M, H8 >> l, W8 >> l, generator=g)
        if extremes:
            flat = lv.view(-1)
            idx = torch.randperm(flat.numel(), generator=g)[:max(8, flat.numel() // 50)]
            vals = torch.tensor([1e5, -7e4, 6e4, -57344.0, 3e-5, -2e-6, 6.0e-5, 1e-7])
            flat[idx] = vals[torch.arange(idx.numel()) % 8]
        pyr.append(lv.contiguous())
    w = torch.randn(256, 324, generator=g) * 0.05
    w = w - w.mean(1, keepdim=True)
    b = torch.randn(256, generator=g) * 0.1
    return pyr, w, b


def make_flow(kind, n, H8, W8, seed=0):
    """[M, 2] fp32.  Every value is a multiple of 2^-10 (2^-6 where large): pixel + flow is then exact in fp32, as the kernel forms it."""
    g = torch.Generator().manual_seed(1000 + seed)
    M = n * H8 * W8
    uni = torch.round((torch.rand(M, 2, generator=g) * 6 - 3) * 1024) / 1024
    integer = torch.randint(-3, 4, (M, 2), generator=g).float()
    outside = torch.where(torch.rand(M, 2, generator=g) < 0.5, -1e4, 1e4) + torch.round(torch.rand(M, 2, generator=g) * 64) / 64
    if kind == "zero":
        return torch.zeros(M, 2)
    if kind == "uniform":
        return uni
    if kind == "integer":
        return integer
    if kind == "outside":
        return outside
    assert kind == "mix"
    pick = torch.randint(0, 4, (M, 1), generator=g)
    return torch.where(pick == 0, torch.zeros(M, 2), torch.where(pick == 1, uni, torch.where(pick == 2, integer, outside)))


def taps_fp64(pyr, flow, n, H8, W8):
    """[M, 324] fp64."""
    M = n * H8 * W8
    p = torch.arange(M) % (H8 * W8)
    cx = ((p % W8).float() + flow[:, 0].float()).double()      # (exact: make_flow)
    cy = ((p // W8).float() + flow[:, 1].float()).double()
    rows = torch.arange(M).view(M, 1, 1)
    d = torch.arange(10)
    out = []
    for l in range(4):
        hl, wl = H8 >> l, W8 >> l
        xs, ys = cx / (1 << l), cy / (1 << l)
        x0f, y0f = xs.floor(), ys.floor()
        qx, qy = (xs - x0f).view(M, 1, 1), (ys - y0f).view(M, 1, 1)
        ix = (x0f.long() - 4).view(M, 1) + d      # [M, 10]
        iy = (y0f.long() - 4).view(M, 1) + d
        ok = ((ix >= 0) & (ix < wl)).view(M, 1, 10) & ((iy >= 0) & (iy < hl)).view(M, 10, 1)
        win = pyr[l].double().view(M, hl, wl)[rows, iy.clamp(0, hl - 1).view(M, 10, 1), ix.clamp(0, wl - 1).view(M, 1, 10)] * ok      # [M, y, x]
        tl, tr, bl, br = win[:, :9, :9], win[:, :9, 1:], win[:, 1:, :9], win[:, 1:, 1:]
        c0, c1 = tl + qy * (bl - tl), tr + qy * (br - tr)
        v = c0 + qx * (c1 - c0)                      # [M, j (y), i (x)]
        out.append(v.permute(0, 2, 1).reshape(M, 81))
    return torch.cat(out, 1)


def weight_scale(w):
    """sw of ops.h8_weight_scale, without importing the library."""
    import math
    m = float(w.abs().max())
    return 2.0 ** max(min(0 if m == 0.0 else math.floor(math.log2(448.0 / m)), 100), -100)


def c1_fp64(taps, w, b, corrections=True):
    """The f16c8 arithmetic in fp64 -> [M, 256]; corrections=False: the plain fp16 product (both fp8 products dropped)."""
    x = taps.clamp(-57344.0, 57344.0)
    wd = w.double()
    xh, wh = f16(x), f16(wd)
    y = xh @ wh.t()
    if corrections:
        sw = weight_scale(w)
        xl8, xh8 = e5m2((x - xh) * 2048.0), e5m2(x)
        wh8, wl8 = e4m3(wd * sw), e4m3((wd - wh) * (sw * 2048.0))
        y = y + (xl8 @ wh8.t() + xh8 @ wl8.t()) / (sw * 2048.0)
    return (y + b.double()).relu()


def encode_decode(v):
    """What the pair row of an fp64 value decodes to (xh + xl' 2^-11): the 14-bit output encoding both tiles' errors are dominated by."""
    x = v.clamp(-57344.0, 57344.0)
    xh = f16(x)
    return xh + e5m2((x - xh) * 2048.0) / 2048.0


def rel_err(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())
