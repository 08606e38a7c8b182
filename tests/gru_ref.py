"""TEST INFRASTRUCTURE (not collected by pytest, not product): the two gate launches of one SepConvGRU half-step of vtgb_raft_update's refinement loop
(include/vtgb.h vtgb_raft_gru_half; csrc/raft_x3.hip x3_gru_half; the epilogues EPI_X3ZR / EPI_X3Q of csrc/gemm_h8.hip and csrc/gemm_pp.hip) stated in
fp64 on the CPU, and the inputs and bounds tests/test_gpu_gru_half.py and tests/test_gru_half_abi.py share.

  operands: the device's own roundings, decoded from the pair BYTES the device reads (pack_pair is the CPU statement of vtgb_pair_pack):
            f16c8 (csrc/pair_h8.h)  xh = fp16(x), xl' = e5m2((x - xh) 2^11), xh8 = e5m2(x); Wh = fp16(w), Wh8 = e4m3(w sw), Wl' = e4m3((w - Wh) sw 2^11)
                                    pre = xh . Wh + (xl' . Wh8 + xh8 . Wl') 2^-11 / sw + start
            bf16x3                  hi = bf16(x), lo = bf16(x - hi); Wh = bf16(w), Wl = bf16(w - Wh);   pre = hi . Wh + lo . Wh + hi . Wl + start
  launches: z | r   pre over [h | x] (256 channels in, 256 out): z = sigmoid(pre[:, :128]), rh = sigmoid(pre[:, 128:]) * h
            q       pre over [rh | x] (256 in, 128 out): h' = (1 - z) h + z tanh(pre)
            h = the value the h pair decodes to (ops.pair_unpack semantics); products, sums, sigmoid and tanh in fp64 (dtype=torch.float32: the same
            operands through torch's fp32 convolutions -- what fp32 accumulation alone costs, the unit of the bounds)
  bounds  : E = 4 e_f32 on a pre-activation (e_f32 = max |pre fp64 - pre fp32|; the 4: the matrix instruction's internal order and rounding differ from
            the CPU's blocked FMAs, and the device adds the scaled fp8 products in fp32), T = 2^-20 for the fast sigmoid / tanh (v_exp_f32 and v_rcp_f32
            are ~1 ulp, __expf's argument rounding is |v| 2^-24 relative to exp and the sigmoid's sensitivity to it is min(1/4, e^-|v|): < 2^-22 for
            the sigmoid, < 2^-21 for the tanh form; 2^-20 leaves a factor of 2), P = the pair encoding's own error.
"""
import math

import torch
import torch.nn.functional as F

from emul_f16c8 import bf16, e4m3, e5m2, f16

BF16X3, F16C8 = 2, 3      # include/vtgb.h
FMT = {"f16c8": F16C8, "bf16x3": BF16X3}
SHAPES = [(2, 9, 13), (5, 16, 16), (3, 28, 28)]      # (images, H8, W8); the first: 234 rows = one partial tile that straddles two images, 5x1 on 9 rows
DROPS = {F16C8: ("xl.Wh8", "xh8.Wl"), BF16X3: ("lo.Wh", "hi.Wl")}      # the correction products of a format (pre_act's `drop`)
T = 2.0 ** -20
SAT = 100.0


def kernel_hw(half):
    return (1, 5) if half == 0 else (5, 1)


def make_inputs(n, H8, W8, half, seed=0, extremes=False):
    """h, x [M, 128] fp32; w_zr [256, kh, kw, 256], w_q [128, kh, kw, 256] over the input channels [h | x]; start_zr [M, 256], start_q [M, 128].
    h = tanh(1.5 randn); x post-ReLU-like with a positive offset; every output channel's weights sum to zero, so the outputs are small differences of
    large products and the correction products show (tests/test_gru_half_abi.py: dropping one is >= 4 x the bounds away).
    extremes: the start maps of 300 scattered (row, channel) positions are +-100 (the gate saturates; `sat_zr`, `sat_q` = (rows, channels, signs))
    and some h values are +-0 and the smallest magnitudes a pair holds."""
    g = torch.Generator().manual_seed(1000 * seed + 10 * half + (5 if extremes else 0) + n * H8 * W8)
    M = n * H8 * W8
    kh, kw = kernel_hw(half)
    h = torch.tanh(1.5 * torch.randn(M, 128, generator=g))
    x = torch.relu(torch.randn(M, 128, generator=g) * (torch.rand(M, 1, generator=g) * 4.0 + 0.1)) + 0.05 * torch.randn(M, 128, generator=g) + 0.5
    d = {"h": h, "x": x}
    for name, co in (("zr", 256), ("q", 128)):
        w = torch.randn(co, kh, kw, 256, generator=g) * 0.05
        d["w_" + name] = (w - w.mean((1, 2, 3), keepdim=True)).contiguous()
        d["start_" + name] = torch.randn(M, co, generator=g)
    if extremes:
        for name, co in (("zr", 256), ("q", 128)):
            idx = torch.randperm(M * co, generator=g)[:300]
            rows, cols = idx // co, idx % co
            sign = torch.where(torch.arange(300) % 2 == 0, 1.0, -1.0)
            d["start_" + name][rows, cols] = SAT * sign
            d["sat_" + name] = (rows, cols, sign)
        idx = torch.randperm(M * 128, generator=g)[:64]
        tiny = torch.tensor([0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -27, -2.0 ** -27, 2.0 ** -126, -2.0 ** -133])      # fp16's / e5m2 2^-11's / bf16's smallest
        h.view(-1)[idx] = tiny[torch.arange(64) % 8]
    return d


# ---- pair rows [M, 2 C] int16 (include/vtgb.h vtgb_pair_pack with ld_pair = C)
def pack_pair(v, fmt):
    M, C_ = v.shape
    v = v.float()
    if fmt == BF16X3:
        hi = v.to(torch.bfloat16)
        lo = (v - hi.float()).to(torch.bfloat16)
        return torch.cat([hi.view(torch.int16), lo.view(torch.int16)], 1).contiguous()
    x = v.clamp(-57344.0, 57344.0)
    xh = x.to(torch.float16)
    r8 = ((x - xh.float()) * 2048.0).to(torch.float8_e5m2).view(torch.uint8).reshape(M, C_ // 4, 4)
    v8 = x.to(torch.float8_e5m2).view(torch.uint8).reshape(M, C_ // 4, 4)
    lo = torch.stack([r8, v8], 2).reshape(M, 2 * C_).contiguous().view(torch.int16)
    return torch.cat([xh.view(torch.int16), lo], 1).contiguous()


def pair_operands(rows, fmt):
    """The operands a pair row enters a contraction as, fp64 [M, C] each: bf16x3 (hi, lo); f16c8 (xh, xl', xh8)."""
    rows = rows.cpu()
    M, C_ = rows.shape[0], rows.shape[1] // 2
    if fmt == BF16X3:
        v = rows.view(torch.bfloat16).double()
        return v[:, :C_], v[:, C_:]
    xh = rows[:, :C_].contiguous().view(torch.float16).double()
    by = rows[:, C_:].contiguous().view(torch.uint8).reshape(M, C_ // 4, 2, 4)
    xl8, xh8 = (by[:, :, i].reshape(M, C_).contiguous().view(torch.float8_e5m2).double() for i in (0, 1))
    return xh, xl8, xh8


def pair_value(rows, fmt):
    """The value a pair stands for where an epilogue reads it back element-wise (ops.pair_unpack): hi + lo; xh + xl' 2^-11."""
    o = pair_operands(rows, fmt)
    return o[0] + (o[1] if fmt == BF16X3 else o[1] / 2048.0)


def encode_decode(v, fmt):
    """What the pair row of an fp64 value decodes to."""
    if fmt == BF16X3:
        hi = bf16(v)
        return hi + bf16(v - hi)
    x = v.clamp(-57344.0, 57344.0)
    xh = f16(x)
    return xh + e5m2((x - xh) * 2048.0) / 2048.0


def P(v, fmt):
    """The pair encoding's bound: f16c8 what tests/test_gpu_h8.py holds pair_pack to; bf16x3 two bf16 roundings."""
    return 2.0 ** -14 * v.abs() + 2.0 ** -25 if fmt == F16C8 else 2.0 ** -16 * v.abs() + 2.0 ** -40


def weight_scale(w):
    """sw of ops.h8_weight_scale, without importing the library."""
    m = float(w.abs().max())
    return 2.0 ** max(min(0 if m == 0.0 else math.floor(math.log2(448.0 / m)), 100), -100)


def pre_act(fmt, a_rows, x_rows, w, start, shape, half, dtype=torch.float64, drop=None):
    """The pre-activation [M, co] of one launch: the convolution of [a | x] (pair rows) with w [co, kh, kw, 256] + start.  drop: one of DROPS[fmt]."""
    n, H8, W8 = shape
    kh, kw = kernel_hw(half)
    assert drop is None or drop in DROPS[fmt]
    acts = [torch.cat([a, b], 1) for a, b in zip(pair_operands(a_rows, fmt), pair_operands(x_rows, fmt))]
    wd = w.double()

    def cv(act, wt):
        # (contiguous NCHW / OIHW: on channels-last views torch's CPU fp32 convolution takes a path that sums ~5 x less accurately, and e_f32 with it)
        y = F.conv2d(act.view(n, H8, W8, 256).permute(0, 3, 1, 2).to(dtype).contiguous(), wt.permute(0, 3, 1, 2).to(dtype).contiguous(), None, padding=(kh // 2, kw // 2))
        return y.permute(0, 2, 3, 1).reshape(n * H8 * W8, -1)

    if fmt == BF16X3:
        hi, lo = acts
        wh = bf16(wd)
        wl = bf16(wd - wh)
        y = cv(hi, wh)
        if drop != "lo.Wh":
            y = y + cv(lo, wh)
        if drop != "hi.Wl":
            y = y + cv(hi, wl)
    else:
        xh, xl8, xh8 = acts
        sw = weight_scale(w)
        wh = f16(wd)
        wh8, wl8 = e4m3(wd * sw), e4m3((wd - wh) * (sw * 2048.0))
        y = cv(xh, wh)
        c = torch.zeros_like(y)
        if drop != "xl.Wh8":
            c = c + cv(xl8, wh8)
        if drop != "xh8.Wl":
            c = c + cv(xh8, wl8)
        y = y + c * (1.0 / (sw * 2048.0))
    return y + start.to(dtype)


def e_f32(fmt, a_rows, x_rows, w, start, shape, half, pre64=None):
    """max |pre fp64 - the same rounded operands through torch's fp32 convolutions|: what fp32 accumulation alone costs on these inputs."""
    if pre64 is None:
        pre64 = pre_act(fmt, a_rows, x_rows, w, start, shape, half)
    return float((pre64 - pre_act(fmt, a_rows, x_rows, w, start, shape, half, dtype=torch.float32).double()).abs().max())


def gates_zr(pre, hval):
    """(z, r h) of the z | r launch."""
    return torch.sigmoid(pre[:, :128]), torch.sigmoid(pre[:, 128:]) * hval


def gate_q(pre, z, hval):
    return (1.0 - z) * hval + z * torch.tanh(pre)


# ---- the bounds of the issue (a), element-wise; e = e_f32 of the launch, E = 4 e
def bound_z(e):
    return e + T                                                         # E / 4 + T: the sigmoid's slope is <= 1 / 4


def bound_rh(e, hval, rh_ref, fmt):
    return hval.abs() * (e + T) + P(rh_ref, fmt)


def bound_h(e, z, hval, h_ref, fmt):
    return z * (4.0 * e + T) + P(h_ref, fmt) + 4.0 * 2.0 ** -24 * (hval.abs() + 1.0)      # tanh's slope is <= 1; four fp32 roundings of the blend


def stage0(fmt, d, shape, half, drop=None, h_rows=None, x_rows=None):
    """The z | r launch of make_inputs' dict d in fp64 (h_rows / x_rows: these pair rows instead of d's h / x): dict(pre, z, rh, hval, h_rows, x_rows)."""
    h_rows = pack_pair(d["h"], fmt) if h_rows is None else h_rows.cpu()
    x_rows = pack_pair(d["x"], fmt) if x_rows is None else x_rows.cpu()
    pre = pre_act(fmt, h_rows, x_rows, d["w_zr"], d["start_zr"], shape, half, drop=drop)
    hval = pair_value(h_rows, fmt)
    z, rh = gates_zr(pre, hval)
    return dict(pre=pre, z=z, rh=rh, hval=hval, h_rows=h_rows, x_rows=x_rows)


def stage1(fmt, d, shape, half, rh_rows, z32, hq_rows, x_rows, drop=None):
    """The q launch in fp64 from the values it reads: rh pair rows, z fp32, the h pair it updates: dict(pre, h_new, hval, z)."""
    pre = pre_act(fmt, rh_rows, x_rows, d["w_q"], d["start_q"], shape, half, drop=drop)
    hval, z = pair_value(hq_rows, fmt), z32.cpu().double()
    return dict(pre=pre, h_new=gate_q(pre, z, hval), hval=hval, z=z)
