"""CPU-only checks of tests/conv_ref.py, the fp64 reference tests/test_gpu_conv_launch.py holds the convolution launches to: it is torch's own fp64
convolution for odd kernels, the 4 x 1 tap rule is the asymmetric padding of the stem table (include/vtgb.h), and the exact-pair construction of the
routing tests decomposes as claimed."""
import os

import pytest
import torch
import torch.nn.functional as F

import conv_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kh,kw,stride,H,W", [(3, 3, 1, 9, 13), (3, 3, 2, 18, 26), (1, 1, 2, 18, 26), (1, 1, 1, 5, 7), (1, 5, 1, 9, 13), (5, 1, 1, 9, 13), (7, 7, 2, 16, 12)])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_reference_is_torch_conv2d_in_fp64(kh, kw, stride, H, W, act):
    g = torch.Generator().manual_seed(kh * 10 + kw + stride)
    x, w, b = torch.randn(3, 6, H, W, generator=g).double(), torch.randn(5, 6, kh, kw, generator=g).double(), torch.randn(5, generator=g).double()
    want = F.conv2d(x, w, b, stride=stride, padding=(kh // 2, kw // 2))
    want = want.relu() if act == 1 else torch.sigmoid(want) if act == 2 else want
    got = R.conv_ref(x, w, b, stride=stride, act=act)
    assert got.shape == want.shape == (3, 5, H // stride, W // stride)
    assert torch.allclose(got, want, rtol=0, atol=1e-12)
    bound = R.conv_bound(x, w, b, stride=stride)
    assert torch.allclose(bound, F.conv2d(x.abs(), w.abs(), b.abs(), stride=stride, padding=(kh // 2, kw // 2)), rtol=0, atol=1e-12)
    assert (got.abs() <= bound + 1e-12).all() or act == 2


def test_tails_and_scale():
    g = torch.Generator().manual_seed(3)
    x, w, b = torch.randn(2, 4, 6, 5, generator=g), torch.randn(8, 4, 3, 3, generator=g), torch.randn(8, generator=g)
    skip, tw = torch.randn(2, 8, 6, 5, generator=g), torch.randn(3, 8, generator=g)
    base = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    assert torch.allclose(R.conv_ref(x, w, b, act=1, resid=skip, post_relu=True), (base.relu() + skip.double()).relu(), atol=1e-12)
    assert torch.allclose(R.conv_ref(x, w, b, act=1, resid=skip), base.relu() + skip.double(), atol=1e-12)
    assert torch.allclose(R.conv_ref(x, w, b, act=1, tail_w=tw), torch.einsum("nchw,oc->nohw", base.relu(), tw.double()), atol=1e-12)
    assert torch.allclose(R.conv_ref(x, w, b, out_scale=0.25), 0.25 * base, atol=1e-12)


def test_four_by_one_taps_are_the_stem_tables_asymmetric_padding():
    """include/vtgb.h: the stem is a 4 x 1 convolution over the 2 x 2 space-to-depth image with ky = 2 tY + py - 1 of a 7 x 7 / stride 2 / pad 3
    convolution, i.e. input row 2 oy + ky - 3 = 2 (oy + tY - 2) + py: packed rows oy - 2 .. oy + 1 -- two rows of zeros above, one below."""
    h = open(os.path.join(REPO, "include", "vtgb.h")).read()
    assert "ky = 2 tY + py - 1" in h and "4x1 convolution" in h
    g = torch.Generator().manual_seed(4)
    x, w, b = torch.randn(2, 6, 10, 7, generator=g).double(), torch.randn(5, 6, 4, 1, generator=g).double(), torch.randn(5, generator=g).double()
    want = F.conv2d(F.pad(x, (0, 0, 2, 1)), w, b)
    got = R.conv_ref(x, w, b)
    assert got.shape == want.shape == (2, 5, 10, 7) and torch.allclose(got, want, rtol=0, atol=1e-12)
    # and on a real 7 x 7 / 2 / 3 convolution of one channel, written as that table: rows only (kx folded into the channel axis is the same argument)
    img, k7 = torch.randn(1, 1, 16, 1, generator=g).double(), torch.randn(1, 1, 7, 1, generator=g).double()
    want7 = F.conv2d(img, k7, stride=(2, 1), padding=(3, 0))                               # [1, 1, 8, 1]
    packed = img.view(1, 1, 8, 2, 1).permute(0, 1, 3, 2, 4).reshape(1, 2, 8, 1)            # channel py of packed row Y = image row 2 Y + py
    w4 = torch.zeros(1, 2, 4, 1, dtype=torch.float64)
    for tY in range(4):
        for py in range(2):
            if 2 * tY + py - 1 >= 0:
                w4[0, py, tY, 0] = k7[0, 0, 2 * tY + py - 1, 0]
    assert torch.allclose(R.conv_ref(packed, w4), want7, rtol=0, atol=1e-12)


def test_rows_and_pair_helpers_round_trip():
    from videotgb_amd import ops
    g = torch.Generator().manual_seed(5)
    x = R.inputs(g, 2, 8, 3, 5)
    r = R.rows(x)
    assert r.shape == (30, 8) and torch.equal(r[1 * 15 + 2 * 5 + 4], x[1, :, 2, 4]) and torch.equal(R.unrows(r, 2, 3, 5), x.double())
    p = R.pair_rows(r)
    hi, lo = ops._bf16_parts(r)
    assert p.shape == (30, 16) and torch.equal(p.view(torch.bfloat16).float(), torch.cat([hi, lo], 1))
    back = ops.pair_unpack(p, 8, ops.BF16X3)
    assert ((back - r).abs() <= 2.0 ** -17 * r.abs()).all() and (x > 0).float().mean() > 0.4


@pytest.mark.parametrize("lo", [True, False])
def test_exact_pairs_decompose_as_claimed(lo):
    """v = a + b 2^-9: ops._bf16_parts (what split3 packs the weights with, and what vtgb_pair_pack does to an activation) returns hi == a and
    lo == b 2^-9 for every generated value, both sets are used in full, and the predicted result sum a c + 2^-9 sum (a d + b c) -- the fp64 convolution
    minus 2^-18 sum b d -- is a multiple of 2^-9 below 2^15, hence representable in fp32 like every partial sum of it, in any order."""
    from videotgb_amd import ops
    g = torch.Generator().manual_seed(6)
    a, b = R.exact_parts(g, (200000,), lo)
    assert set(a.tolist()) == {-2.0, -1.0, 1.0, 2.0} and set(b.tolist()) == ({float(v) for v in range(-3, 4)} if lo else {0.0})
    v = R.exact_value(a, b)
    assert torch.equal(v.double(), a.double() + b.double() * 2.0 ** -9)
    hi, l = ops._bf16_parts(v)
    assert torch.equal(hi, a) and torch.equal(l, b * 2.0 ** -9)
    assert torch.equal(R.pair_rows(v.view(-1, 8)).view(torch.bfloat16).float(), torch.cat([a.view(-1, 8), b.view(-1, 8) * 2.0 ** -9], 1))
    # the largest contraction of the routing tests: 3 x 3 over 256 channels (K = 2304 <= 3456), and a stride-2 one
    for (ci, kh, kw, stride) in ((256, 3, 3, 1), (64, 3, 3, 2), (128, 4, 1, 1)):
        xa, xb = R.exact_parts(g, (1, ci, 8, 6), lo)
        wa, wb = R.exact_parts(g, (16, ci, kh, kw), lo)
        pred = R.exact_conv(xa, xb, wa, wb, stride)
        full = R.conv_ref(R.exact_value(xa, xb), R.exact_value(wa, wb), stride=stride)
        assert torch.equal(pred, full - 2.0 ** -18 * R.conv_ref(xb, wb, stride=stride))          # (fp64 holds all of it exactly)
        assert torch.equal(pred.float().double(), pred) and torch.equal(pred * 512, (pred * 512).round()) and pred.abs().max() < 2.0 ** 15
        mag = R.conv_ref(xa.abs(), wa.abs(), stride=stride) + 2.0 ** -9 * (R.conv_ref(xa.abs(), wb.abs(), stride=stride) + R.conv_ref(xb.abs(), wa.abs(), stride=stride))
        assert mag.max() < 2.0 ** 15                 # every partial sum, in any order and sign pattern, stays below 2^15 = 2^24 units of 2^-9
        if lo:
            assert (pred != full).any()              # the dropped term is visible: the test distinguishes three products from four
    assert 3456 * (4 + 2.0 ** -9 * 12) < 2.0 ** 15
