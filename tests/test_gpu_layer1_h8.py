"""-m gpu: one layer1 convolution of the RAFT encoders at f16c8 through its unit entry (include/vtgb.h vtgb_raft_layer1_h8): the row-resident kernel the
encoders launch (variant 1; variant 2 = + the moments per 256-row tile) against the implicit GEMM it replaces there (variant 0), BIT FOR BIT -- the fp32 rows
fnet normalises, cnet's relu(.) pair rows, and the ResidualBlock tail relu(x + relu(.)) as an f16c8 and as a bf16 pair -- and variant 0 against an fp64
convolution of the operands the pairs stand for, within the bound tests/test_gpu_h8.py uses for vtgb_pair_conv (2^-14 of sum |x| |w| + |b|).  Then the encoders
with the dispatch on and off: the features must not move by a bit."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (n, H, W) at the convolution's own resolution: the minimum size; a small multi-image case; W no multiple of the 16-pixel fragment; the widest row (largest
# ring); one image cut into runs of rows; several images per workgroup and a last partial round of the persistent grid
SHAPES = [(1, 4, 16), (3, 32, 32), (5, 36, 52), (2, 20, 112), (1, 112, 112), (7, 112, 112)]
PAD_ROWS = 96           # rows behind the image in every output buffer: must stay as they were
POISON16, POISON32 = 0x7E7E, float("nan")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _poisoned(M, pair, dev):
    if pair:
        return torch.full((M + PAD_ROWS, 128), POISON16, dtype=torch.int16, device=dev)
    return torch.full((M + PAD_ROWS, 64), POISON32, dtype=torch.float32, device=dev)


def _tail_untouched(buf, M, pair):
    t = buf[M:]
    return bool((t == POISON16).all()) if pair else bool(torch.isnan(t).all())


_cache = {}


def _case(dev, shape):
    """Everything the tests of one shape compare, computed once: per variant the fp32 rows (post-ReLU-like and signed inputs), the three pair epilogues, the moments."""
    if shape in _cache:
        return _cache[shape]
    from videotgb_amd import _lib as L
    from videotgb_amd import ops
    n, H, W = shape
    M = n * H * W
    g = torch.Generator().manual_seed(H * 1000 + W * 7 + n)
    x = torch.randn(n, 64, H, W, generator=g) * (torch.rand(n, 1, H, W, generator=g) * 10 + 0.1)
    x = torch.relu(x) + 0.05 * torch.randn(n, 64, H, W, generator=g).abs() * (torch.rand(n, 64, H, W, generator=g) < 0.3)      # post-ReLU-like: zeros, a wide range of magnitudes
    xs = torch.randn(n, 64, H, W, generator=g) * (torch.rand(n, 1, H, W, generator=g) * 5 + 0.1)                           # signed rows
    w = torch.randn(64, 64, 3, 3, generator=g) * 0.05
    b = torch.randn(64, generator=g)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(M, 64).contiguous()
    c = dict(n=n, H=H, W=W, M=M, x=x, xs=xs, w=w, b=b)
    c["xr"] = ops.pair_pack(rows(x).to(dev))
    c["xsr"] = ops.pair_pack(rows(xs).to(dev))
    c["wk"] = w.permute(0, 2, 3, 1).contiguous().to(dev)
    c["bd"] = b.to(dev)
    moments = H * W >= 256
    c["moments"] = moments

    def run(variant, kind, xin, resid=None, mom=False):
        pair = kind != L.CONV_OUT_F32
        buf = _poisoned(M, pair, dev)
        r = ops.raft_layer1_h8(xin, c["wk"], c["bd"], n, H, W, variant=variant, out_kind=kind, resid=resid, moments=mom, out=buf)
        assert _tail_untouched(buf, M, pair), f"variant {variant} wrote behind the image"
        return (buf[:M].clone(), r[1].clone()) if mom else buf[:M].clone()

    c["run"] = run
    for v in (0, 1):
        c["f32", v] = run(v, L.CONV_OUT_F32, c["xr"])
        c["f32s", v] = run(v, L.CONV_OUT_F32, c["xsr"])
        c["relu", v] = run(v, L.CONV_OUT_PAIR_F16C8, c["xr"])
        c["tail", v] = run(v, L.CONV_OUT_PAIR_F16C8, c["xr"], resid=c["xsr"])
        c["tailb", v] = run(v, L.CONV_OUT_PAIR_BF16, c["xr"], resid=c["xsr"])
    if moments:
        c["f32m", 0], c["mom", 0] = run(0, L.CONV_OUT_F32, c["xr"], mom=True)
        c["f32m", 2], c["mom", 2] = run(2, L.CONV_OUT_F32, c["xr"], mom=True)
    _cache[shape] = c
    return c


@pytest.mark.parametrize("shape", SHAPES)
def test_rows_and_pair_epilogues_have_the_implicit_gemms_bits(dev, shape):
    c = _case(dev, shape)
    for key in ("f32", "f32s", "relu", "tail", "tailb"):
        a, b = c[key, 0], c[key, 1]
        assert not torch.isnan(a).any() if a.dtype == torch.float32 else bool((a != POISON16).any())
        assert torch.equal(a, b), f"{key}: {int((a != b).sum())} of {a.numel()} elements differ"
    assert c["f32", 0].abs().max() > 0 and c["relu", 0].any() and c["tail", 0].any() and c["tailb", 0].any()


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[1] * s[2] >= 256])
def test_tile_order_moments_have_the_implicit_gemms_bits(dev, shape):
    c = _case(dev, shape)
    assert torch.equal(c["f32m", 2], c["f32m", 0]) and torch.equal(c["f32m", 0], c["f32", 0])
    assert torch.equal(c["mom", 2], c["mom", 0])
    rows = c["f32", 0].view(c["n"], -1, 64).double()
    want = torch.stack([rows.sum(1), (rows * rows).sum(1)], -1)
    assert torch.allclose(c["mom", 0].double(), want, rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("shape", SHAPES)
def test_implicit_gemm_vs_fp64(dev, shape):
    """Variant 0 against fp64 from the values the input pairs stand for (the bit comparison carries the bound over to the row-resident kernel)."""
    from videotgb_amd import ops
    c = _case(dev, shape)
    n, H, W, M = c["n"], c["H"], c["W"], c["M"]
    img = lambda r: r.cpu().view(n, H, W, 64).permute(0, 3, 1, 2).double()
    xd, sd = img(ops.pair_unpack(c["xr"], 64)), img(ops.pair_unpack(c["xsr"], 64))
    w, b = c["w"].double(), c["b"].double()
    conv = F.conv2d(xd, w, b, padding=1)
    bound = F.conv2d(xd.abs(), w.abs(), None, padding=1) + b.abs().view(1, -1, 1, 1)
    err = ((img(c["f32", 0]) - conv).abs() / bound).max().item()
    err_relu = ((img(ops.pair_unpack(c["relu", 0], 64)) - conv.relu()).abs() / bound).max().item()
    tail = (sd + conv.relu()).relu()
    tb = bound + sd.abs()
    err_tail = ((img(ops.pair_unpack(c["tail", 0], 64)) - tail).abs() / tb).max().item()
    err_tailb = ((img(ops.pair_unpack(c["tailb", 0], 64, ops.BF16X3)) - tail).abs() / tb).max().item()
    print(f"[layer1 h8 {shape}] max err / bound: fp32 rows {err:.3e}, relu pair {err_relu:.3e}, tail {err_tail:.3e}, tail as bf16 pair {err_tailb:.3e} (2^-14 = {2.0 ** -14:.3e})")
    assert max(err, err_relu, err_tail, err_tailb) <= 2.0 ** -14


@pytest.mark.parametrize("shape", SHAPES)
def test_repeated_calls_give_equal_bits(dev, shape):
    from videotgb_amd import _lib as L
    c = _case(dev, shape)
    for _ in range(3):
        assert torch.equal(c["run"](1, L.CONV_OUT_F32, c["xr"]), c["f32", 1])
        assert torch.equal(c["run"](1, L.CONV_OUT_PAIR_BF16, c["xr"], resid=c["xsr"]), c["tailb", 1])
    if c["moments"]:
        for _ in range(3):
            rows, mom = c["run"](2, L.CONV_OUT_F32, c["xr"], mom=True)
            assert torch.equal(rows, c["f32m", 2]) and torch.equal(mom, c["mom", 2])


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] > 1])
def test_a_batched_call_equals_single_image_calls(dev, shape):
    from videotgb_amd import _lib as L
    from videotgb_amd import ops
    c = _case(dev, shape)
    n, H, W = shape
    hw = H * W
    for i in range(n):
        xi, ri = c["xr"][i * hw:(i + 1) * hw].contiguous(), c["xsr"][i * hw:(i + 1) * hw].contiguous()
        one = ops.raft_layer1_h8(xi, c["wk"], c["bd"], 1, H, W, variant=1)
        assert torch.equal(one, c["f32", 1][i * hw:(i + 1) * hw])
        one = ops.raft_layer1_h8(xi, c["wk"], c["bd"], 1, H, W, variant=1, out_kind=L.CONV_OUT_PAIR_F16C8, resid=ri)
        assert torch.equal(one, c["tail", 1][i * hw:(i + 1) * hw])
        if c["moments"] and hw % 256 == 0:      # (the moments are added per 256-row tile of the CALL: image-aligned only when H * W is a multiple of 256)
            _, mom = ops.raft_layer1_h8(xi, c["wk"], c["bd"], 1, H, W, variant=2, moments=True)
            assert torch.equal(mom[0], c["mom", 2][i])


@pytest.mark.parametrize("net,bn", [("fnet.", False), ("cnet.", True)])
@pytest.mark.parametrize("n,H,W", [(2, 64, 64), (3, 72, 104)])
def test_encoder_features_do_not_move_with_the_dispatch(dev, tiny_sd, net, bn, n, H, W):
    """vtgb_raft_encoder at VTGB_F16C8 with layer1 on the row-resident kernel (both nets) and on the implicit GEMM: bit-equal features."""
    from videotgb_amd import _lib as L
    from videotgb_amd import ops
    sd = tiny_sd["instructblip"][1]
    rsd = {k[len("of_extractor."):]: v.to(dev) for k, v in sd.items() if k.startswith("of_extractor.")}
    w = ops.RaftEncoderWeights(rsd, net, bn, ops.raft_dtype_code("f16c8"))
    fr = torch.randint(0, 256, (n, 3, H, W), generator=torch.Generator().manual_seed(H + W)).float().to(dev)
    setter = L.lib().vtgb_debug_set_l1_h8
    setter.argtypes, setter.restype = [L.C.c_int], None
    try:
        setter(0)
        off = ops.raft_encoder(w, fr).clone()
        setter(3)
        on = ops.raft_encoder(w, fr).clone()
        setter(1)
        cnet_only = ops.raft_encoder(w, fr).clone()
    finally:
        setter(3)      # the library's default: both nets
    assert torch.isfinite(off).all() and off.abs().max() > 0
    assert torch.equal(on, off) and torch.equal(cnet_only, off)
