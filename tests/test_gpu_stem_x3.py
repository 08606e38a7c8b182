"""-m gpu: the RAFT encoders' stem at bf16x3 / f16c8 through its unit entry (include/vtgb.h vtgb_raft_stem): the fused kernel the encoders launch
(variant 1: csrc/conv64.hip stem7x7_kernel in its split-operand form, the packed rows built in LDS) against the route it replaced and still falls back
to (variant 0: raft_stem_pack_kernel + the 4 x 1 implicit GEMM, + the pair pass for cnet).

Both routes accumulate every output element in one order -- the bias, then one in-order chain of bf16 MFMAs over K in the weight table's order -- so the
comparisons are bit comparisons (torch.equal), of the fp32 rows and of cnet's pair rows in both formats.  The fused kernel's own moments are associated
differently (per run of rows instead of per 256-row tile): each route's moments are held against float64 sums of its OWN fp32 rows with the a-priori
bound of fp32 summation.  Variant 2 -- what the encoder launches for fnet: the fused rows, and the moments re-added per tile in the GEMM epilogue's
order -- must give variant 0's moments bit for bit (images of >= 256 half-resolution pixels).
Any order of adding N fp32 terms (sequential, tree or mixed) is within gamma_(N-1) sum |x_i| of the exact sum, gamma_k = k u / (1 - k u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2); a sum of squares has one more rounding per term (the square, or none
where it is fused into the addition), so gamma_N sum x_i^2 bounds it.  N = H/2 * W/2 terms per image and channel; gamma_N is used for both.

Shapes (n, H, W): the minimum (H/2 = 4, W/2 = 16); W/2 = 52, no multiple of the 16-pixel fragment (partial fragments, stores past the row); W/2 = 112,
the widest row (the most builder threads, the largest ring); 224 x 224 with one image (cut into runs of rows) and with seven (several images per
workgroup, a last partial round of the persistent grid).  Frames: integers 0..255 (RAFT's convention: the lo half of the pair is zero) and randn (what
the eval path and the benchmark hand RAFT: |x| < 5, where x - 127.5 needs the lo half)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 32), (3, 64, 64), (5, 72, 104), (2, 40, 224), (1, 224, 224), (7, 224, 224)]
KINDS = ["int", "randn"]
U = 2.0 ** -24
PAD_ROWS = 37          # rows behind the image in the poisoned outputs


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _weights():
    g = torch.Generator().manual_seed(77)
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.08
    b = torch.randn(64, generator=g) * 0.3
    b[5] = 0.0
    return w, b


def _frames(shape, kind):
    n, H, W = shape
    g = torch.Generator().manual_seed(1000 * n + H + W + (7 if kind == "int" else 0))
    if kind == "int":
        return torch.randint(0, 256, (n, 3, H, W), generator=g).float()
    return torch.randn(n, 3, H, W, generator=g)


_CASES = {}


def _case(dev, shape, kind):
    """One shape's frames and both variants' outputs of all three kinds, computed once and left unchanged."""
    key = (shape, kind)
    if key in _CASES:
        return _CASES[key]
    from videotgb_amd import _lib as L, ops
    w, b = _weights()
    img = _frames(shape, kind).to(dev)
    res = {"img": img, "w": w, "b": b}
    for v in (0, 1):
        res["f32", v], res["mom", v] = ops.raft_stem(img, w, b, variant=v)
        res["bf16", v] = ops.raft_stem(img, w, b, variant=v, out_kind=L.CONV_OUT_PAIR_BF16)
        res["h8", v] = ops.raft_stem(img, w, b, variant=v, out_kind=L.CONV_OUT_PAIR_F16C8)
    n, H, W = shape
    if (H // 2) * (W // 2) >= 256:
        res["f32", 2], res["mom", 2] = ops.raft_stem(img, w, b, variant=2)
    _CASES[key] = res
    return res


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_fused_rows_equal_the_gemm_route_bit_for_bit(dev, shape, kind):
    c = _case(dev, shape, kind)
    n, H, W = shape
    assert c["f32", 1].shape == (n * (H // 2) * (W // 2), 64)
    assert bool(torch.isfinite(c["f32", 0]).all()) and float(c["f32", 0].abs().max()) > 0.1      # (the comparison is not one of zeros)
    d = (c["f32", 1] - c["f32", 0]).abs().max().item()
    print(f"[stem x3 {shape} {kind}] max |fused - gemm| = {d:.3e} at max |out| = {c['f32', 0].abs().max().item():.3e}")
    assert torch.equal(c["f32", 1], c["f32", 0])
    if ("f32", 2) in c:
        assert torch.equal(c["f32", 2], c["f32", 0])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [s for s in SHAPES if (s[1] // 2) * (s[2] // 2) >= 256])
def test_tile_order_moments_equal_the_gemm_route_bit_for_bit(dev, shape, kind):
    """Shapes: 1024 pixels per image (4 tiles each), 1872 and 2240 (tiles that straddle two images, a last partial tile), 12544 = 49 tiles."""
    c = _case(dev, shape, kind)
    d = (c["mom", 2] - c["mom", 0]).abs().max().item()
    d1 = (c["mom", 1] - c["mom", 0]).abs().max().item()
    print(f"[stem x3 {shape} {kind}] max |moments - gemm route's|: tile order {d:.3e}, per run of rows {d1:.3e} at max {c['mom', 0].abs().max().item():.3e}")
    assert torch.equal(c["mom", 2], c["mom", 0])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] > 1])
def test_rows_do_not_depend_on_the_position_in_the_batch(dev, shape, kind):
    from videotgb_amd import ops
    c = _case(dev, shape, kind)
    n, H, W = shape
    hw = (H // 2) * (W // 2)
    for i in range(n):
        for v in (0, 1, 2):
            alone, mom = ops.raft_stem(c["img"][i:i + 1], c["w"], c["b"], variant=v)
            assert torch.equal(alone, c["f32", v][i * hw:(i + 1) * hw]), (i, v)
            if v == 1 or hw % 256 == 0:      # (variants 0, 2 add per 256-row tile of the BATCH: an image's tiles move with its position unless hw % 256 == 0)
                assert torch.equal(mom[0], c["mom", v][i]), (i, v)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_moments_are_the_sums_of_the_stored_rows(dev, shape, kind):
    c = _case(dev, shape, kind)
    n, H, W = shape
    N = (H // 2) * (W // 2)
    gamma = N * U / (1.0 - N * U)
    for v in (0, 1, 2) if ("f32", 2) in c else (0, 1):
        x = c["f32", v].double().view(n, N, 64)
        s1, s2, sa = x.sum(1), (x * x).sum(1), x.abs().sum(1)
        e1 = ((c["mom", v][:, :, 0].double() - s1).abs() / sa).max().item()
        e2 = ((c["mom", v][:, :, 1].double() - s2).abs() / s2).max().item()
        print(f"[stem x3 moments {shape} {kind} variant {v}] sum: {e1:.3e} of sum |x|, squares: {e2:.3e} of sum x^2; bound gamma_{N} = {gamma:.3e}")
        assert e1 <= gamma and e2 <= gamma


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_two_calls_give_the_same_bits(dev, shape, kind):
    from videotgb_amd import _lib as L, ops
    c = _case(dev, shape, kind)
    for v in (1, 2) if ("f32", 2) in c else (1,):
        out, mom = ops.raft_stem(c["img"], c["w"], c["b"], variant=v)
        assert torch.equal(out, c["f32", v]) and torch.equal(mom, c["mom", v])
    assert torch.equal(ops.raft_stem(c["img"], c["w"], c["b"], variant=1, out_kind=L.CONV_OUT_PAIR_BF16), c["bf16", 1])
    assert torch.equal(ops.raft_stem(c["img"], c["w"], c["b"], variant=1, out_kind=L.CONV_OUT_PAIR_F16C8), c["h8", 1])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_pair_rows_equal_the_pair_pass_over_the_gemm_rows(dev, shape, kind):
    """cnet: relu(.) as pair rows straight from the accumulators = variant 0's fp32 rows through ReLU and vtgb_pair_pack, in both formats -- and
    variant 0's own pair rows (pack + GEMM + pair pass, the parent's route)."""
    from videotgb_amd import ops
    from videotgb_amd.ops import BF16X3, F16C8
    c = _case(dev, shape, kind)
    relu = torch.clamp_min(c["f32", 0], 0.0)
    assert float((relu > 0).float().mean()) > 0.2 and float((relu == 0).float().mean()) > 0.2      # both sides of the ReLU
    for name, fmt in (("bf16", BF16X3), ("h8", F16C8)):
        want = ops.pair_pack(relu, fmt)
        assert c[name, 1].shape == want.shape == (relu.shape[0], 128)
        assert torch.equal(c[name, 0], want), name
        assert torch.equal(c[name, 1], want), name


# (variant 2 takes images of >= 256 half-resolution pixels)
@pytest.mark.parametrize("shape,variant", [(s, v) for s in [(1, 8, 32), (5, 72, 104), (2, 40, 224), (7, 224, 224)] for v in (0, 1, 2) if v < 2 or s != (1, 8, 32)])
def test_poisoned_buffers_leave_no_trace_and_rows_past_the_image_stay(dev, shape, variant):
    from videotgb_amd import _lib as L, ops
    c = _case(dev, shape, "randn")
    n, H, W = shape
    M2 = n * (H // 2) * (W // 2)
    need = L.lib().vtgb_raft_stem_workspace_bytes(L.C.byref(L.RaftStemArgs(n, H, W, 0, L.CONV_OUT_PAIR_BF16, None, None, None, None, None, None, 0)))
    need = max(need, L.lib().vtgb_raft_stem_workspace_bytes(L.C.byref(L.RaftStemArgs(n, H, W, 0, L.CONV_OUT_F32, None, None, None, None, None, None, 0))))
    assert need > 0

    def poisoned_ws():
        return torch.full((need + 4096,), 0xFF, dtype=torch.uint8, device=dev)      # fp32 / bf16 / fp16 NaN patterns throughout

    out = torch.full((M2 + PAD_ROWS, 64), float("nan"), dtype=torch.float32, device=dev)
    rows, mom = ops.raft_stem(c["img"], c["w"], c["b"], variant=variant, out=out, workspace=poisoned_ws())
    assert rows.data_ptr() == out.data_ptr()
    assert bool(torch.isfinite(out[:M2]).all()) and bool(torch.isfinite(mom).all())
    assert torch.equal(out[:M2], c["f32", variant]) and torch.equal(mom, c["mom", variant])
    assert bool(torch.isnan(out[M2:]).all())
    if variant == 2:
        return
    for name, kind in (("bf16", L.CONV_OUT_PAIR_BF16), ("h8", L.CONV_OUT_PAIR_F16C8)):
        outp = torch.full((M2 + PAD_ROWS, 128), 0x7FFF, dtype=torch.int16, device=dev)      # NaN as bf16 and as fp16
        ops.raft_stem(c["img"], c["w"], c["b"], variant=variant, out_kind=kind, out=outp, workspace=poisoned_ws())
        assert torch.equal(outp[:M2], c[name, variant]), name
        assert bool(torch.isfinite(ops.pair_unpack(outp[:M2], 64, ops.BF16X3 if name == "bf16" else ops.F16C8)).all())
        assert bool((outp[M2:] == 0x7FFF).all()), name
