"""-m gpu: the fused f16c8 correlation lookup + convc1 launch through its unit entry (include/vtgb.h vtgb_raft_lookup_convc1): the split-K tile that
vtgb_raft_update launches (variant 1, two workgroups per CU) against the whole-K tile it replaced (variant 0) and against the same arithmetic in fp64
(tests/lookup_ref.py).

err(variant) = max |decoded c1 - ref| / max |ref|, ref = the f16c8 arithmetic in fp64.  Only the order of the fp32 additions differs between the tiles
and both errors are dominated by the 14-bit output encoding, so err(1) <= 1.5 err(0) on the same inputs; no absolute bound.  The inputs are such that the
test sees the fp8 half: the reference with both correction products dropped is >= 4 x 1.5 err(0) away from the full one (13-22 x the output encoding's
own error on the CPU, tests/test_lookup_split_abi.py), and each tile is closer to the full reference than that.
Measured on an MI355X (err(0), err(1) per shape over the four in-range flow kinds): see DESIGN.md section 4."""
import pytest
import torch

import lookup_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


_CASES = {}


def _case(dev, shape):
    """Inputs, fp64 references and both tiles' outputs of one shape, computed once: {flow kind: (ref, ref without corrections, rows v0, rows v1)}."""
    if shape in _CASES:
        return _CASES[shape]
    from videotgb_amd import ops
    n, H8, W8 = shape
    pyr, w, b = R.make_inputs(n, H8, W8, extremes=(shape == (5, 16, 16)))
    pd = [p.to(dev) for p in pyr]
    res = {"inputs": (pyr, w, b, pd)}
    for kind in R.FLOWS:
        fl = R.make_flow(kind, n, H8, W8)
        taps = R.taps_fp64(pyr, fl, n, H8, W8)
        rows = [ops.raft_lookup_convc1(pd, fl.to(dev), w, b, H8, W8, variant=v) for v in (0, 1)]
        res[kind] = (R.c1_fp64(taps, w, b), R.c1_fp64(taps, w, b, corrections=False), rows[0], rows[1], fl)
    _CASES[shape] = res
    return res


@pytest.mark.parametrize("shape", R.SHAPES)
def test_split_tile_is_as_close_to_fp64_as_the_whole_k_tile(dev, shape):
    from videotgb_amd import ops
    case = _case(dev, shape)
    for kind in ("zero", "uniform", "integer", "mix"):
        ref, ref16, r0, r1, _ = case[kind]
        e0, e1 = (R.rel_err(ops.pair_unpack(r, 256).cpu(), ref) for r in (r0, r1))
        d16 = R.rel_err(ref16, ref)
        print(f"[lookup+convc1 {shape} {kind}] err(0) = {e0:.3e}  err(1) = {e1:.3e}  fp16-only reference: {d16:.3e} = {d16 / max(e0, 1e-30):.1f} x err(0)")
        assert d16 >= 4 * 1.5 * e0          # the inputs show the fp8 half
        assert e1 <= 1.5 * e0
        assert e0 < d16 / 4 and e1 < d16 / 4


@pytest.mark.parametrize("shape", R.SHAPES)
def test_windows_outside_every_level_give_relu_bias(dev, shape):
    from videotgb_amd import ops
    case = _case(dev, shape)
    _, _, b, _ = case["inputs"]
    _, _, r0, r1, _ = case["outside"]
    want = ops.pair_pack(b.relu().view(1, 256).expand(r0.shape[0], 256).contiguous().to(dev))
    assert torch.equal(r0, want) and torch.equal(r1, want)


@pytest.mark.parametrize("variant", [0, 1])
def test_a_pixel_does_not_depend_on_its_batch(dev, variant):
    from videotgb_amd import ops
    # tiles that straddle images: the five pairs one by one
    n, H8, W8 = 5, 16, 16
    case = _case(dev, (n, H8, W8))
    pyr, w, b, pd = case["inputs"]
    full, fl = case["mix"][2 + variant], case["mix"][4]
    HW = H8 * W8
    for i in range(n):
        sl = slice(i * HW, (i + 1) * HW)
        one = ops.raft_lookup_convc1([p[sl].contiguous() for p in pd], fl[sl].to(dev), w, b, H8, W8, variant=variant)
        assert torch.equal(one, full[sl]), f"pair {i}"
    # M = 234 (a partial last tile: a wave with 2 of its 8 pixels, waves with none) inside a larger call: rows 0 .. 233 unchanged
    n, H8, W8 = 2, 9, 13
    case = _case(dev, (n, H8, W8))
    pyr, w, b, pd = case["inputs"]
    small, fl = case["mix"][2 + variant], case["mix"][4]
    pyr2, _, _ = R.make_inputs(1, H8, W8, seed=7)
    fl2 = R.make_flow("mix", 1, H8, W8, seed=7)
    big = ops.raft_lookup_convc1([torch.cat([a, c.to(dev)]) for a, c in zip(pd, pyr2)], torch.cat([fl, fl2]).to(dev), w, b, H8, W8, variant=variant)
    assert small.shape[0] == 234 and torch.equal(big[:234], small)


@pytest.mark.parametrize("variant", [0, 1])
def test_three_calls_return_equal_bits(dev, variant):
    from videotgb_amd import ops
    n, H8, W8 = 3, 28, 28
    case = _case(dev, (n, H8, W8))
    pyr, w, b, pd = case["inputs"]
    first, fl = case["uniform"][2 + variant], case["uniform"][4].to(dev)
    for _ in range(2):
        assert torch.equal(ops.raft_lookup_convc1(pd, fl, w, b, H8, W8, variant=variant), first)


def test_two_workgroups_of_the_split_tile_are_resident_per_cu(dev):
    from videotgb_amd import ops
    n, H8, W8 = 2, 9, 13
    pyr, w, b, pd = _case(dev, (n, H8, W8))["inputs"]
    fl = R.make_flow("zero", n, H8, W8).to(dev)
    occ = [ops.raft_lookup_convc1(pd, fl, w, b, H8, W8, variant=v, want_occupancy=True)[1] for v in (0, 1)]
    print(f"[lookup+convc1] resident workgroups per CU: whole-K tile {occ[0]}, split-K tile {occ[1]}")
    assert occ[1] == 2 and occ[0] == 1
