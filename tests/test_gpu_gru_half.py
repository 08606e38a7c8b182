"""-m gpu: the two gate launches of a SepConvGRU half-step of vtgb_raft_update's refinement loop at f16c8 and bf16x3, through their unit entry (include/vtgb.h
vtgb_raft_gru_half -- the launches the loop itself runs, csrc/raft_x3.hip x3_gru_half) against the same arithmetic in fp64 (tests/gru_ref.py).

Every launch is judged on its own: the q launch's reference reads the DEVICE's z and r h.  Bounds (gru_ref.py; none fixed in advance, every one built
from reference-only quantities computed on the CPU and printed): e_f32 = what fp32 accumulation alone costs on the launch's pre-activation, E = 4 e_f32,
T = 2^-20 for the fast sigmoid / tanh, P = the pair encoding's own error;
    |z - z_ref| <= E / 4 + T      |rh - r_ref h| <= |h| (E / 4 + T) + P(r_ref h)      |h' - h'_ref| <= z (E + T) + P(h'_ref) + 4 2^-24 (|h| + 1)
A single dropped correction product is >= 99 x (f16c8) / >= 1398 x (bf16x3) these bounds away on the same inputs (tests/test_gru_half_abi.py, CPU).
Measured on an MI355X: the table in DESIGN.md section 4."""
import pytest
import torch

import gru_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


_CASES = {}


def _to(dev, d):
    return {k: v.to(dev) for k, v in d.items() if not k.startswith("sat_")}


def _case(dev, fmt, shape, half, extremes=False):
    """Inputs, both launches' device outputs (z | r, then q on a copy of h from the device's own z and r h) and their fp64 references, computed once."""
    key = (fmt, shape, half, extremes)
    if key in _CASES:
        return _CASES[key]
    from videotgb_amd import ops
    f = R.FMT[fmt]
    n, H8, W8 = shape
    d = R.make_inputs(n, H8, W8, half, extremes=extremes)
    s0 = R.stage0(f, d, shape, half)
    e0 = R.e_f32(f, s0["h_rows"], s0["x_rows"], d["w_zr"], d["start_zr"], shape, half, s0["pre"])
    g = _to(dev, d)
    g["h_rows"], g["x_rows"] = s0["h_rows"].to(dev), s0["x_rows"].to(dev)
    z, rh, _ = ops.raft_gru_half(f, g["h_rows"], g["x_rows"], g["start_zr"], None, g["w_zr"], None, H8, W8, half, stage=0)
    hq = g["h_rows"].clone()
    ops.raft_gru_half(f, g["h_rows"], g["x_rows"], None, g["start_q"], None, g["w_q"], H8, W8, half, stage=1, rh=rh, z=z, h_q=hq)
    s1 = R.stage1(f, d, shape, half, rh.cpu(), z.cpu(), s0["h_rows"], s0["x_rows"])
    e1 = R.e_f32(f, rh.cpu(), s0["x_rows"], d["w_q"], d["start_q"], shape, half, s1["pre"])
    _CASES[key] = dict(f=f, d=d, g=g, s0=s0, s1=s1, e0=e0, e1=e1, z=z, rh=rh, hq=hq)
    return _CASES[key]


def _check_stage0(tag, f, s0, e0, z_dev, rh_dev):
    """Bound (a) of the z | r launch; returns the two ratios to the bound."""
    z, rh = z_dev.cpu().double(), R.pair_value(rh_dev, f)
    assert torch.isfinite(z).all() and torch.isfinite(rh).all()
    ez, erh = (z - s0["z"]).abs(), (rh - s0["rh"]).abs()
    qz, qrh = float((ez / R.bound_z(e0)).max()), float((erh / R.bound_rh(e0, s0["hval"], s0["rh"], f)).max())
    print(f"[gru half {tag} z|r] max |pre| = {float(s0['pre'].abs().max()):.1f}  e_f32 = {e0:.2e}  max |z - ref| = {float(ez.max()):.2e} = {qz:.2f} x its bound"
          f" ({R.bound_z(e0):.2e})  max |rh - ref| = {float(erh.max()):.2e}, {qrh:.2f} x its bound")
    assert qz <= 1.0 and qrh <= 1.0
    return qz, qrh


def _check_stage1(tag, f, s1, e1, hq_dev):
    h_new = R.pair_value(hq_dev, f)
    assert torch.isfinite(h_new).all()
    eh = (h_new - s1["h_new"]).abs()
    qh = float((eh / R.bound_h(e1, s1["z"], s1["hval"], s1["h_new"], f)).max())
    print(f"[gru half {tag} q  ] max |pre| = {float(s1['pre'].abs().max()):.1f}  e_f32 = {e1:.2e}  max |h' - ref| = {float(eh.max()):.2e}, {qh:.2f} x its bound")
    assert qh <= 1.0
    return qh


# ---- a. each launch against fp64
@pytest.mark.parametrize("stage", [0, 1])
@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("fmt", ["f16c8", "bf16x3"])
@pytest.mark.parametrize("shape", R.SHAPES)
def test_launch_vs_fp64(dev, shape, fmt, half, stage):
    c = _case(dev, fmt, shape, half)
    tag = f"{fmt} {shape} half={half}"
    if stage == 0:
        _check_stage0(tag, c["f"], c["s0"], c["e0"], c["z"], c["rh"])
    else:
        _check_stage1(tag, c["f"], c["s1"], c["e1"], c["hq"])


# ---- b. saturated gates, zeros and the smallest magnitudes of h
@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("fmt", ["f16c8", "bf16x3"])
def test_saturated_gates_stay_finite_and_exact(dev, fmt, half):
    shape = (5, 16, 16)
    c = _case(dev, fmt, shape, half, extremes=True)
    f, d, s0, s1 = c["f"], c["d"], c["s0"], c["s1"]
    tag = f"{fmt} {shape} half={half} extremes"
    _check_stage0(tag, f, s0, c["e0"], c["z"], c["rh"])      # (finite everywhere: no NaN from exp overflow)
    _check_stage1(tag, f, s1, c["e1"], c["hq"])
    z, rh, h_new, hval = c["z"].cpu().double(), R.pair_value(c["rh"], f), R.pair_value(c["hq"], f), s0["hval"]
    rows, cols, sign = d["sat_zr"]
    up = (sign > 0).double()
    isz = cols < 128
    assert isz.any() and (~isz).any()
    assert ((z[rows[isz], cols[isz]] - up[isz]).abs() <= R.T).all()                                        # z within T of 0 or 1
    rr, rc = rows[~isz], cols[~isz] - 128
    want = up[~isz] * hval[rr, rc]                                                                         # r h within bound of 0 or h
    assert ((rh[rr, rc] - want).abs() <= hval[rr, rc].abs() * R.T + R.P(want, f)).all()
    rows, cols, sign = d["sat_q"]
    zq, hq = s1["z"][rows, cols], s1["hval"][rows, cols]
    want = (1.0 - zq) * hq + sign.double() * zq                                                            # h' = (1 - z) h +- z within bound
    assert ((h_new[rows, cols] - want).abs() <= zq * R.T + R.P(want, f) + 4.0 * 2.0 ** -24 * (hq.abs() + 1.0)).all()


# ---- c. the narrow and the wide tile of the f16c8 z | r launch agree bit for bit; for the other launches: a pixel does not depend on its batch
_BIG = {}


def _wide_batch(dev):
    """Images of 16 x 16 (one 256-row m-tile each) that launch_conv_h8's cost model gives the 256-wide tile, from the device's CU count."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count      # (hipDeviceAttributeMultiprocessorCount)

    def narrow(m_tiles):
        return ((2 * m_tiles + cus - 1) // cus) * 1.1 < ((m_tiles + cus - 1) // cus) * 2.0

    n = next(m for m in range(3, 8 * cus) if not narrow(m)) + 3      # (256 CUs: 132)
    assert not narrow(n) and narrow(2)
    return n


def _big(dev, fmt, half):
    key = (fmt, half)
    if key not in _BIG:
        from videotgb_amd import ops
        f, n = R.FMT[fmt], _wide_batch(dev)
        d = R.make_inputs(n, 16, 16, half, seed=3)
        g = _to(dev, d)
        g["h_rows"], g["x_rows"] = R.pack_pair(d["h"], f).to(dev), R.pack_pair(d["x"], f).to(dev)
        z, rh, _ = ops.raft_gru_half(f, g["h_rows"], g["x_rows"], g["start_zr"], None, g["w_zr"], None, 16, 16, half, stage=0)
        _BIG[key] = (f, n, g, z, rh)
    return _BIG[key]


@pytest.mark.parametrize("stage", [0, 1])
@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("fmt", ["f16c8", "bf16x3"])
def test_first_images_alone_give_the_bits_of_the_large_batch(dev, fmt, half, stage):
    from videotgb_amd import ops
    f, n, g, z, rh = _big(dev, fmt, half)
    m2 = 2 * 256
    cut = lambda t: t[:m2].contiguous()
    if stage == 0:
        z2, rh2, _ = ops.raft_gru_half(f, cut(g["h_rows"]), cut(g["x_rows"]), cut(g["start_zr"]), None, g["w_zr"], None, 16, 16, half, stage=0)
        assert torch.equal(z2, z[:m2]) and torch.equal(rh2, rh[:m2]) and z.abs().max() > 0 and rh.abs().max() > 0
        return
    hq, hq2 = g["h_rows"].clone(), cut(g["h_rows"])
    ops.raft_gru_half(f, g["h_rows"], g["x_rows"], None, g["start_q"], None, g["w_q"], 16, 16, half, stage=1, rh=rh, z=z, h_q=hq)
    ops.raft_gru_half(f, hq2, cut(g["x_rows"]), None, cut(g["start_q"]), None, g["w_q"], 16, 16, half, stage=1, rh=cut(rh), z=cut(z), h_q=hq2)
    assert torch.equal(hq2, hq[:m2]) and not torch.equal(hq, g["h_rows"])


# ---- d. reproducibility, stage 2 = stage 0 then stage 1, and what each launch must leave alone
@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("fmt", ["f16c8", "bf16x3"])
def test_reproducible_and_in_place_safe(dev, fmt, half):
    from videotgb_amd import ops
    shape = (3, 28, 28)
    n, H8, W8 = shape
    c = _case(dev, fmt, shape, half)
    f, g = c["f"], c["g"]
    h0, x0 = g["h_rows"].clone(), g["x_rows"].clone()
    for _ in range(3):      # stage 2, in place on a copy of h (as the loop runs it): the bits of stage 0 followed by stage 1
        h = h0.clone()
        z, rh, hq = ops.raft_gru_half(f, h, g["x_rows"], g["start_zr"], g["start_q"], g["w_zr"], g["w_q"], H8, W8, half, stage=2)
        assert hq is h and torch.equal(z, c["z"]) and torch.equal(rh, c["rh"]) and torch.equal(h, c["hq"])
        assert torch.equal(g["x_rows"], x0)
    # stage 0 leaves h and x alone; stage 1 leaves rh, z and x alone (the case's own runs wrote c["z"], c["rh"], c["hq"] from g)
    z, rh, _ = ops.raft_gru_half(f, g["h_rows"], g["x_rows"], g["start_zr"], None, g["w_zr"], None, H8, W8, half, stage=0)
    assert torch.equal(g["h_rows"], h0) and torch.equal(g["x_rows"], x0) and torch.equal(z, c["z"]) and torch.equal(rh, c["rh"])
    z_in, rh_in, hq = z.clone(), rh.clone(), h0.clone()
    ops.raft_gru_half(f, g["h_rows"], g["x_rows"], None, g["start_q"], None, g["w_q"], H8, W8, half, stage=1, rh=rh, z=z, h_q=hq)
    assert torch.equal(z, z_in) and torch.equal(rh, rh_in) and torch.equal(g["x_rows"], x0) and torch.equal(g["h_rows"], h0)
    assert torch.equal(hq, c["hq"]) and not torch.equal(hq, h0)


# ---- e. the 1x5 half-step hands its in-place h to the 5x1 one
@pytest.mark.parametrize("fmt", ["f16c8", "bf16x3"])
def test_two_half_steps_chained(dev, fmt):
    from videotgb_amd import ops
    shape = (2, 9, 13)
    n, H8, W8 = shape
    f = R.FMT[fmt]
    d = [R.make_inputs(n, H8, W8, half, seed=11) for half in (0, 1)]
    x_rows = R.pack_pair(d[0]["x"], f)
    h = R.pack_pair(d[0]["h"], f).to(dev)
    xg = x_rows.to(dev)
    for half in (0, 1):
        g = _to(dev, d[half])
        h_in = h.clone()
        z, rh, _ = ops.raft_gru_half(f, h, xg, g["start_zr"], g["start_q"], g["w_zr"], g["w_q"], H8, W8, half, stage=2)      # in place on h
        s0 = R.stage0(f, d[half], shape, half, h_rows=h_in, x_rows=x_rows)
        e0 = R.e_f32(f, s0["h_rows"], x_rows, d[half]["w_zr"], d[half]["start_zr"], shape, half, s0["pre"])
        _check_stage0(f"{fmt} chained half={half}", f, s0, e0, z, rh)
        s1 = R.stage1(f, d[half], shape, half, rh.cpu(), z.cpu(), h_in.cpu(), x_rows)
        e1 = R.e_f32(f, rh.cpu(), x_rows, d[half]["w_q"], d[half]["start_q"], shape, half, s1["pre"])
        _check_stage1(f"{fmt} chained half={half}", f, s1, e1, h)
        assert not torch.equal(h, h_in)
