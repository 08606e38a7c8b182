"""The acceptance rules of tests/llm_refs.py, shown to have teeth without a GPU: fp32 torch arithmetic standing in for the kernels of
csrc/llm.hip (the same operations in the same places, rounded where the kernels round) passes every rule on the input sets of
tests/test_gpu_llm_kernels.py with an off-centre share of at most a tenth of the cap, and each mutant -- one plausible kernel bug
each -- is rejected by the rule meant to catch it."""
import pytest
import torch

import llm_refs as R
from llm_refs import BF16, F32

TENTH = R.CAP / 10


# ------------------------------------------------------------------------------------------------------- the kernels in fp32 torch arithmetic
def emul_rmsnorm(x, delta, w, eps, dtype, mutant=None):
    """-> x_after, h as llm_rmsnorm_kernel / llm_rmsnorm_vec_kernel compute them"""
    H = x.shape[-1]
    v = x.float() if delta is None else (x.float() + delta.float()).to(dtype).float()
    sq = x.float() if mutant == "delta_after_variance" else v
    ss = (sq * sq).sum(-1, keepdim=True)
    var = ss / float(256 * ((H + 255) // 256) if mutant == "padded_mean" else H)
    e = torch.tensor(eps, dtype=F32)
    rs = 1.0 / (var.sqrt() + e) if mutant == "eps_outside_sqrt" else torch.rsqrt(var + e)
    if mutant == "neighbour_rs":
        rs = rs.roll(1, 0)
    n = v * rs
    if mutant != "n_unrounded":
        n = n.to(dtype).float()
    return v.to(dtype), (w.float() * n).to(dtype)


def emul_act(kind, g, u, dtype, mutant=None):
    """-> act as llm_silu_mul*_kernel (kind 0) / llm_gated_act_kernel compute it (u None: ungated)"""
    gf = g.float()
    if mutant == "exact_gelu_for_gelu_new":
        kind = 3
    if kind == 0:
        f = gf / (1.0 + torch.exp(-gf))
    elif kind == 1:
        f = 0.5 * gf * (1.0 + torch.tanh(0.7978845608028654 * (gf + 0.044715 * gf * gf * gf)))
    elif kind == 2:
        f = torch.clamp_min(gf, 0.0)
    else:
        f = 0.5 * gf * (1.0 + torch.erf(gf * 0.70710678118654752440))
    if mutant != "s_unrounded":
        f = f.to(dtype).float()
    if u is None:
        return f.to(dtype)
    uf = u.float().roll(-1, -1) if mutant == "u_from_next_column" else u.float()
    return (f * uf).to(dtype)


def emul_parts_sum(part, S, M, cols, mutant=None):
    """-> [M, cols] bf16 as parts_sum reads a FLAT fragment buffer: element (r, i) = the sum over sp, ascending, of
    flat[(((i >> 7) S + sp) M + r) 128 + (i & 127)], rounded once"""
    flat = part.reshape(-1)
    nb = cols // 128
    i = torch.arange(cols)
    b, c = i >> 7, i & 127
    r = torch.arange(M)[:, None]
    acc = torch.zeros(M, cols)
    for sp in range(S):
        tile = (sp * nb + b) if mutant == "splits_and_tiles_swapped" else (b * S + sp)
        acc = acc + flat[(tile[None] * M + r) * 128 + c[None]]
    return acc.bfloat16()


def _rms_cases():
    for dtype in (BF16, F32):
        for rows, H in R.RMS_SHAPES[dtype]:
            for with_delta in (True, False):
                for eps in R.RMS_EPS:
                    yield dtype, rows, H, with_delta, eps


# -------------------------------------------------------------------------------------------------------------------------- the rules pass
def test_bf16_neighbours_and_single_rounding():
    t = torch.tensor([1.0, -1.0, 0.0, -0.0, 3.3895e38, 9.1835e-41], dtype=BF16)
    lo, hi = R.bf16_neighbours(t)
    assert lo[0].item() == 1.0 - 2.0 ** -8 and hi[0].item() == 1.0 + 2.0 ** -7
    assert lo[1].item() == -1.0 - 2.0 ** -7 and hi[1].item() == -1.0 + 2.0 ** -8
    assert hi[2].item() == hi[3].item() == -lo[2].item() == -lo[3].item() == 2.0 ** -133
    assert torch.isinf(hi[4]) and lo[5].item() == 0.0
    x = torch.randn(4096, generator=torch.Generator().manual_seed(0)).bfloat16()
    lo, hi = R.bf16_neighbours(x)
    assert (lo < x).all() and (x < hi).all()
    assert R.same_bits(R.bf16_neighbours(lo)[1], x) and R.same_bits(R.bf16_neighbours(hi)[0], x)
    # 1 + 2^-8 + 2^-40 lies above the tie between 1 and 1 + 2^-7: one rounding goes up, the two roundings through fp32 go to even (down)
    v = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40, 1.0 + 2.0 ** -8 - 2.0 ** -40, 1.0 + 2.0 ** -8], dtype=torch.float64)
    assert R.rnd(v, BF16).tolist() == [1.0 + 2.0 ** -7, 1.0, 1.0]
    assert v.float().bfloat16().tolist() == [1.0, 1.0, 1.0]


def test_fp32_arithmetic_passes_the_rmsnorm_rule_on_the_gpu_input_sets():
    """Measured here (torch 2.x CPU, every bf16 case of RMS_SHAPES x delta x eps): 0 of the elements off the centre value, none outside
    the three candidates."""
    off = total = 0
    for k, (dtype, rows, H, with_delta, eps) in enumerate(_rms_cases()):
        x, delta, w = R.rmsnorm_inputs(rows, H, dtype, seed=k)
        delta = delta if with_delta else None
        x_after, h = emul_rmsnorm(x, delta, w, eps, dtype)
        share = R.check_rmsnorm(h, x_after, x, delta, w, eps, dtype)
        if dtype == BF16:
            off, total = off + share * h.numel(), total + h.numel()
        if rows > 1:
            assert not h[-1].any()
    print(f"rmsnorm bf16: off-centre share {off / total:.3e} of {total} elements")
    assert off / total <= TENTH


def _act_sets():
    for k, (rows, I) in enumerate(R.SILU_SHAPES):
        yield 100 + k, rows, I


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_fp32_arithmetic_passes_the_activation_rule_on_the_gpu_input_sets(kind):
    """Measured here (torch CPU fp32 as the kernel, every shape of SILU_SHAPES, gated and ungated, bf16; shares are off-centre elements
    over the elements of the capped range):
      SiLU      g >= -88    0          (all g: 4.3e-6 -- the g = -90 edge of each call, where expf overflows; accepted by the floor)
      gelu_new  g >= -1     0          (all g: 6.6e-2)
      gelu      g >= -1     0          (all g: 6.0e-2)
    (1.6 M elements, gated and ungated each), so the GELU kinds stay capped on g >= -1 (llm_refs.GELU_CAP_FROM); the whole-range share is what the
    cancellation in 1 + tanh / 1 + erf costs in fp32 at g < -1 and is not a defect."""
    off = total = off_all = total_all = 0
    for seed, rows, I in _act_sets():
        for dtype in (BF16, F32):
            g, u = R.act_inputs(rows, I, dtype, seed)
            for uu in (u, None):
                got = emul_act(kind, g, uu, dtype)
                share = R.check_act(got, kind, g, uu, dtype)
                if dtype == BF16 and kind != 2:
                    n = int((g.double() >= (R.SILU_CAP_FROM if kind == 0 else R.GELU_CAP_FROM)).sum())
                    off, total = off + share * n, total + n
                    centre = R.act_ref(kind, g, uu, dtype)[1]
                    off_all, total_all = off_all + int((got != centre).sum()), total_all + g.numel()
    if kind != 2:
        print(f"{R.KINDS[kind]} bf16: off-centre share {off / total:.3e} on the capped range, {off_all / total_all:.3e} over all g")
        assert off / total <= TENTH


def test_fragment_builder_states_the_layout_parts_sum_reads():
    for cols, S, M in ((4096, 2, 1), (2048, 7, 5), (1152, 3, 3)):
        part, delta = R.make_fragments(cols, S, M, seed=S)
        assert part.shape == (cols // 128, S, M, 128) and part.dtype == F32 and delta.dtype == BF16
        assert R.same_bits(emul_parts_sum(part, S, M, cols), delta)


# ------------------------------------------------------------------------------------------------------------------- the mutants are rejected
@pytest.mark.parametrize("mutant,dtype,rows,H,eps", [
    ("neighbour_rs", BF16, 3, 4096, 1e-6), ("neighbour_rs", F32, 3, 2048, 1e-6), ("neighbour_rs", BF16, 130, 4096, 1e-5),
    ("padded_mean", BF16, 4, 257, 1e-6), ("padded_mean", F32, 2, 100, 1e-5), ("padded_mean", BF16, 2, 100, 1e-6),
    ("n_unrounded", BF16, 3, 4096, 1e-6), ("n_unrounded", BF16, 4, 257, 1e-5),
    ("eps_outside_sqrt", BF16, 3, 4096, 1e-6), ("eps_outside_sqrt", F32, 3, 4096, 1e-6), ("eps_outside_sqrt", BF16, 4, 257, 1e-5),
    ("delta_after_variance", BF16, 3, 2048, 1e-6), ("delta_after_variance", F32, 4, 257, 1e-5),
])
def test_rmsnorm_mutants_are_rejected(mutant, dtype, rows, H, eps):
    x, delta, w = R.rmsnorm_inputs(rows, H, dtype, seed=7)
    x_after, h = emul_rmsnorm(x, delta, w, eps, dtype)
    R.check_rmsnorm(h, x_after, x, delta, w, eps, dtype)                       # (the unmutated arithmetic passes on these inputs)
    x_after, h = emul_rmsnorm(x, delta, w, eps, dtype, mutant)
    with pytest.raises(AssertionError, match="rmsnorm"):
        R.check_rmsnorm(h, x_after, x, delta, w, eps, dtype)


def test_rmsnorm_rule_rejects_a_wrong_residual():
    x, delta, w = R.rmsnorm_inputs(3, 2048, BF16, seed=8)
    x_after, h = emul_rmsnorm(x, delta, w, 1e-6, BF16)
    x_after[0, 5] = R.bf16_neighbours(x_after[0, 5:6])[1][0]
    with pytest.raises(AssertionError, match="one rounding"):
        R.check_rmsnorm(h, x_after, x, delta, w, 1e-6, BF16)
    with pytest.raises(AssertionError, match="one rounding"):                    # delta == NULL: x is untouched
        R.check_rmsnorm(h, x_after, x, None, w, 1e-6, BF16)


@pytest.mark.parametrize("mutant,kind,dtype,rows,I", [
    ("s_unrounded", 0, BF16, 3, 11008), ("s_unrounded", 0, BF16, 3, 100),
    ("u_from_next_column", 0, BF16, 3, 100), ("u_from_next_column", 0, F32, 5, 7), ("u_from_next_column", 0, BF16, 2, 2056),
    ("exact_gelu_for_gelu_new", 1, BF16, 3, 100), ("exact_gelu_for_gelu_new", 1, F32, 3, 100), ("exact_gelu_for_gelu_new", 1, BF16, 300, 3501),
])
def test_activation_mutants_are_rejected(mutant, kind, dtype, rows, I):
    g, u = R.act_inputs(rows, I, dtype, seed=9)
    R.check_act(emul_act(kind, g, u, dtype), kind, g, u, dtype)
    with pytest.raises(AssertionError, match=R.KINDS[kind]):
        R.check_act(emul_act(kind, g, u, dtype, mutant), kind, g, u, dtype)


def test_relu_rule_is_exact():
    g, u = R.act_inputs(3, 100, BF16, seed=10)
    got = emul_act(2, g, u, BF16)
    R.check_act(got, 2, g, u, BF16)
    i = int((got[0] != 0).nonzero()[0])
    got[0, i] = R.bf16_neighbours(got[0, i:i + 1])[1][0]
    with pytest.raises(AssertionError, match="relu"):
        R.check_act(got, 2, g, u, BF16)


@pytest.mark.parametrize("cols,S,M", [(4096, 2, 1), (2048, 3, 5), (1536, 5, 3)])
def test_parts_sum_with_splits_and_tiles_swapped_is_rejected(cols, S, M):
    part, delta = R.make_fragments(cols, S, M, seed=11)
    assert R.same_bits(emul_parts_sum(part, S, M, cols), delta)
    assert not R.same_bits(emul_parts_sum(part, S, M, cols, "splits_and_tiles_swapped"), delta)
    # ... and through the consumer's rule: x afterwards must be bf16(x + delta) bit for bit
    x, _, w = R.rmsnorm_inputs(M, cols, BF16, seed=12)
    wrong = emul_parts_sum(part, S, M, cols, "splits_and_tiles_swapped")
    x_after, h = emul_rmsnorm(x, wrong, w, 1e-6, BF16)
    with pytest.raises(AssertionError, match="one rounding"):
        R.check_rmsnorm(h, x_after, x, delta, w, 1e-6, BF16)
