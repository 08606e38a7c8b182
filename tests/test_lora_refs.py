"""The rule of tests/lora_refs.py on the host: it accepts two fp32 emulations of the LoRA update with different summation orders, and
rejects the mistakes a kernel or its caller could make."""
import pytest
import torch

import lora_refs as R

CASES = [(torch.float32, 256, 8, 4.0), (torch.bfloat16, 256, 8, 4.0), (torch.float32, 96, 3, 0.3), (torch.bfloat16, 96, 64, 0.3)]


@pytest.mark.parametrize("dtype,K,r,scaling", CASES)
@pytest.mark.parametrize("order", ["sequential", "pairwise"])
def test_the_rule_accepts_fp32_emulations_in_either_summation_order(dtype, K, r, scaling, order):
    x, y, segs = R.make_case(dtype, K, r, 5, scaling)
    got = R.emulate(x, y, segs, order)
    assert R.verdict(x, y, segs, got) is None
    assert not torch.equal(got, y)


def test_the_two_emulations_differ_somewhere():
    """(Otherwise "either order" would be one order.)  fp32, where no output rounding hides the last bits."""
    x, y, segs = R.make_case(torch.float32, 256, 8, 17, 4.0)
    assert not torch.equal(R.emulate(x, y, segs, "sequential"), R.emulate(x, y, segs, "pairwise"))


def _mutants(x, y, segs):
    (c0, A0, B0, s0), (c1, A1, B1, s1) = segs
    good = R.emulate(x, y, segs, "sequential")
    out = {"the adapter is ignored": y.clone(),
           "the scaling is dropped": R.emulate(x, y, [(c0, A0, B0, 1.0), (c1, A1, B1, 1.0)]),
           "A and B of the two segments are swapped": R.emulate(x, y, [(c0, A1, B0[:, :], s0), (c1, A0, B1, s1)])}
    n = min(B0.shape[0], B1.shape[0])
    wrong = y.clone()      # segment 0's d lands on segment 1's columns (and segment 0 stays as it was)
    wrong[:, c1: c1 + n] = R.emulate(x, y[:, c1: c1 + n], [(0, A0, B0[:n], s0)])
    out["d is added into the neighbouring segment"] = wrong
    stray = good.clone()
    stray[2, 40] = (stray[2, 40].float() + 1.0).to(y.dtype)      # column 40 belongs to no segment
    out["a write lands in an untouched column"] = stray
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("scaling", [4.0, 0.3])
def test_the_rule_rejects_the_mutants(dtype, scaling):
    x, y, segs = R.make_case(dtype, 256, 8, 5, scaling)
    assert R.verdict(x, y, segs, R.emulate(x, y, segs)) is None
    for name, got in _mutants(x, y, segs).items():
        assert R.verdict(x, y, segs, got) is not None, name


def test_the_rule_rejects_non_finite_values_and_a_single_wrong_value():
    x, y, segs = R.make_case(torch.float32, 256, 8, 5, 4.0)
    good = R.emulate(x, y, segs)
    bad = good.clone()
    bad[1, 3] = float("inf")
    assert "non-finite" in R.verdict(x, y, segs, bad)
    bad = good.clone()
    bad[4, 70] = bad[4, 70] + 1e-3      # far above e (~1e-5 here), far below d
    assert R.verdict(x, y, segs, bad) is not None
