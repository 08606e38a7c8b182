"""-m gpu: ops.beam_candidates_eos (vtgb_llm_beam_candidates_eos), the list instantiation of the beam candidate kernel.

With a one-element list its scores and indices are ops.beam_candidates' BIT FOR BIT on every case of tests/beam_refs.py.  With three ids it is
compared with the fp64 reference called with the list, on the cases' logits with 20.0 planted at all three ids, under the rule of
tests/test_gpu_beam_candidates.py: indices equal, scores within its SCORE_TOL, on inputs whose consecutive reference candidates are GAP apart.
The three planted values of a row are equal numbers, so where the ids are free the reference has exact ties: those are resolved by ascending
index in the reference (a stable sort) and in the kernel alike, and the gap condition is asked of every other pair of neighbours."""
import functools

import pytest
import torch

import beam_refs as R
import test_gpu_beam_candidates as TC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return "cuda:0"


def _both(case, dev, ids):
    from videotgb_amd import ops
    x, seq, step, run = case["logits"].to(dev), case["seq"].to(dev), torch.tensor([case["step"]], device=dev), case["running"].to(dev)
    return x, seq, step, run, ops.eos_list(ids, x.shape[1], dev)


@pytest.mark.parametrize("V", R.VOCABS)
@pytest.mark.parametrize("K", R.BEAMS)
def test_a_one_element_list_equals_the_one_id_entry_bit_for_bit(dev, V, K):
    from videotgb_amd import ops
    cases = [R.candidate_case(V, K, B, bf16, variant) for B in R.BATCHES for bf16 in (False, True) for variant in (0, 1, 2)]
    cases += [R.tie_case(V, K, B, bf16) for B in R.BATCHES for bf16 in (False, True)]
    for case in cases:
        eos = case["eos"]
        x, seq, step, run, lst = _both(case, dev, [] if eos is None else [eos])
        s0, i0 = ops.beam_candidates(x, seq, step, run, case["penalty"], eos, case["min_new"])
        s1, i1 = ops.beam_candidates_eos(x, seq, step, run, lst, case["penalty"], case["min_new"])
        assert torch.equal(i0, i1) and torch.equal(s0.view(torch.int32), s1.view(torch.int32)), (V, K, case["step"], case["min_new"])
        if eos is not None:      # the id twice: the same again
            s2, i2 = ops.beam_candidates_eos(x, seq, step, run, ops.eos_list([eos, eos], V, dev), case["penalty"], case["min_new"])
            assert torch.equal(i0, i2) and torch.equal(s0.view(torch.int32), s2.view(torch.int32))


def _gap_but_exact_ties(case, K):
    """beam_refs._gap over the first 2K + 1 reference candidates, exact ties (the planted equal values) left out; inf when all tie."""
    s, _ = R.candidates_ref(n=2 * K + 1, **case)
    d = s[:, :-1] - s[:, 1:]
    d = d[d != 0]
    return float(d.min()) if d.numel() else float("inf")


@functools.lru_cache(maxsize=None)
def _three_id_case(V, K, B, bf16, variant):
    """The case of beam_refs with 20.0 planted at three ids -- its own eos and two more, the first draw from a fixed seed for which the
    reference's neighbours are equal or GAP apart (the search reads the reference alone)."""
    base = R.candidate_case(V, K, B, bf16, variant)
    g = torch.Generator().manual_seed(4242 + V + 7 * K + B + int(bf16) + 3 * variant)
    for _ in range(64):
        more = [int(t) for t in torch.randint(0, V, (2,), generator=g)]
        ids = [base["eos"]] + more
        if len(set(ids)) < 3:
            continue
        x = base["logits"].clone()
        x[:, ids] = 20.0
        case = dict(base, logits=x, eos=ids)
        free = not case["step"] < case["min_new"]      # free ids: the draw must put all three among the reference's candidates
        if _gap_but_exact_ties(case, K) >= R.GAP and (not free or set(ids) <= set((R.candidates_ref(**case)[1] % V).flatten().tolist())):
            return case
    raise AssertionError("no three ids with the reference's gap")


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("V,K,B", [(120, 5, 1), (1000, 2, 1), (1000, 5, 3), (32000, 8, 1), (32001, 5, 3), (32001, 2, 3)])
def test_three_ids_against_the_reference(dev, V, K, B, bf16):
    from videotgb_amd import ops
    for variant in (0, 1, 2):
        case = _three_id_case(V, K, B, bf16, variant)
        ids = case["eos"]
        assert _gap_but_exact_ties(case, K) >= R.GAP
        ref_s, ref_i = R.candidates_ref(**case)
        x, seq, step, run, lst = _both(case, dev, ids)
        score, idx = ops.beam_candidates_eos(x, seq, step, run, lst, case["penalty"], case["min_new"])
        err = (score.cpu().double() - ref_s).abs().max().item()
        print(f"V={V} K={K} B={B} bf16={bf16} variant={variant}: |score - fp64| {err:.3e}")
        assert torch.equal(idx.cpu().long(), ref_i), (variant, idx.cpu().tolist(), ref_i.tolist())
        assert err <= TC.SCORE_TOL, (variant, err)
        tokens = set((idx.cpu().long() % V).flatten().tolist())
        blocked = case["step"] < case["min_new"]
        if blocked:      # none of the three ids is a candidate although each holds its row's largest logit
            assert not tokens & set(ids), (variant, tokens)
            one = ops.beam_candidates_eos(x, seq, step, run, ops.eos_list(ids[:1], V, dev), case["penalty"], case["min_new"])[1]
            assert set((one.cpu().long() % V).flatten().tolist()) & set(ids[1:])      # (blocking the first id alone lets the others through)
        else:            # free: all three are
            assert set(ids) <= tokens, (variant, tokens)


def test_out_and_workspace_operands_are_used(dev):
    """Nothing is allocated when ``out`` and ``workspace`` are given: the results are the caller's tensors."""
    from videotgb_amd import ops
    case = R.candidate_case(1000, 5, 3, True, 0)
    x, seq, step, run, lst = _both(case, dev, [case["eos"], 3, 4])
    out = (torch.zeros(3, 10, device=dev), torch.zeros(3, 10, dtype=torch.int32, device=dev))
    ws = torch.zeros(ops.beam_candidates_workspace_bytes(15, 5, 1000), dtype=torch.uint8, device=dev)
    s, i = ops.beam_candidates_eos(x, seq, step, run, lst, case["penalty"], case["min_new"], out=out, workspace=ws)
    assert s is out[0] and i is out[1]
    s2, i2 = ops.beam_candidates_eos(x, seq, step, run, lst, case["penalty"], case["min_new"])
    assert torch.equal(s, s2) and torch.equal(i, i2)
