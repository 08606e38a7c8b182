"""-m gpu: ops.beam_candidates (vtgb_llm_beam_candidates) against the fp64 reference of tests/beam_refs.py.

Indices must EQUAL the reference's: the cases are generated (beam_refs.candidate_case) so that the reference's consecutive candidates among
the first 2K + 1 are at least 1e-3 apart, which is asserted here on every case and in test_beam_refs.py on the CPU.
Scores: the torch fp32 statement of the same rule (log_softmax, penalty, + running at fp32: what transformers computes) deviates from fp64
by at most 7.66e-6 on these inputs (scores of magnitude 10 .. 16, fp32 spacing 9.5e-7; measured over all 144 cases on the CPU, printed
per case below); the kernel, whose sums run in another order, gets 4 x that: SCORE_TOL = 3.07e-5."""
import pytest
import torch

import beam_refs as R

pytestmark = pytest.mark.gpu

TORCH_FP32_DEVIATION = 7.66e-6
SCORE_TOL = 4 * TORCH_FP32_DEVIATION


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return "cuda:0"


def _run(case, dev):
    from videotgb_amd import ops
    return ops.beam_candidates(case["logits"].to(dev), case["seq"].to(dev), torch.tensor([case["step"]], device=dev), case["running"].to(dev),
                               case["penalty"], case["eos"], case["min_new"])


@pytest.mark.parametrize("V", R.VOCABS)
@pytest.mark.parametrize("K", R.BEAMS)
def test_candidates_equal_the_reference(dev, V, K):
    for B in R.BATCHES:
        for bf16 in (False, True):
            for variant in (0, 1, 2):
                case = R.candidate_case(V, K, B, bf16, variant)
                assert R._gap(case, K) >= R.GAP
                ref_s, ref_i = R.candidates_ref(**case)
                t32 = R.candidates_ref(dtype=torch.float32, **case)[0]
                score, idx = _run(case, dev)
                assert score.shape == idx.shape == (B, 2 * K) and score.dtype == torch.float32 and idx.dtype == torch.int32
                err = (score.cpu().double() - ref_s).abs().max().item()
                print(f"V={V} K={K} B={B} bf16={bf16} variant={variant}: |score - fp64| {err:.3e} (torch fp32: {(t32.double() - ref_s).abs().max().item():.3e})")
                assert torch.equal(idx.cpu().long(), ref_i), (B, bf16, variant)
                assert err <= SCORE_TOL, (B, bf16, variant, err)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("V,K,B", [(120, 2, 1), (1000, 5, 3), (32001, 8, 3)])
def test_exact_ties_come_in_ascending_flat_index(dev, V, K, B, bf16):
    """Identical rows with equal running scores: a row's bits do not depend on its place, so every score occurs K times exactly."""
    case = R.tie_case(V, K, B, bf16)
    ref_s, ref_i = R.candidates_ref(**case)
    score, idx = _run(case, dev)
    assert torch.equal(idx.cpu().long(), ref_i)
    s = score.cpu()
    assert torch.equal(s[:, :K], s[:, :1].expand(B, K)) and torch.equal(s[:, K:], s[:, K: K + 1].expand(B, K))
    assert (s.double() - ref_s).abs().max().item() <= SCORE_TOL


def test_a_rows_bits_do_not_depend_on_batch_beams_or_place(dev):
    V = 32001
    case = R.candidate_case(V, 5, 3, True, 1)
    x, seq = case["logits"].to(dev), case["seq"].to(dev)
    step = torch.tensor([case["step"]], device=dev)
    from videotgb_amd import ops
    zero = torch.zeros(3, 5, device=dev)
    s_all, i_all = ops.beam_candidates(x, seq, step, zero, 1.5)
    for r in (0, 7, 14):      # the row alone, as a batch of one beam: its own 2 best
        s1, i1 = ops.beam_candidates(x[r: r + 1].contiguous(), seq[r: r + 1].contiguous(), step, torch.zeros(1, 1, device=dev), 1.5)
        b, k = divmod(r, 5)
        mine = (i_all[b] // V) == k
        got = s_all[b][mine][:2]
        assert torch.equal(got, s1[0][: got.numel()]) and torch.equal((i_all[b][mine][:2] % V), i1[0][: got.numel()])
