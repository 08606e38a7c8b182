"""tests/beam_refs.py on the host: the fp64 candidate rule against transformers' own pieces (log_softmax, RepetitionPenaltyLogitsProcessor,
MinNewTokensLengthLogitsProcessor, torch.topk) on the same inputs, the tie order, the gather, and the property the GPU test relies on -- the
reference's candidates of every generated case are at least GAP apart."""
import pytest
import torch

import beam_refs as R


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("V,K,B", [(120, 2, 1), (1000, 5, 3), (32001, 8, 1)])
def test_reference_equals_the_transformers_statement(V, K, B, variant):
    case = R.candidate_case(V, K, B, False, variant)
    s64, i64 = R.candidates_ref(**case)
    s32, i32 = R.candidates_ref(dtype=torch.float32, **case)
    hs, hi = R.hf_statement(**case)
    assert torch.equal(i32, hi) and torch.equal(s32, hs)      # the same rule at fp32: the same bits
    assert torch.equal(i64, hi)                               # and at fp64 the same candidates (they are GAP apart)
    assert (s64 - hs.double()).abs().max() < 1e-4
    if variant == 0:      # the blocked eos, which would win every row, is no candidate; only row 0 of every item is
        assert not (i64 % V == case["eos"]).any() and (i64 // V == 0).all()
    else:                 # the penalty moved the best token of a row: it was generated
        assert case["penalty"] == 1.0 or not torch.equal(i64, R.candidates_ref(**dict(case, penalty=1.0))[1])


def test_a_duplicated_id_is_penalised_once_and_ids_behind_step_are_not():
    x = torch.tensor([[2.0, 1.0, 0.5, 0.0]] * 2)
    seq = torch.tensor([[0, 0, 1, 2], [3, 3, 3, 1]])
    s, i = R.candidates_ref(x, seq, 3, torch.zeros(1, 2), penalty=2.0, n=8)
    lp = torch.log_softmax(x.double(), -1)
    want = torch.stack([lp[0] * torch.tensor([2.0, 2.0, 1.0, 1.0]).double(), lp[1] * torch.tensor([1.0, 1.0, 1.0, 2.0]).double()]).reshape(1, 8)
    assert torch.equal(s, want.sort(-1, descending=True).values)


@pytest.mark.parametrize("bf16", [False, True])
def test_equal_scores_come_in_ascending_flat_index(bf16):
    V, K, B = 1000, 5, 3
    case = R.tie_case(V, K, B, bf16)
    s, i = R.candidates_ref(**case)
    assert torch.equal(s[:, :K], s[:, :1].expand(B, K)) and torch.equal(s[:, K:], s[:, K: K + 1].expand(B, K)) and (s[:, 0] > s[:, K]).all()
    assert torch.equal(i[:, :K] // V, torch.arange(K).expand(B, K)) and (i[:, :K] % V == i[:, :1] % V).all()
    assert torch.equal(i[:, K:] // V, torch.arange(K).expand(B, K))


@pytest.mark.parametrize("V", R.VOCABS)
@pytest.mark.parametrize("K", R.BEAMS)
def test_generated_cases_keep_the_gap(V, K):
    for B in R.BATCHES:
        for bf16 in (False, True):
            for variant in (0, 1, 2):
                case = R.candidate_case(V, K, B, bf16, variant)
                assert R._gap(case, K) >= R.GAP


def test_gather_materialises_prompt_then_ancestors():
    B, K, nkv, tp, tg, hd, n_prompt = 2, 3, 2, 8, 4, 2, 5
    R_ = B * K
    cp = torch.arange(B * nkv * tp * hd, dtype=torch.float32).view(B, nkv, tp, hd)
    cg = 1000 + torch.arange(R_ * nkv * tg * hd, dtype=torch.float32).view(R_, nkv, tg, hd)
    src = torch.randint(0, R_, (R_, tg), generator=torch.Generator().manual_seed(0)).int()
    out = R.gather_cache(cp, cg, src, n_prompt, K)
    assert out.shape == (R_, nkv, tp + tg, hd)
    for r in range(R_):
        assert torch.equal(out[r, :, :n_prompt], cp[r // K, :, :n_prompt])
        for s in range(tg):
            assert torch.equal(out[r, :, n_prompt + s], cg[src[r, s], :, s])
    assert (out[:, :, n_prompt + tg:] == 0).all()
