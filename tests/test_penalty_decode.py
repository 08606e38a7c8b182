"""A repetition penalty on ONE beam on the graph decoders (opt-in: ``penalty=True``), on the host: the decoders' torch path at fp32 against HF
``generate`` token for token, on the tiny Llama of tests/test_beam_decode.py (lm_head x 40) and the tiny T5 of tests/test_t5_beam_decode.py.

Every case first shows ON HF ALONE that the penalty decides ids: the penalised output differs from the unpenalised one in every row, so a
decoder that ignored the penalty could not pass.  The batch of 3 has a padded row in both fixtures."""
import functools
import types

import pytest
import torch

import test_beam_decode as TB
import test_t5_beam_decode as TT

MODELS = ("llama", "t5")
N_NEW = dict(llama=TB.N_NEW, t5=TT.N_NEW)


@functools.lru_cache(maxsize=None)
def _hf_cached(model, B, key):
    kw = dict(key)
    if model == "llama":
        return TB._hf(B, max_new_tokens=N_NEW[model], **kw)
    return TT._hf(B, max_new_tokens=N_NEW[model], **kw)[:, 1:]      # (without the start token)


def _hf(model, B, **kw):
    """HF generate's GENERATED ids [B, n] (greedy, pad 0; computed once per request, shared, never written)."""
    return _hf_cached(model, B, tuple(sorted(kw.items())))


@functools.lru_cache(maxsize=None)
def _decoder(model):
    from videotgb_amd.decode import GreedyDecoder, T5GreedyDecoder
    return GreedyDecoder(TB._llama(), fused=False, penalty=True) if model == "llama" else T5GreedyDecoder(TT._t5(), fused=False, penalty=True)


def _ours(model, B, dec=None, **kw):
    x, m = (TB if model == "llama" else TT)._inputs(B)
    out = (dec or _decoder(model)).generate(x, N_NEW[model], attention_mask=m, pad_token_id=0, **kw)
    return out if model == "llama" else out[:, 1:]


def _rows_differ(model, B, p, **kw):
    ref, plain = _hf(model, B, repetition_penalty=p, **kw), _hf(model, B, **kw)
    n = min(ref.shape[1], plain.shape[1])
    return all((ref[b, :n] != plain[b, :n]).any() for b in range(B))


def _penalty_decides(model, B, p, **kw):
    """The condition, on HF alone: every row's penalised ids differ from its unpenalised ones."""
    ref = _hf(model, B, repetition_penalty=p, **kw)
    assert _rows_differ(model, B, p, **kw), (model, B, p, kw, ref.tolist(), _hf(model, B, **kw).tolist())
    return ref


@functools.lru_cache(maxsize=None)
def _eos(model, p, min_step=1):
    """(eos id, row, step) from HF's own penalised eos-free output of the batch of 3: with it as eos, HF ends that row early (at ``step`` >=
    ``min_step``, the rest pad) and leaves another row running to the last column -- late enough that the penalty has decided ids of every
    row before (the condition above holds for the request with this eos too)."""
    B, n = 3, N_NEW[model]
    free = _hf(model, B, repetition_penalty=p, eos_token_id=None)
    for j in range(min_step, n - 1):
        for r in range(B):
            e = int(free[r, j])
            if e == 0:
                continue
            ref = _hf(model, B, repetition_penalty=p, eos_token_id=e)
            row = ref[r].tolist()
            early = e in row and row.index(e) == j and all(t == 0 for t in row[j + 1:])
            full = any(e not in ref[b].tolist() for b in range(B)) and ref.shape[1] == n
            if early and full and _rows_differ(model, B, p, eos_token_id=e):
                return e, r, j
    raise AssertionError("no eos id that ends one row early and leaves one running in HF's penalised output of this fixture")


@pytest.mark.parametrize("p", [1.5, 0.7])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("model", MODELS)
def test_greedy_ids_equal_hf_generate(model, B, p):
    ref = _penalty_decides(model, B, p, eos_token_id=None)
    out = _ours(model, B, repetition_penalty=p, eos_token_id=None)
    assert torch.equal(out, ref), (model, B, p, out.tolist(), ref.tolist())
    assert ref.shape == (B, N_NEW[model])


@pytest.mark.parametrize("p", [1.5, 0.7])
@pytest.mark.parametrize("model", MODELS)
def test_one_row_ends_early_and_one_runs_to_the_end(model, p):
    e, r, j = _eos(model, p)
    ref = _penalty_decides(model, 3, p, eos_token_id=e)
    out = _ours(model, 3, repetition_penalty=p, eos_token_id=e)
    assert torch.equal(out, ref), (model, p, e, out.tolist(), ref.tolist())
    assert ref[r, j] == e and (ref[r, j + 1:] == 0).all() and any(e not in row for row in ref.tolist())


@pytest.mark.parametrize("model", MODELS)
def test_min_new_tokens_blocks_eos_behind_the_penalty(model):
    """HF's order: the penalty, then the eos block.  The eos id ends its row at step j >= 2; min_new_tokens = j + 1 blocks it there."""
    p = 1.5
    e, r, j = _eos(model, p, min_step=2)
    plain = _hf(model, 3, repetition_penalty=p, eos_token_id=e)
    ref = _penalty_decides(model, 3, p, eos_token_id=e, min_new_tokens=j + 1)
    assert ref.tolist() != plain.tolist() and not (ref[:, :j + 1] == e).any()
    out = _ours(model, 3, repetition_penalty=p, eos_token_id=e, min_new_tokens=j + 1)
    assert torch.equal(out, ref), (model, e, j, out.tolist(), ref.tolist())


@pytest.mark.parametrize("p", [1.5, 0.7])
@pytest.mark.parametrize("B", [1, 3])
def test_cold_sampling_equals_hf_greedy_with_the_penalty(B, p):
    """Llama: sampling at temperature 1e-6 with top_p = 0.9 degenerates to the greedy token of the PENALISED scores (penalty before the warpers)."""
    ref = _penalty_decides("llama", B, p, eos_token_id=None)
    noise = torch.rand(N_NEW["llama"], B, generator=torch.Generator().manual_seed(11))
    out = _ours("llama", B, repetition_penalty=p, eos_token_id=None, do_sample=True, temperature=1e-6, top_p=0.9, sample_noise=noise)
    assert torch.equal(out, ref), (B, p, out.tolist(), ref.tolist())


def test_t5_the_start_token_is_seen():
    """A statement without ``start_id`` -- the Llama case, generated ids only -- differs from HF somewhere over these requests: the start
    token is id 0, which this model only comes to emit once a stronger penalty (2.0) has pushed the ids it repeats below it."""
    dec = _decoder("t5")
    differs = False
    for B, p in ((1, 1.5), (3, 1.5), (3, 0.7), (3, 2.0)):
        ref = _hf("t5", B, repetition_penalty=p, eos_token_id=None)
        dec._penalty_start = types.MethodType(lambda self: None, dec)
        try:
            differs |= not torch.equal(_ours("t5", B, repetition_penalty=p, eos_token_id=None), ref)
        finally:
            del dec._penalty_start
        assert torch.equal(_ours("t5", B, repetition_penalty=p, eos_token_id=None), ref)
    assert differs
    assert dec._penalty_start() == TT._t5().config.decoder_start_token_id == 0 and _decoder("llama")._penalty_start() is None


@pytest.mark.parametrize("model", MODELS)
def test_a_default_decoder_still_raises(model):
    from videotgb_amd.decode import GreedyDecoder, T5GreedyDecoder
    plain = (TB if model == "llama" else TT)._decoder()
    x, _ = (TB if model == "llama" else TT)._inputs(1)
    assert plain.penalty is False and _decoder(model).penalty is True
    with pytest.raises(NotImplementedError, match="repetition_penalty with one beam: use HF generate"):
        plain.generate(x, 4, num_beams=1, repetition_penalty=1.5)
    for dec in (plain, _decoder(model)):
        for bad in (0.0, -1.5):
            with pytest.raises(ValueError):
                dec.generate(x, 4, repetition_penalty=bad)
    assert (GreedyDecoder if model == "llama" else T5GreedyDecoder).PENALTY_KERNEL is True


@pytest.mark.parametrize("model", MODELS)
def test_the_penalty_is_part_of_the_state_and_of_its_key(model):
    dec, ref_dec = _decoder(model), (TB if model == "llama" else TT)._decoder()
    _ours(model, 3, repetition_penalty=1.5, eos_token_id=None)
    k15, st15 = next(reversed(dec.graphs.items()))
    assert st15["pen"] == 1.5 and st15["pen_t"].tolist() == [1.5] and ("penalty", 1.5) in k15 and "pen_out" not in st15
    _ours(model, 3, repetition_penalty=0.7, eos_token_id=None)
    k07, st07 = next(reversed(dec.graphs.items()))
    assert st07 is not st15 and st07["pen"] == 0.7 and k07 != k15
    _ours(model, 3, repetition_penalty=1.5, eos_token_id=None)
    assert next(reversed(dec.graphs.values())) is st15      # the cached state is reused
    # p == 1: the state, its key and its ids are those of a decoder without the opt-in
    out = _ours(model, 3, repetition_penalty=1.0, eos_token_id=None)
    k1, st1 = next(reversed(dec.graphs.items()))
    assert "pen" not in st1 and "pen_t" not in st1 and not any(isinstance(v, tuple) and v and v[0] == "penalty" for v in k1)
    assert torch.equal(out, _ours(model, 3, dec=ref_dec, eos_token_id=None)) and k1 == next(reversed(ref_dec.graphs))
    assert torch.equal(out, _hf(model, 3, eos_token_id=None))
