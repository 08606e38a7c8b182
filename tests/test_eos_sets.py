"""Eos-id SETS on the graph decoders (opt-in: ``eos_sets=True``), on the host: the decoders' torch path at fp32 against HF ``generate`` token
for token, on the tiny Llama of tests/test_llama_variants.py and the tiny T5 of tests/test_t5_beam_decode.py.

Every case takes its set from HF's own eos-free output of the fixture -- an id that ends row 0 early, another id that ends another row at a
different step, an id that never occurs -- and first shows ON HF ALONE that at least two different ids of the set each end a row and that the
request with only the set's first id gives other ids: a decoder that honoured only the first id could not pass."""
import functools
import warnings

import pytest
import torch

import test_llama_variants as LV
import test_t5_beam_decode as TT

N_LLAMA, N_T5 = LV.N_NEW, TT.N_NEW
BEAMS = dict(num_beams=3, repetition_penalty=1.5, length_penalty=1.0)


def _key(kw):
    return tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in kw.items()))


@functools.lru_cache(maxsize=None)
def _hf_cached(model, padded, B, key):
    kw = {k: (list(v) if isinstance(v, tuple) else v) for k, v in key}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if model == "llama":
            x, m = LV._inputs(padded)
            return LV._llama().generate(inputs_embeds=x[:B], attention_mask=m[:B], do_sample=False, max_new_tokens=N_LLAMA, **kw)
        x, m = TT._inputs(B)
        return TT._t5().generate(inputs_embeds=x, attention_mask=m, do_sample=False, max_new_tokens=N_T5, **kw)[:, 1:]      # (without the start token)


def _hf(model, padded=False, B=3, **kw):
    """HF generate's GENERATED ids [B, n] for the fixture (computed once per request, shared, never written)."""
    return _hf_cached(model, padded, B, _key(kw))


@functools.lru_cache(maxsize=None)
def _decoder(model):
    from videotgb_amd.decode import GreedyDecoder, T5GreedyDecoder
    return GreedyDecoder(LV._llama(), fused=False, eos_sets=True) if model == "llama" else T5GreedyDecoder(TT._t5(), fused=False, eos_sets=True)


def _ours(model, padded=False, B=3, **kw):
    if model == "llama":
        x, m = LV._inputs(padded)
        return _decoder(model).generate(x[:B], N_LLAMA, attention_mask=m[:B], **kw)
    x, m = TT._inputs(B)
    return _decoder(model).generate(x, N_T5, attention_mask=m, **kw)[:, 1:]


def _enders(out, ids, pad):
    """Per row of HF's output the id of ``ids`` that ended it before the last column, or None (what follows it is ``pad``)."""
    res = []
    for row in out.tolist():
        hit = [j for j, t in enumerate(row) if t in ids]
        j = hit[0] if hit else None
        res.append(row[j] if j is not None and j < len(row) - 1 and all(t == pad for t in row[j + 1:]) else None)
    return res


@functools.lru_cache(maxsize=None)
def _eos_set(model, padded=False, beams=False, min_new=0):
    """(e0, e1, u) from HF's eos-free output: e0 ends row 0 early, e1 ends another row at another step, u never occurs; shown on HF alone --
    two different ids each end a row, and the request with only e0 gives other ids.  ``min_new``: ids generated from that step on."""
    kw = dict(BEAMS) if beams else {}
    free = _hf(model, padded, eos_token_id=None, pad_token_id=0, **kw)
    n = free.shape[1]
    V = (LV._llama() if model == "llama" else TT._t5()).config.vocab_size
    u = next(v for v in range(V - 1, 0, -1) if v not in free.flatten().tolist())
    for j0 in range(max(min_new, 1), n - 1):
        for r in range(1, free.shape[0]):
            for j1 in range(max(min_new, 1), n - 1):
                e0, e1 = int(free[0, j0]), int(free[r, j1])
                if j1 == j0 or e0 == e1 or 0 in (e0, e1):
                    continue
                ids = (e0, e1, u)
                ref = _hf(model, padded, eos_token_id=list(ids), pad_token_id=0, **kw)
                ends = _enders(ref, ids, e0 if beams else 0)      # (beams: pad 0 fills with the first id)
                only = _hf(model, padded, eos_token_id=e0, pad_token_id=0, **kw)
                if ends[0] is not None and len({e for e in ends if e is not None}) >= 2 and u not in ref.flatten().tolist() and ref.tolist() != only.tolist():
                    return ids
    raise AssertionError("no eos set with two ending ids in HF's output of this fixture")


def _check(model, ids, padded=False, B=3, **kw):
    ref, out = _hf(model, padded, B, eos_token_id=list(ids), **kw), _ours(model, padded, B, eos_token_id=list(ids), **kw)
    assert torch.equal(out, ref), (model, ids, kw, out.tolist(), ref.tolist())
    return ref


@pytest.mark.parametrize("model", ["llama", "t5"])
def test_greedy_ids_equal_hf_generate(model):
    ids = _eos_set(model)
    ref = _check(model, ids, pad_token_id=0)
    assert len({e for e in _enders(ref, ids, 0) if e is not None}) >= 2      # two different ids of the set each end a row
    assert ref.tolist() != _hf(model, eos_token_id=ids[0], pad_token_id=0).tolist()
    assert torch.equal(_ours(model, eos_token_id=list(ids[::-1]), pad_token_id=0), ref)      # (with an explicit pad the order does not matter)


@pytest.mark.parametrize("model", ["llama", "t5"])
def test_greedy_padded_batch(model):
    padded = model == "llama"      # (the T5 fixture's batch of 3 has a padded encoder row as it is)
    ids = _eos_set(model, padded)
    ref = _check(model, ids, padded, pad_token_id=0)
    assert len({e for e in _enders(ref, ids, 0) if e is not None}) >= 2


@pytest.mark.parametrize("model", ["llama", "t5"])
def test_min_new_tokens_blocks_every_id(model):
    """The set's ids end rows at steps j0 != j1; min_new_tokens past both blocks both (HF alone: other ids than with min_new_tokens = 0)."""
    ids = _eos_set(model)
    plain = _hf(model, eos_token_id=list(ids), pad_token_id=0)
    first = [min(j for j, t in enumerate(row) if t in ids) for row in plain.tolist() if any(t in ids for t in row)]
    m = max(first) + 1      # one past the latest first hit: every hit of the plain request is blocked
    ref = _check(model, ids, pad_token_id=0, min_new_tokens=m)
    assert ref.tolist() != plain.tolist()
    assert not any(t in ids for row in ref[:, :m].tolist() for t in row)
    m2 = min(first) + 1     # between the two: the earlier id is blocked, the later one still ends its row
    if m2 != m:
        ref2 = _check(model, ids, pad_token_id=0, min_new_tokens=m2)
        assert ref2.tolist() not in (plain.tolist(), ref.tolist())


@pytest.mark.parametrize("model", ["llama", "t5"])
def test_pad_default_is_the_first_id(model):
    """No pad_token_id: HF pads finished rows with eos[0]."""
    ids = _eos_set(model)
    lm = LV._llama() if model == "llama" else TT._t5()
    keep = lm.generation_config.pad_token_id
    lm.generation_config.pad_token_id = None      # (the fixtures' generation configs name pad 0; the case is the request without any)
    try:
        ref = _hf(model, eos_token_id=list(ids))
    finally:
        lm.generation_config.pad_token_id = keep
    out = _ours(model, eos_token_id=list(ids), pad_token_id=None)
    assert torch.equal(out, ref), (out.tolist(), ref.tolist())
    assert ids[0] != 0 and (ref[0, -1] == ids[0]) and ref.tolist() != _hf(model, eos_token_id=list(ids), pad_token_id=0).tolist()


def test_keyword_stop_plus_the_set():
    """B = 1 (row 0 of the Llama fixture): a keyword and the set -- whichever comes first ends the row, against HF with the same criteria."""
    from test_decode import _Tok
    from videotgb_amd.builder_utils import KeywordsStoppingCriteria
    from videotgb_amd.decode import keyword_stop_plan
    free = _hf("llama", eos_token_id=None, pad_token_id=0)[0].tolist()
    end = 5
    ids = (_eos_set("llama")[2], free[end])      # the id that never occurs first: the row ends on the set's SECOND id
    assert free.index(free[end]) == end and free[end - 2] != free[end - 1]
    x, m = LV._inputs(False)
    prompt = torch.zeros(1, 3, dtype=torch.long)
    lens = []
    for kw in (f"t{free[end - 2]} t{free[end - 1]}", "t4711 t4712"):      # a keyword met before the set's id; one never met (the set ends the row)
        crit = KeywordsStoppingCriteria([kw], _Tok(), prompt)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref = LV._llama().generate(inputs_embeds=x[:1], attention_mask=m[:1], do_sample=False, max_new_tokens=N_LLAMA, stopping_criteria=[crit],
                                       eos_token_id=list(ids), pad_token_id=0)
        out = _decoder("llama").generate(x[:1], N_LLAMA, attention_mask=m[:1], eos_token_id=list(ids), pad_token_id=0, **keyword_stop_plan([crit]))
        assert torch.equal(out, ref), (kw, out.tolist(), ref.tolist())
        lens.append(ref.shape[1])
    assert lens == [end, end + 1]


@pytest.mark.parametrize("min_new", [0, 4])
@pytest.mark.parametrize("model", ["llama", "t5"])
def test_beam_ids_equal_hf_generate(model, min_new):
    ids = _eos_set(model, beams=True, min_new=min_new)
    kw = dict(BEAMS, pad_token_id=0, **(dict(min_new_tokens=min_new) if min_new else {}))
    ref = _check(model, ids, **kw)
    assert len({e for e in _enders(ref, ids, ids[0]) if e is not None}) >= 2
    assert ref.tolist() != _hf(model, eos_token_id=ids[0], **kw).tolist()
    if min_new:      # a set whose ids come earlier: HF alone shows that the block changes the output, and no blocked id is generated
        early = _eos_set(model, beams=True)
        plain = _hf(model, eos_token_id=list(early), **dict(BEAMS, pad_token_id=0))
        blocked = _check(model, early, **kw)
        assert blocked.tolist() != plain.tolist()
        assert not any(t in early for row in blocked[:, :min_new].tolist() for t in row)


@pytest.mark.parametrize("model", ["llama", "t5"])
def test_what_stays_refused_and_what_collapses(model):
    from videotgb_amd import ops
    from videotgb_amd.decode import GreedyDecoder, T5GreedyDecoder
    ids = _eos_set(model)
    lm = LV._llama() if model == "llama" else TT._t5()
    V = lm.config.vocab_size
    plain = (GreedyDecoder if model == "llama" else T5GreedyDecoder)(lm, fused=False)
    assert plain.eos_sets is False and _decoder(model).eos_sets is True
    x = (LV._inputs(False)[0] if model == "llama" else TT._inputs(3)[0])
    with pytest.raises(NotImplementedError, match="one eos_token_id"):      # without the opt-in: today's refusal
        plain.generate(x, 4, eos_token_id=list(ids))
    with pytest.raises(NotImplementedError):
        _decoder(model).generate(x, 4, eos_token_id=list(range(1, ops.EOS_MAX + 2)))      # 9 ids
    with pytest.raises(NotImplementedError):
        _decoder(model).generate(x, 4, eos_token_id=[ids[0], V])      # an id >= V
    with pytest.raises(NotImplementedError):
        _decoder(model).generate(x, 4, eos_token_id=[ids[0], -1])
    assert ops.EOS_MAX == 8
    _decoder(model).generate(x, 4, eos_token_id=list(range(1, ops.EOS_MAX + 1)))      # 8 ids are served
    # [e, e] is the request e: the same ids, through a state without a device list
    e = ids[0]
    assert torch.equal(_ours(model, eos_token_id=[e, e], pad_token_id=0), _hf(model, eos_token_id=e, pad_token_id=0))
    st = next(reversed(_decoder(model).graphs.values()))
    assert st["eos"] == e and "eos_t" not in st
    _ours(model, eos_token_id=[ids[1], ids[0], ids[1]], pad_token_id=0)
    st = next(reversed(_decoder(model).graphs.values()))
    assert st["eos"] == (ids[1], ids[0]) and st["eos_t"].tolist() == [ids[1], ids[0]] and st["eos_t"].dtype == torch.int32      # the caller's order, duplicates dropped
    assert torch.equal(_ours(model, eos_token_id=None, pad_token_id=0), _hf(model, eos_token_id=None, pad_token_id=0))
    assert "eos_t" not in next(reversed(_decoder(model).graphs.values()))
