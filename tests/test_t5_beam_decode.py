"""Beam search on the T5 graph decoder (opt-in: beam_search="graph+t5"), on the host: the decoder's torch path at fp32 against HF ``generate``
(transformers' ``_beam_search`` over an encoder-decoder) token for token, on the tiny random T5 of tests/test_decode.py whose lm_head is
scaled x 4 so that the beams' log-probabilities spread and beams really re-order; and the opt-in envelopes as a table: under "graph+t5" the
T5 beam rows plan to the decoder and every Llama row decides as under "graph", under "graph" and "hf" the T5 beam rows stay on HF."""
import functools
import inspect
import types
import warnings

import pytest
import torch

import test_beam_decode as TB      # the "graph" table and the planners' stand-ins
import test_padded_decode as T

N_NEW, P, D = 20, 7, 64
SHIPPED_SF = dict(length_penalty=1, repetition_penalty=1.5, num_beams=5, min_length=1, max_length=250)      # LSTP_SF_blip2.yaml / LSTP_TG_blip2.yaml


@functools.lru_cache(maxsize=None)
def _t5():
    from test_decode import _t5 as tiny_t5
    lm = tiny_t5("cpu")
    with torch.no_grad():
        lm.lm_head.weight.mul_(4.0)
    return lm


@functools.lru_cache(maxsize=None)
def _decoder():
    from videotgb_amd.decode import T5GreedyDecoder
    return T5GreedyDecoder(_t5(), fused=False)


@functools.lru_cache(maxsize=None)
def _inputs(B):
    g = torch.Generator().manual_seed(5 + B)
    x = torch.randn(B, P, D, generator=g) * 0.5
    m = torch.ones(B, P, dtype=torch.long)
    if B > 1:
        m[1, -2:] = 0      # a padded encoder row
    return x, m


def _hf(B, **kw):
    x, m = _inputs(B)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return _t5().generate(inputs_embeds=x, attention_mask=m, do_sample=False, pad_token_id=0, **kw)


def _ours(B, n=N_NEW, **kw):
    x, m = _inputs(B)
    return _decoder().generate(x, n, attention_mask=m, pad_token_id=0, **kw)


@functools.lru_cache(maxsize=None)
def _eos_ids(B, K):
    """eos ids chosen from what the model emits: the first distinct tokens of the unconstrained search's output (one item alone repeats
    itself after a few tokens, and only an early token ends its search before the last step)."""
    free = _hf(B, num_beams=K, repetition_penalty=1.5, max_new_tokens=N_NEW, eos_token_id=None)
    seen = []
    for t in free[:, 1:].flatten().tolist():
        if t not in seen and t != 0:
            seen.append(t)
    return tuple(seen[:4])


@pytest.mark.parametrize("K", [2, 3, 5])
@pytest.mark.parametrize("B", [1, 3])
def test_ids_equal_hf_generate(B, K):
    ended, full = False, False
    for eos in (None,) + _eos_ids(B, K):
        kw = dict(num_beams=K, repetition_penalty=1.5, length_penalty=1.0, eos_token_id=eos)
        ref, out = _hf(B, max_new_tokens=N_NEW, **kw), _ours(B, **kw)
        assert torch.equal(out, ref), (B, K, eos, out.tolist(), ref.tolist())
        assert (ref[:, 0] == 0).all()      # the ids start with decoder_start_token_id
        if eos is None:
            full |= ref.shape[1] == 1 + N_NEW
        else:
            gen = ref[:, 1:]
            has = (gen == eos).any(-1)
            n = (gen == eos).int().argmax(-1)
            ended |= bool((has & (n < gen.shape[1] - 1)).any()) or gen.shape[1] < N_NEW
            full |= bool((~has).any())
            for b in range(B):      # pad_token_id = 0: a finished row is filled with EOS (HF: ``pad_token_id or eos_token_id``)
                if has[b]:
                    assert (gen[b, n[b]:] == eos).all() and (out[b, 1 + n[b]:] == eos).all()
    assert ended and full, "the eos ids must end at least one row early and leave at least one running to the end"


@pytest.mark.parametrize("repetition_penalty", [1.0, 1.5])
def test_the_repetition_penalty_sees_the_start_token(repetition_penalty):
    """HF's decoder input is the start token (id 0), so RepetitionPenaltyLogitsProcessor penalises id 0 from the first step on."""
    B, K = 3, 3
    kw = dict(num_beams=K, repetition_penalty=repetition_penalty, eos_token_id=None)
    ref = _hf(B, max_new_tokens=N_NEW, **kw)
    assert torch.equal(_ours(B, **kw), ref)
    if repetition_penalty != 1.0:      # the penalty matters for this model, so the case above is no accident
        assert not torch.equal(ref, _hf(B, max_new_tokens=N_NEW, **dict(kw, repetition_penalty=1.0)))


def test_the_start_tokens_penalty_decides_ids():
    """A decoder that left the start token out of the penalised ids (the Llama case: only generated ids) returns other ids than HF somewhere
    over these requests: penalising id 0 is visible, not a no-op."""
    from videotgb_amd.decode import _GraphDecoder
    dec = _decoder()
    differs = False
    for B, K in ((3, 3), (3, 5), (1, 5)):
        kw = dict(num_beams=K, repetition_penalty=1.5, eos_token_id=None)
        ref = _hf(B, max_new_tokens=N_NEW, **kw)
        dec._beam_candidates = types.MethodType(_GraphDecoder._beam_candidates, dec)      # the shared statement: generated ids only
        try:
            differs |= not torch.equal(_ours(B, **kw), ref)
        finally:
            del dec._beam_candidates
        assert torch.equal(_ours(B, **kw), ref)
    assert differs


def test_the_shipped_sf_generate_configs_through_graph_generate(monkeypatch):
    """The shipped dictionary with max_length / min_length, through ``graph_generate`` of an owner that says "graph+t5" (the planner only
    serves embeddings on the device: the stand-in says so, the decoder itself runs its torch path on the host)."""
    from videotgb_amd import decode
    B = 3
    x, m = _inputs(B)
    cfgs = dict(SHIPPED_SF, max_length=1 + N_NEW, min_length=4)
    ref = _hf(B, **cfgs)

    class OnDevice:      # what plan_decode reads of the embeddings
        is_cuda, shape = True, x.shape
    monkeypatch.setattr(decode, "make_decoder", lambda lm, **kw: _decoder())
    real = decode.plan_decode
    monkeypatch.setattr(decode, "plan_decode", lambda lm, emb, am, gc, env: real(lm, OnDevice, am, gc, env))
    owner = types.SimpleNamespace(beam_search="graph+t5")
    out = decode.graph_generate(owner, _t5(), x, m, cfgs)
    assert out is not None and torch.equal(out, ref), (out, ref)
    assert not (ref[:, 1:4] == 1).any()      # min_length 4 = three generated tokens without eos (id 1)
    assert decode.graph_generate(types.SimpleNamespace(beam_search="graph"), _t5(), x, m, cfgs) is None
    assert decode.graph_generate(types.SimpleNamespace(), _t5(), x, m, cfgs) is None
    assert decode.generated_length(_t5(), cfgs, P) == (N_NEW, 3)


@pytest.mark.parametrize("length_penalty", [0.0, 1.0, 2.0])
def test_length_penalty(length_penalty):
    B, K = 3, 3
    for eos in _eos_ids(B, K)[:2]:
        kw = dict(num_beams=K, repetition_penalty=1.5, length_penalty=length_penalty, eos_token_id=eos)
        assert torch.equal(_ours(B, **kw), _hf(B, max_new_tokens=N_NEW, **kw)), (length_penalty, eos)


def test_min_new_tokens_blocks_eos():
    B, K = 3, 3
    base = dict(num_beams=K, repetition_penalty=1.5)
    early = [e for e in _eos_ids(B, K) if (_hf(B, max_new_tokens=N_NEW, eos_token_id=e, **base)[:, 1:11] == e).any()]
    assert early, "an eos id that ends a row within 10 tokens"
    kw = dict(base, eos_token_id=early[0], min_new_tokens=10)
    ref, out = _hf(B, max_new_tokens=N_NEW, **kw), _ours(B, **kw)
    assert torch.equal(out, ref) and not (ref[:, 1:11] == early[0]).any()


def test_the_winning_beam_changes_parents():
    B, K = 3, 5
    _ours(B, num_beams=K, repetition_penalty=1.5, eos_token_id=None)
    st = next(reversed(_decoder().graphs.values()))
    bi = st["beam_bi"][:, 0]      # the best beam's parents, with the batch offset
    assert (bi >= 0).all() and torch.equal(bi // K, torch.arange(B)[:, None].expand(B, N_NEW).int())
    assert ((bi % K)[:, 1:] != 0).any(), "every winning beam descended from beam 0 at every step: nothing was re-ordered"


def test_what_the_decoder_refuses():
    from videotgb_amd import ops
    from videotgb_amd.decode import T5GreedyDecoder, check_mode
    x, _ = _inputs(1)
    dec = _decoder()
    for kw in (dict(do_sample=True), dict(stop_ids=[[5, 6]]), dict(text_stop=lambda ids: False)):
        with pytest.raises(NotImplementedError):
            dec.generate(x, 4, num_beams=2, **kw)
    with pytest.raises(NotImplementedError):
        dec.generate(x, 4, num_beams=1, repetition_penalty=1.5)
    with pytest.raises(NotImplementedError):
        dec.generate(x, 4, num_beams=ops.BEAM_MAX_BEAMS + 1)
    with pytest.raises(ValueError):
        dec.generate(x, 4, num_beams=0)
    with pytest.raises(ValueError):
        dec.generate(x, 4, num_beams=2, repetition_penalty=0.0)
    from transformers import T5Config, T5ForConditionalGeneration
    small = T5ForConditionalGeneration(T5Config(vocab_size=8, d_model=16, d_kv=4, d_ff=16, num_layers=1, num_heads=2, decoder_start_token_id=0)).eval()
    with pytest.raises(NotImplementedError):      # 2 K > V
        T5GreedyDecoder(small, fused=False).generate(torch.zeros(1, 3, 16), 4, num_beams=5)
    assert "NotImplementedError" in inspect.getsource(T5GreedyDecoder.generate)
    assert [check_mode("beam_search", v) for v in ("hf", "graph", "graph+t5")] == ["hf", "graph", "graph+t5"]
    for bad in ("on", "t5", "graph+T5", True, None):
        with pytest.raises(ValueError):
            check_mode("beam_search", bad)
    assert ops.ATTENTION_ROWS_BEAM_MAX_KEYS == 1920


# ------------------------------------------------------------------------------------------------------------------------ envelopes
BASE = T.BASE
SF = dict(BASE, num_beams=5, repetition_penalty=1.5, length_penalty=1.0)
BEAMS5 = dict(BASE, num_beams=5, repetition_penalty=1.0, length_penalty=1.0)
T5_ROWS = {"T5 beams", "shipped beam family, T5"}

# (case, model_type, mask, request, LSTP.generate's decision, eval_forward's decision) with beam_search="graph+t5": the T5 beam rows of the
# "graph" table with their new decisions, and more T5 rows
T5_OPT_IN = [
    ("T5 beams", "t5", "ones", dict(do_sample=False, num_beams=5, max_new_tokens=8), BEAMS5, dict(BEAMS5, max_new_tokens=8)),
    ("shipped beam family, T5", "t5", "ones", T.SHIPPED_BEAMS, "hf", dict(SF, max_new_tokens=249)),      # (LSTP.generate knows no max_length)
    ("shipped beam family, T5, min_length 3", "t5", "ones", dict(T.SHIPPED_BEAMS, min_length=3), "hf", dict(SF, max_new_tokens=249, min_new_tokens=2)),
    ("T5 beams, padded", "t5", "padded", dict(do_sample=False, num_beams=5, repetition_penalty=1.5, max_new_tokens=8),
     dict(SF, attention_mask=T.PADDED), dict(SF, attention_mask=T.PADDED, max_new_tokens=8)),
    ("T5 beams with sampling", "t5", "ones", dict(do_sample=True, temperature=0.2, num_beams=5, max_new_tokens=8), "hf", "hf"),
    ("T5 beams, repetition_penalty=0", "t5", "ones", dict(do_sample=False, num_beams=5, repetition_penalty=0, max_new_tokens=8), "hf", "hf"),
    ("T5 beams, early_stopping", "t5", "ones", dict(do_sample=False, num_beams=5, early_stopping=True, max_new_tokens=8), "hf", "hf"),
    ("T5 beams, num_return_sequences", "t5", "ones", dict(do_sample=False, num_beams=5, num_return_sequences=2, max_new_tokens=8), "hf", "hf"),
    ("T5 beams with keyword stopping", "t5", "ones1", dict(do_sample=False, num_beams=5, max_new_tokens=8, stopping_criteria=[T._keyword_criteria()]),
     "hf", "hf"),
    ("T5, one beam, repetition_penalty=1.5", "t5", "ones", dict(do_sample=False, repetition_penalty=1.5, max_new_tokens=8), "hf", "hf"),
    ("T5 beams, max_length 1", "t5", "ones", dict(T.SHIPPED_BEAMS, max_length=1), "hf", "hf"),
]


def _decisions(case, owner, monkeypatch):
    name, model_type, mask, request = case[:4]
    module = TB._module_decision(model_type, mask, request, owner, monkeypatch) if "stopping_criteria" not in request else None
    return TB._generate_decision(model_type, mask, request, owner), module


@pytest.mark.parametrize("case", T5_OPT_IN, ids=[c[0] for c in T5_OPT_IN])
def test_t5_beam_rows_under_graph_t5(case, monkeypatch):
    want_generate, want_module = case[4:]
    got_generate, got_module = _decisions(case, types.SimpleNamespace(beam_search="graph+t5"), monkeypatch)
    assert got_generate == want_generate, case[0]
    assert got_module is None or got_module == want_module, case[0]
    for owner in (types.SimpleNamespace(beam_search="graph"), types.SimpleNamespace(beam_search="hf"), types.SimpleNamespace()):
        if case[3].get("num_beams", 1) > 1:      # without the new value every T5 beam row still plans to HF
            assert _decisions(case, owner, monkeypatch) in (("hf", "hf"), ("hf", None)), (case[0], owner)


OTHER_ROWS = [c for c in TB.OPT_IN if c[0] not in T5_ROWS]
assert len(OTHER_ROWS) == len(TB.OPT_IN) - 2


@pytest.mark.parametrize("case", OTHER_ROWS, ids=[c[0] for c in OTHER_ROWS])
def test_every_other_row_decides_as_under_graph(case, monkeypatch):
    """The "graph" table under "graph+t5": every row but the two T5 beam rows (re-decided above) keeps its decision."""
    want_generate, want_module = case[4:]
    got_generate, got_module = _decisions(case, types.SimpleNamespace(beam_search="graph+t5"), monkeypatch)
    assert got_generate == want_generate and (got_module is None or got_module == want_module), case[0]


PLAIN_ROWS = [c for c in T.ENVELOPE if c[3].get("num_beams", 1) == 1 and "max_length" not in c[3]]      # (the others: the opt-in tables)


@pytest.mark.parametrize("case", PLAIN_ROWS, ids=[c[0] for c in PLAIN_ROWS])
def test_rows_without_beams_decide_as_today(case, monkeypatch):
    name, model_type, mask, request, want_generate, want_module = case
    got_generate, got_module = _decisions(case, types.SimpleNamespace(beam_search="graph+t5"), monkeypatch)
    assert got_generate == want_generate and (got_module is None or got_module == want_module), name


def test_envelope_values():
    from videotgb_amd import decode as D
    assert D.Envelope._fields[-2:] == ("beams", "t5_beams") and D.Envelope._field_defaults["t5_beams"] is False
    for env in (D.GENERATE_ENVELOPE, D.MODULE_ENVELOPE, D.GENERATE_ENVELOPE_BEAMS, D.MODULE_ENVELOPE_BEAMS):
        assert env.t5_beams is False
    assert D.GENERATE_ENVELOPE_T5_BEAMS == D.GENERATE_ENVELOPE_BEAMS._replace(t5_beams=True)
    assert D.MODULE_ENVELOPE_T5_BEAMS == D.MODULE_ENVELOPE_BEAMS._replace(t5_beams=True)
    t5, graph = types.SimpleNamespace(beam_search="graph+t5"), types.SimpleNamespace(beam_search="graph")
    assert D.envelope_for(t5, module=True) is D.MODULE_ENVELOPE_T5_BEAMS and D.envelope_for(t5, module=False) is D.GENERATE_ENVELOPE_T5_BEAMS
    assert D.envelope_for(graph, module=True) is D.MODULE_ENVELOPE_BEAMS and D.envelope_for(graph, module=False) is D.GENERATE_ENVELOPE_BEAMS
    assert D.envelope_for(types.SimpleNamespace(), module=True) is D.MODULE_ENVELOPE


def test_the_owners_accept_the_value():
    from videotgb_amd import builder_utils, models, modules
    for fn in (models._LSTPBase.__init__, builder_utils.load_pretrained_model, modules._LSTPLightningBase.__init__):
        assert "graph+t5" in inspect.getdoc(fn) or "graph+t5" in inspect.getsource(fn), fn
