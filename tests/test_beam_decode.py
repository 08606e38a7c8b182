"""Beam search on the Llama graph decoder (opt-in: beam_search="graph"), on the host: the decoder's torch path at fp32 against HF ``generate``
(transformers' ``_beam_search``) token for token, on a tiny random Llama whose lm_head is scaled x 40 (unscaled, random-init logits are
nearly flat and every beam ties); and the opt-in envelopes as a table, next to the proof that an owner without ``beam_search`` plans as before."""
import functools
import inspect
import types
import warnings

import pytest
import torch

import test_padded_decode as T      # the existing envelope table and its planners' stand-ins

N_NEW, P = 24, 9
SHIPPED_SF = dict(length_penalty=1, repetition_penalty=1.5, num_beams=5, min_length=1, max_length=250, top_p=0.9, temperature=0.8)


@functools.lru_cache(maxsize=None)
def _llama():
    from videotgb_amd import llm
    lm = llm.build_llama("tiny", dtype=torch.float32, device="cpu", seed=3, num_hidden_layers=3, num_key_value_heads=1).eval()
    with torch.no_grad():
        lm.lm_head.weight.mul_(40.0)
    return lm


@functools.lru_cache(maxsize=None)
def _decoder():
    from videotgb_amd.decode import GreedyDecoder
    return GreedyDecoder(_llama(), fused=False)


@functools.lru_cache(maxsize=None)
def _inputs(B):
    g = torch.Generator().manual_seed(3 + B)
    x = torch.randn(B, P, 32, generator=g)
    m = torch.ones(B, P, dtype=torch.long)
    if B > 1:
        m[1, :3] = 0      # a padded row (leading pads)
    return x, m


def _hf(B, **kw):
    x, m = _inputs(B)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return _llama().generate(inputs_embeds=x, attention_mask=m, do_sample=False, pad_token_id=0, **kw)


def _ours(B, n=N_NEW, **kw):
    x, m = _inputs(B)
    return _decoder().generate(x, n, attention_mask=m, pad_token_id=0, **kw)


@functools.lru_cache(maxsize=None)
def _eos_ids(B, K):
    """eos ids chosen from what the model emits: tokens of the unconstrained search's output from the third position on."""
    free = _hf(B, num_beams=K, repetition_penalty=1.5, max_new_tokens=N_NEW, eos_token_id=None)
    seen = []
    for t in free[:, 2:].flatten().tolist():
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
        if eos is None:
            full |= ref.shape[1] == N_NEW
        else:
            n = (ref == eos).int().argmax(-1)
            has = (ref == eos).any(-1)
            ended |= bool((has & (n < ref.shape[1] - 1)).any()) or ref.shape[1] < N_NEW
            full |= bool((~has).any())
            for b in range(B):      # pad_token_id = 0: a finished row is filled with EOS (HF: ``pad_token_id or eos_token_id``)
                if has[b]:
                    assert (ref[b, n[b]:] == eos).all() and (out[b, n[b]:] == eos).all()
    assert ended and full, "the eos ids must end at least one row early and leave at least one running to the end"


def test_the_shipped_sf_generate_configs():
    B = 3
    ref = _hf(B, **dict(SHIPPED_SF, max_length=P + N_NEW))      # over embeddings HF generates max_length - P tokens, min_length - P < 0: no block
    out = _ours(B, num_beams=5, repetition_penalty=1.5, length_penalty=1, eos_token_id=2, min_new_tokens=max(1 - P, 0))
    assert ref.shape[1] <= N_NEW and torch.equal(out, ref)
    from videotgb_amd.decode import generated_length
    assert generated_length(_llama(), dict(SHIPPED_SF, max_length=P + N_NEW), P) == (N_NEW, 0)
    assert generated_length(_llama(), dict(SHIPPED_SF, max_new_tokens=7), P) == (7, 0) and generated_length(_llama(), dict(num_beams=5), P) is None
    t5 = types.SimpleNamespace(config=types.SimpleNamespace(model_type="t5"))
    assert generated_length(t5, dict(max_length=250, min_length=3), P) == (249, 2)


@pytest.mark.parametrize("length_penalty", [0.0, 1.0, 2.0])
def test_length_penalty(length_penalty):
    B, K = 3, 3
    for eos in _eos_ids(B, K)[:2]:
        kw = dict(num_beams=K, repetition_penalty=1.5, length_penalty=length_penalty, eos_token_id=eos)
        assert torch.equal(_ours(B, **kw), _hf(B, max_new_tokens=N_NEW, **kw)), (length_penalty, eos)


def test_min_new_tokens_blocks_eos():
    B, K = 3, 3
    base = dict(num_beams=K, repetition_penalty=1.5)
    early = [e for e in _eos_ids(B, K) if (_hf(B, max_new_tokens=N_NEW, eos_token_id=e, **base)[:, :12] == e).any()]
    assert early, "an eos id that ends a row within 12 tokens"
    kw = dict(base, eos_token_id=early[0], min_new_tokens=12)
    ref, out = _hf(B, max_new_tokens=N_NEW, **kw), _ours(B, **kw)
    assert torch.equal(out, ref) and not (ref[:, :12] == early[0]).any()


def test_the_winning_beam_changes_parents():
    B, K = 3, 5
    _ours(B, num_beams=K, repetition_penalty=1.5, eos_token_id=None)
    st = next(reversed(_decoder().graphs.values()))
    bi = st["beam_bi"][:, 0]      # the best beam's parents, with the batch offset
    assert (bi >= 0).all() and torch.equal(bi // K, torch.arange(B)[:, None].expand(B, N_NEW).int())
    assert ((bi % K)[:, 1:] != 0).any(), "every winning beam descended from beam 0 at every step: nothing was re-ordered"


def test_what_the_decoders_refuse():
    from videotgb_amd.decode import GreedyDecoder, T5GreedyDecoder, check_mode
    x, m = _inputs(1)
    dec = _decoder()
    with pytest.raises(NotImplementedError):
        dec.generate(x, 4, num_beams=2, do_sample=True)
    with pytest.raises(NotImplementedError):
        dec.generate(x, 4, num_beams=2, stop_ids=[[5, 6]])
    with pytest.raises(NotImplementedError):
        dec.generate(x, 4, num_beams=2, text_stop=lambda ids: False)
    with pytest.raises(NotImplementedError):
        dec.generate(x, 4, num_beams=1, repetition_penalty=1.5)
    with pytest.raises(ValueError):
        dec.generate(x, 4, num_beams=0)
    with pytest.raises(NotImplementedError):
        GreedyDecoder(_llama(), fused=False, kv_cache="fp8").generate(x, 4, num_beams=2)
    assert "num_beams" in inspect.signature(T5GreedyDecoder.generate).parameters
    src = inspect.getsource(T5GreedyDecoder.generate)
    assert "NotImplementedError" in src
    assert check_mode("beam_search", "hf") == "hf" and check_mode("beam_search", "graph") == "graph"
    with pytest.raises(ValueError):
        check_mode("beam_search", "on")


def test_the_option_is_accepted_everywhere_and_defaults_to_hf():
    from videotgb_amd import builder_utils, models, modules
    for fn in (models._LSTPBase.__init__, models._LSTPBase.from_cfg.__func__, builder_utils.load_pretrained_model, modules._LSTPLightningBase.__init__):
        assert inspect.signature(fn).parameters["beam_search"].default == "hf", fn
    assert len(set(modules.TARGETS.values())) == 8 and all(issubclass(c, modules._LSTPLightningBase) for c in modules.TARGETS.values())
    params = list(inspect.signature(models._LSTPBase._graph_plan).parameters)
    assert params[:7] == ["lm", "inputs_embeds", "attention_mask", "do_sample", "temperature", "stopping_criteria", "kw"] and params[7:] == ["env"]


# ------------------------------------------------------------------------------------------------------------------------ envelopes
BASE, PADDED = T.BASE, T.PADDED
BEAMS5 = dict(BASE, num_beams=5, repetition_penalty=1.0, length_penalty=1.0)
SF = dict(BASE, num_beams=5, repetition_penalty=1.5, length_penalty=1.0)

# (case, model_type, mask, request, LSTP.generate's decision, eval_forward's decision) with beam_search="graph"
OPT_IN = [
    ("num_beams=5", "llama", "ones", dict(do_sample=False, num_beams=5, max_new_tokens=8), BEAMS5, dict(BEAMS5, max_new_tokens=8)),
    ("num_beams=5, penalties", "llama", "ones", dict(do_sample=False, num_beams=5, repetition_penalty=1.5, length_penalty=2, max_new_tokens=8),
     dict(BASE, num_beams=5, repetition_penalty=1.5, length_penalty=2.0), dict(BASE, num_beams=5, repetition_penalty=1.5, length_penalty=2.0, max_new_tokens=8)),
    ("num_beams=5, padded", "llama", "padded", dict(do_sample=False, num_beams=5, max_new_tokens=8), dict(BEAMS5, attention_mask=PADDED),
     dict(BEAMS5, attention_mask=PADDED, max_new_tokens=8)),
    ("shipped beam family: max_length 250 over 5 prompt positions", "llama", "ones", T.SHIPPED_BEAMS, "hf", dict(SF, max_new_tokens=245)),
    ("shipped beam family, min_length past the prompt", "llama", "ones", dict(T.SHIPPED_BEAMS, min_length=9), "hf",
     dict(SF, max_new_tokens=245, min_new_tokens=4)),
    ("max_new_tokens wins over max_length, min_new_tokens over min_length", "llama", "ones",
     dict(T.SHIPPED_BEAMS, max_new_tokens=8, min_length=9, min_new_tokens=2), "hf", dict(SF, max_new_tokens=8, min_new_tokens=2)),
    ("max_length inside the prompt", "llama", "ones", dict(T.SHIPPED_BEAMS, max_length=5), "hf", "hf"),
    ("one beam, max_length", "llama", "ones", dict(do_sample=False, max_length=13), "hf", dict(BASE, max_new_tokens=8)),
    ("one beam, max_length, T5", "t5", "ones", dict(do_sample=False, max_length=9, min_length=3), "hf", dict(BASE, max_new_tokens=8, min_new_tokens=2)),
    ("one beam, repetition_penalty=1.5", "llama", "ones", dict(do_sample=False, repetition_penalty=1.5, max_new_tokens=8), "hf", "hf"),
    ("beams with sampling", "llama", "ones", dict(do_sample=True, temperature=0.2, num_beams=5, max_new_tokens=8), "hf", "hf"),
    ("beams, repetition_penalty=0", "llama", "ones", dict(do_sample=False, num_beams=5, repetition_penalty=0, max_new_tokens=8), "hf", "hf"),
    ("beams, early_stopping", "llama", "ones", dict(do_sample=False, num_beams=5, early_stopping=True, max_new_tokens=8), "hf", "hf"),
    ("beams, num_return_sequences", "llama", "ones", dict(do_sample=False, num_beams=5, num_return_sequences=2, max_new_tokens=8), "hf", "hf"),
    ("beams with keyword stopping", "llama", "ones1", dict(do_sample=False, num_beams=5, max_new_tokens=8, stopping_criteria=[T._keyword_criteria()]),
     "hf", "hf"),
    ("T5 beams", "t5", "ones", dict(do_sample=False, num_beams=5, max_new_tokens=8), "hf", "hf"),
    ("shipped beam family, T5", "t5", "ones", T.SHIPPED_BEAMS, "hf", "hf"),
    ("an unsupported model_type with beams", "opt", "ones", dict(do_sample=False, num_beams=5, max_new_tokens=8), "hf", "hf"),
]


def _generate_decision(model_type, mask, request, owner):
    from videotgb_amd.decode import envelope_for
    from videotgb_amd.models import _LSTPBase
    lm, emb, am = T._envelope_inputs(model_type, mask)
    kw = {k: v for k, v in request.items() if k not in ("do_sample", "temperature", "stopping_criteria", "max_new_tokens", "use_cache")}
    try:
        plan = _LSTPBase._graph_plan(lm, emb, am, request.get("do_sample", False), request.get("temperature"), request.get("stopping_criteria"), kw,
                                     envelope_for(owner, module=False))
    except AssertionError:
        return "AssertionError"
    return "hf" if plan is None else T._canonical(plan)


def _module_decision(model_type, mask, request, owner, monkeypatch):
    from videotgb_amd import decode
    lm, emb, am = T._envelope_inputs(model_type, mask)
    calls = []

    class Recorder:
        def __init__(self, lm_):
            self.lm, self.key = lm_, decode.weights_key(lm_)

        def generate(self, inputs_embeds, max_new_tokens, **kwargs):
            calls.append(dict(kwargs, max_new_tokens=max_new_tokens))
            return "ids"
    monkeypatch.setattr(decode, "make_decoder", Recorder)
    out = decode.graph_generate(owner, lm, emb, am, request)
    assert (out is None and not calls) or (out == "ids" and len(calls) == 1)
    return "hf" if out is None else T._canonical(calls[0])


@pytest.mark.parametrize("case", OPT_IN, ids=[c[0] for c in OPT_IN])
def test_opt_in_envelopes(case, monkeypatch):
    name, model_type, mask, request, want_generate, want_module = case
    owner = types.SimpleNamespace(beam_search="graph")
    assert _generate_decision(model_type, mask, request, owner) == want_generate, name
    if "stopping_criteria" not in request:
        assert _module_decision(model_type, mask, request, owner, monkeypatch) == want_module, name


@pytest.mark.parametrize("case", T.ENVELOPE, ids=[c[0] for c in T.ENVELOPE])
def test_without_the_option_every_decision_is_todays(case, monkeypatch):
    """An owner without ``beam_search`` (and one that says "hf") gets the decisions of the existing table, row by row; with "graph" every
    row that does not ask for beams or for a length as max_length keeps its decision as well."""
    name, model_type, mask, request, want_generate, want_module = case
    for owner in (types.SimpleNamespace(), types.SimpleNamespace(beam_search="hf")):
        assert _generate_decision(model_type, mask, request, owner) == want_generate, name
        if "stopping_criteria" not in request:
            assert _module_decision(model_type, mask, request, owner, monkeypatch) == want_module, name
    if request.get("num_beams", 1) == 1 and "max_length" not in request:
        owner = types.SimpleNamespace(beam_search="graph")
        assert _generate_decision(model_type, mask, request, owner) == want_generate, name
        if "stopping_criteria" not in request:
            assert _module_decision(model_type, mask, request, owner, monkeypatch) == want_module, name


def test_envelope_values_are_unchanged():
    from videotgb_amd import decode as D
    assert D.GENERATE_ENVELOPE.beams is False and D.MODULE_ENVELOPE.beams is False
    assert D.GENERATE_ENVELOPE[:4] == D.GENERATE_ENVELOPE_BEAMS[:4] and D.GENERATE_ENVELOPE_BEAMS.beams
    assert D.MODULE_ENVELOPE_BEAMS.keys == D.MODULE_ENVELOPE.keys | {"max_length", "min_length"} and D.MODULE_ENVELOPE_BEAMS[1:4] == D.MODULE_ENVELOPE[1:4]
    assert "max_length" not in D.MODULE_ENVELOPE.keys and D.MODULE_ENVELOPE.neutral == {"num_beams": (1,), "repetition_penalty": (1.0,)}
    with pytest.raises(ValueError):
        D.envelope_for(types.SimpleNamespace(beam_search="yes"), module=True)
