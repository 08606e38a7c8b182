"""A one-beam repetition penalty at the planner and the public interface (opt-in: penalty_decode="graph"): under today's envelopes such a
request still plans to HF generate; under the ``penalty`` twins it plans to the graph decoders with the scalar in the plan -- Llama and T5,
greedy, and Llama sampling --; a neutral penalty plans exactly as today; ``envelope_for`` / ``decoder_for`` read the owner's attribute; the
constructors accept and store the parameter."""
import inspect
import types

import pytest
import torch

import test_padded_decode as T

DEMO = dict(do_sample=True, top_p=0.9, temperature=1.0, num_beams=1, repetition_penalty=1.5, length_penalty=1.0)      # demo/utils/model.py, the slider at 1


def _plan(model_type, request, env, mask="ones"):
    from videotgb_amd import decode
    lm, emb, am = T._envelope_inputs(model_type, mask)
    request = {k: v for k, v in request.items() if k in env.keys or k != "max_new_tokens"}      # (LSTP.generate's envelopes: its own parameter)
    return decode.plan_decode(lm, emb, am, request, env)


def _envelopes():
    from videotgb_amd import decode as D
    return (D.GENERATE_ENVELOPE, D.MODULE_ENVELOPE, D.GENERATE_ENVELOPE_BEAMS, D.MODULE_ENVELOPE_BEAMS, D.GENERATE_ENVELOPE_T5_BEAMS,
            D.MODULE_ENVELOPE_T5_BEAMS, D.GENERATE_ENVELOPE._replace(eos_sets=True))


@pytest.mark.parametrize("model_type", ["llama", "t5"])
def test_todays_envelopes_send_the_penalty_to_hf(model_type):
    from videotgb_amd import decode as D
    for env in _envelopes():
        assert env.penalty is False
        for p in (1.5, 0.7, 2):
            assert _plan(model_type, dict(do_sample=False, max_new_tokens=8, repetition_penalty=p), env) is None, (env, p)
            assert _plan(model_type, dict(do_sample=False, max_new_tokens=8, num_beams=1, repetition_penalty=p), env) is None
    assert _plan(model_type, DEMO, D.GENERATE_ENVELOPE) is None
    assert D.Envelope._field_defaults["penalty"] is False
    assert D.Envelope._fields[D.Envelope._fields.index("eos_sets") + 1] == "penalty" and D.Envelope._fields[-2:] == ("beams", "t5_beams")


@pytest.mark.parametrize("model_type", ["llama", "t5"])
def test_the_twins_plan_the_penalty(model_type):
    from videotgb_amd import decode as D
    for env in _envelopes():
        twin = env._replace(penalty=True)
        for p, want in ((1.5, 1.5), (0.7, 0.7), (2, 2.0), (1e-3, 1e-3)):
            plan = _plan(model_type, dict(do_sample=False, max_new_tokens=8, num_beams=1, repetition_penalty=p), twin)
            assert plan is not None and plan["repetition_penalty"] == want and type(plan["repetition_penalty"]) is float, (env, p)
            assert "num_beams" not in plan and "length_penalty" not in plan
            base = _plan(model_type, dict(do_sample=False, max_new_tokens=8, num_beams=1), env)
            assert {k: v for k, v in plan.items() if k != "repetition_penalty"} == base      # everything else is today's plan
    padded = _plan(model_type, dict(do_sample=False, max_new_tokens=8, repetition_penalty=1.5), D.MODULE_ENVELOPE._replace(penalty=True), mask="padded")
    assert padded["repetition_penalty"] == 1.5 and padded["attention_mask"].tolist() == T.PADDED
    assert _plan(model_type, dict(do_sample=False, repetition_penalty=1.5, eos_token_id=7), D.GENERATE_ENVELOPE._replace(penalty=True))["eos_token_id"] == 7


def test_llama_sampling_with_the_penalty_and_the_demo_request():
    from videotgb_amd import decode as D
    gen = D.GENERATE_ENVELOPE._replace(penalty=True)
    plan = _plan("llama", DEMO, gen)
    assert plan["do_sample"] is True and plan["top_p"] == 0.9 and plan["repetition_penalty"] == 1.5 and "num_beams" not in plan
    assert _plan("t5", DEMO, gen) is None      # (T5 sampling: HF, as today)
    assert _plan("t5", dict(DEMO, do_sample=False), gen)["repetition_penalty"] == 1.5
    # the module envelope samples only under sampled_decode="graph": the penalty changes nothing about that
    mod = D.MODULE_ENVELOPE._replace(penalty=True)
    assert _plan("llama", dict(do_sample=True, max_new_tokens=8, repetition_penalty=1.5), mod) is None
    both = D.envelope_for(types.SimpleNamespace(penalty_decode="graph", sampled_decode="graph"), module=True)
    shipped = dict(do_sample=True, top_p=0.9, temperature=1, num_beams=1, repetition_penalty=1.5, length_penalty=1, min_length=1, max_length=40)
    plan = _plan("llama", shipped, both)
    assert plan["do_sample"] is True and plan["repetition_penalty"] == 1.5
    # beams keep their own path: several beams need the beam envelopes, with or without the penalty switch
    beams = dict(do_sample=False, num_beams=5, repetition_penalty=1.5, max_new_tokens=8)
    assert _plan("llama", beams, gen) is None and _plan("llama", beams, mod) is None
    plan = _plan("llama", beams, D.GENERATE_ENVELOPE_BEAMS._replace(penalty=True))
    assert plan == _plan("llama", beams, D.GENERATE_ENVELOPE_BEAMS) and plan["num_beams"] == 5 and plan["repetition_penalty"] == 1.5


@pytest.mark.parametrize("model_type", ["llama", "t5"])
def test_a_neutral_penalty_plans_exactly_as_today(model_type):
    for env in _envelopes():
        twin = env._replace(penalty=True)
        none_ok = None in env.neutral["repetition_penalty"]
        for req in (dict(do_sample=False, max_new_tokens=8), dict(do_sample=False, max_new_tokens=8, repetition_penalty=1.0),
                    dict(do_sample=False, max_new_tokens=8, repetition_penalty=1), dict(do_sample=False, max_new_tokens=8, num_beams=1, repetition_penalty=1.0)):
            a, b = _plan(model_type, req, env), _plan(model_type, req, twin)
            assert a is not None and a == b and "repetition_penalty" not in b, (env, req)
        req = dict(do_sample=False, max_new_tokens=8, repetition_penalty=None)      # None counts as 1 under the twin
        b = _plan(model_type, req, twin)
        assert b is not None and "repetition_penalty" not in b and b == _plan(model_type, dict(do_sample=False, max_new_tokens=8), env)
        assert (_plan(model_type, req, env) is not None) == none_ok


@pytest.mark.parametrize("model_type", ["llama", "t5"])
def test_what_the_twins_leave_to_hf(model_type):
    from videotgb_amd import decode as D
    for env in (D.GENERATE_ENVELOPE._replace(penalty=True), D.MODULE_ENVELOPE._replace(penalty=True)):
        for bad in (0, 0.0, -1.5, "1.5", True, False, [1.5], float("nan"), float("inf"), 1.5 + 0j):
            assert _plan(model_type, dict(do_sample=False, max_new_tokens=8, repetition_penalty=bad), env) is None, (env, bad)
        assert _plan(model_type, dict(do_sample=False, max_new_tokens=8, repetition_penalty=1.5, num_beams=2), env) is None
        assert _plan(model_type, dict(do_sample=False, max_new_tokens=8, repetition_penalty=1.5, no_repeat_ngram_size=2), env) is None
        assert _plan(model_type, dict(do_sample=False, max_new_tokens=8, repetition_penalty=1.5, encoder_repetition_penalty=1.2), env) is None
    assert _plan(model_type, dict(do_sample=False, repetition_penalty=1.5, length_penalty=2.0), D.GENERATE_ENVELOPE._replace(penalty=True)) is None


def test_envelope_for_reads_the_owner():
    from videotgb_amd import decode as D
    for beam_search, (gen, mod) in (("hf", (D.GENERATE_ENVELOPE, D.MODULE_ENVELOPE)), ("graph", (D.GENERATE_ENVELOPE_BEAMS, D.MODULE_ENVELOPE_BEAMS)),
                                    ("graph+kv8", (D.GENERATE_ENVELOPE_BEAMS, D.MODULE_ENVELOPE_BEAMS)),
                                    ("graph+t5", (D.GENERATE_ENVELOPE_T5_BEAMS, D.MODULE_ENVELOPE_T5_BEAMS))):
        for owner in (types.SimpleNamespace(beam_search=beam_search), types.SimpleNamespace(beam_search=beam_search, penalty_decode="hf")):
            assert D.envelope_for(owner, module=False) is gen and D.envelope_for(owner, module=True) is mod      # today's very objects
        owner = types.SimpleNamespace(beam_search=beam_search, penalty_decode="graph")
        assert D.envelope_for(owner, module=False) == gen._replace(penalty=True) and D.envelope_for(owner, module=True) == mod._replace(penalty=True)
    owner = types.SimpleNamespace(eos_sets="graph", penalty_decode="graph")
    assert D.envelope_for(owner, module=False) == D.GENERATE_ENVELOPE._replace(eos_sets=True, penalty=True)
    assert D.envelope_for(types.SimpleNamespace(), module=False) is D.GENERATE_ENVELOPE
    with pytest.raises(ValueError):
        D.envelope_for(types.SimpleNamespace(penalty_decode="on"), module=False)


def test_check_penalty_decode():
    from videotgb_amd.decode import check_mode
    assert [check_mode("penalty_decode", v) for v in ("hf", "graph")] == ["hf", "graph"]
    for bad in ("on", "Graph", "graph+t5", "", True, False, None, 1, 1.5, ("graph",)):
        with pytest.raises(ValueError, match="penalty_decode"):
            check_mode("penalty_decode", bad)


def test_decoder_for_builds_the_decoder_with_the_flag(monkeypatch):
    from videotgb_amd import decode as D
    lm, _, _ = T._envelope_inputs("llama", "ones")
    made = []

    class Recorder:
        def __init__(self, lm_, **kw):
            made.append(kw)
            self.lm, self.key, self.penalty = lm_, D.weights_key(lm_), kw.get("penalty", False)
    monkeypatch.setattr(D, "make_decoder", Recorder)
    owner = types.SimpleNamespace()
    a = D.decoder_for(owner, lm)
    assert made == [{}] and D.decoder_for(owner, lm) is a      # the default modes: the positional lm alone, as today
    owner.penalty_decode = "graph"
    b = D.decoder_for(owner, lm)
    assert made[1:] == [dict(penalty=True)] and b is not a and D.decoder_for(owner, lm) is b
    owner.penalty_decode = "hf"
    assert D.decoder_for(owner, lm) is not b and made[2:] == [{}]      # rebuilt when the flag differs
    owner.penalty_decode, owner.eos_sets, owner.beam_search, owner.kv_cache, owner.decode_weights = "graph", "graph", "graph+kv8", "fp8", "fp8"
    D.decoder_for(owner, lm)
    assert made[3:] == [dict(weights="fp8", kv_cache="fp8", fp8_beams=True, eos_sets=True, penalty=True)]      # orthogonal to the other modes
    owner.penalty_decode = "on"
    with pytest.raises(ValueError):
        D.decoder_for(owner, lm)


def test_make_decoder_hands_the_flag_on():
    import test_beam_decode as TB
    import test_t5_beam_decode as TT
    from videotgb_amd import decode as D
    assert D.make_decoder(TB._llama()).penalty is False and D.make_decoder(TB._llama(), penalty=True).penalty is True
    assert D.make_decoder(TT._t5()).penalty is False and D.make_decoder(TT._t5(), penalty=True).penalty is True
    both = D.make_decoder(TB._llama(), eos_sets=True, penalty=True)
    assert both.eos_sets is True and both.penalty is True
    for cls in (D.GreedyDecoder, D.T5GreedyDecoder):      # ``penalty`` stands after ``eos_sets``
        names = list(inspect.signature(cls.__init__).parameters)
        assert names[names.index("eos_sets") + 1] == "penalty" and inspect.signature(cls.__init__).parameters["penalty"].default is False


@pytest.mark.parametrize("model", ["llama", "t5"])
def test_graph_generate_serves_the_penalty_on_the_host_path(monkeypatch, model):
    """``graph_generate`` of an owner that says penalty_decode="graph": the module's configuration reaches a decoder built with the flag and
    the ids are HF's; an owner without the attribute leaves the request to HF (None)."""
    import test_penalty_decode as PD
    from videotgb_amd import decode as D
    mod = PD.TB if model == "llama" else PD.TT
    lm = mod._llama() if model == "llama" else mod._t5()
    x, m = mod._inputs(3)
    cfgs = dict(do_sample=False, max_new_tokens=PD.N_NEW[model], num_beams=1, repetition_penalty=1.5, eos_token_id=None, pad_token_id=0)

    class OnDevice:      # what plan_decode reads of the embeddings (it serves embeddings on the device only; the decoder runs its torch path here)
        is_cuda, shape = True, x.shape
    real_plan = D.plan_decode
    monkeypatch.setattr(D, "plan_decode", lambda lm_, emb, am, gc, env: real_plan(lm_, OnDevice, am, gc, env))
    monkeypatch.setattr(D, "make_decoder", lambda lm_, **kw: (D.GreedyDecoder if model == "llama" else D.T5GreedyDecoder)(lm_, fused=False, **kw))
    owner = types.SimpleNamespace(penalty_decode="graph")
    out = D.graph_generate(owner, lm, x, m, cfgs)
    assert out is not None and owner._decoder.penalty is True
    assert torch.equal(out if model == "llama" else out[:, 1:], PD._hf(model, 3, repetition_penalty=1.5, eos_token_id=None))
    assert D.graph_generate(types.SimpleNamespace(), lm, x, m, cfgs) is None
    assert D.graph_generate(types.SimpleNamespace(penalty_decode="hf"), lm, x, m, cfgs) is None


def test_the_constructors_accept_and_store_the_parameter():
    from videotgb_amd import builder_utils, models, modules
    for fn in (models._LSTPBase.__init__, models._LSTPBase.from_cfg.__func__, builder_utils.load_pretrained_model, modules._LSTPLightningBase.__init__):
        p = inspect.signature(fn).parameters
        named = [n for n, v in p.items() if v.kind is not inspect.Parameter.VAR_KEYWORD]
        assert p["penalty_decode"].default == "hf" and named[-1] == "penalty_decode", fn      # the keyword goes last
    assert issubclass(models.LSTP, models._LSTPBase) and issubclass(models.LSTP_blip2, models._LSTPBase)
    assert "__init__" not in vars(models.LSTP) and "__init__" not in vars(models.LSTP_blip2)      # (both take the base's parameters)
    with pytest.raises(ValueError, match="penalty_decode"):
        models.LSTP("nowhere", "cpu", penalty_decode="on")      # (checked before the path is read)
    with pytest.raises(ValueError, match="penalty_decode"):
        builder_utils.load_pretrained_model("ckpt", "instructblip", "sampler", "cpu", load_processors=False, penalty_decode="on")
    for cls in (models._LSTPBase, modules._LSTPLightningBase):
        assert 'self.penalty_decode = check_mode("penalty_decode", penalty_decode)' in inspect.getsource(cls.__init__)
