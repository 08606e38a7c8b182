"""Eos-id sets at the planner and the public interface (opt-in: eos_sets="graph"): under today's envelopes a request with several distinct eos
ids still plans to HF generate; under the ``eos_sets`` twins it plans to the graph decoders with the list in the plan -- Llama and T5, greedy,
sampling and beams --; ``envelope_for`` / ``decoder_for`` read the owner's attribute; the constructors accept and store the parameter."""
import inspect
import types

import pytest
import torch

import test_padded_decode as T

LLAMA31 = [128001, 128008, 128009]      # Llama-3.1-Instruct's generation config


def _inputs(model_type, vocab=128256, mask="ones"):
    lm, emb, am = T._envelope_inputs(model_type, mask)
    lm.config.vocab_size = vocab
    return lm, emb, am


def _plan(model_type, request, env, **kw):
    from videotgb_amd import decode
    lm, emb, am = _inputs(model_type, **kw)
    request = {k: v for k, v in request.items() if k in env.keys or k != "max_new_tokens"}      # (LSTP.generate's envelopes: its own parameter)
    return decode.plan_decode(lm, emb, am, request, env)


def _twins():
    from videotgb_amd import decode as D
    return [(e, e._replace(eos_sets=True)) for e in (D.GENERATE_ENVELOPE, D.MODULE_ENVELOPE, D.GENERATE_ENVELOPE_BEAMS, D.MODULE_ENVELOPE_BEAMS,
                                                     D.GENERATE_ENVELOPE_T5_BEAMS, D.MODULE_ENVELOPE_T5_BEAMS)]


@pytest.mark.parametrize("model_type", ["llama", "t5"])
def test_default_envelopes_send_several_ids_to_hf(model_type):
    from videotgb_amd import decode as D
    for env, _ in _twins():
        assert env.eos_sets is False
        assert _plan(model_type, dict(do_sample=False, max_new_tokens=8, eos_token_id=[2, 7, 9]), env) is None
        assert _plan(model_type, dict(do_sample=False, max_new_tokens=8, eos_token_id=LLAMA31), env) is None
        assert _plan(model_type, dict(do_sample=False, max_new_tokens=8, eos_token_id=[7, 7]), env)["eos_token_id"] == [7]
    lm, emb, am = _inputs(model_type)
    lm.generation_config.eos_token_id = LLAMA31
    assert D.plan_decode(lm, emb, am, dict(do_sample=False), D.GENERATE_ENVELOPE) is None
    assert D.Envelope._field_defaults["eos_sets"] is False


@pytest.mark.parametrize("model_type", ["llama", "t5"])
def test_the_twins_plan_the_list(model_type):
    from videotgb_amd import decode as D
    for _, env in _twins():
        for ids in ([2, 7, 9], LLAMA31, (5, 6), [3, 3, 4]):
            plan = _plan(model_type, dict(do_sample=False, max_new_tokens=8, eos_token_id=ids), env)
            assert plan is not None and plan["eos_token_id"] == list(ids), (env, ids)
        assert _plan(model_type, dict(do_sample=False, max_new_tokens=8, eos_token_id=[7, 7]), env)["eos_token_id"] == [7]      # (one id, repeated: as today)
        assert _plan(model_type, dict(do_sample=False, max_new_tokens=8, eos_token_id=7), env)["eos_token_id"] == 7
    lm, emb, am = _inputs(model_type)
    lm.generation_config.eos_token_id = LLAMA31      # the list as the generation config's default
    plan = D.plan_decode(lm, emb, am, dict(do_sample=False), D.GENERATE_ENVELOPE._replace(eos_sets=True))
    assert plan["eos_token_id"] == LLAMA31 and plan["pad_token_id"] == 0
    padded = _plan(model_type, dict(do_sample=False, max_new_tokens=8, eos_token_id=[2, 7, 9]), D.MODULE_ENVELOPE._replace(eos_sets=True), mask="padded")
    assert padded["eos_token_id"] == [2, 7, 9] and padded["attention_mask"].tolist() == T.PADDED


def test_sampling_and_beams_with_a_set():
    from videotgb_amd import decode as D
    gen = D.GENERATE_ENVELOPE._replace(eos_sets=True)
    plan = _plan("llama", dict(do_sample=True, temperature=0.2, eos_token_id=[2, 7, 9]), gen)
    assert plan["do_sample"] is True and plan["eos_token_id"] == [2, 7, 9]
    assert _plan("t5", dict(do_sample=True, temperature=0.2, eos_token_id=[2, 7, 9]), gen) is None      # (T5 sampling: HF, as today)
    beams = dict(do_sample=False, num_beams=5, repetition_penalty=1.5, max_new_tokens=8, eos_token_id=[2, 7, 9])
    assert _plan("llama", beams, gen) is None      # (beams without beam_search="graph": HF, as today)
    for env, models in ((D.GENERATE_ENVELOPE_BEAMS, ("llama",)), (D.MODULE_ENVELOPE_T5_BEAMS, ("llama", "t5"))):
        for m in models:
            plan = _plan(m, beams, env._replace(eos_sets=True))
            assert plan["num_beams"] == 5 and plan["eos_token_id"] == [2, 7, 9] and plan["repetition_penalty"] == 1.5
            assert _plan(m, beams, env) is None
    assert _plan("t5", beams, D.GENERATE_ENVELOPE_BEAMS._replace(eos_sets=True)) is None


@pytest.mark.parametrize("model_type", ["llama", "t5"])
def test_what_the_twins_leave_to_hf(model_type):
    from videotgb_amd import decode as D, ops
    env = D.GENERATE_ENVELOPE._replace(eos_sets=True)
    assert ops.EOS_MAX == 8
    assert _plan(model_type, dict(do_sample=False, eos_token_id=list(range(1, 10))), env) is None      # 9 ids
    assert _plan(model_type, dict(do_sample=False, eos_token_id=list(range(1, 9))), env) is not None   # 8 ids
    assert _plan(model_type, dict(do_sample=False, eos_token_id=[2, 128256]), env) is None             # an id >= vocab_size
    assert _plan(model_type, dict(do_sample=False, eos_token_id=[2, -1]), env) is None
    assert _plan(model_type, dict(do_sample=False, eos_token_id=[2, 7.0]), env) is None
    assert _plan(model_type, dict(do_sample=False, eos_token_id=LLAMA31), env, vocab=32000) is None
    lm, emb, am = T._envelope_inputs(model_type, "ones")      # a config without vocab_size: no id can be checked
    assert D.plan_decode(lm, emb, am, dict(do_sample=False, eos_token_id=[2, 7]), env) is None


def test_envelope_for_reads_the_owner():
    from videotgb_amd import decode as D
    for beam_search, (gen, mod) in (("hf", (D.GENERATE_ENVELOPE, D.MODULE_ENVELOPE)), ("graph", (D.GENERATE_ENVELOPE_BEAMS, D.MODULE_ENVELOPE_BEAMS)),
                                    ("graph+kv8", (D.GENERATE_ENVELOPE_BEAMS, D.MODULE_ENVELOPE_BEAMS)),
                                    ("graph+t5", (D.GENERATE_ENVELOPE_T5_BEAMS, D.MODULE_ENVELOPE_T5_BEAMS))):
        for owner in (types.SimpleNamespace(beam_search=beam_search), types.SimpleNamespace(beam_search=beam_search, eos_sets="hf")):
            assert D.envelope_for(owner, module=False) is gen and D.envelope_for(owner, module=True) is mod      # today's very objects
        owner = types.SimpleNamespace(beam_search=beam_search, eos_sets="graph")
        assert D.envelope_for(owner, module=False) == gen._replace(eos_sets=True) and D.envelope_for(owner, module=True) == mod._replace(eos_sets=True)
    assert D.envelope_for(types.SimpleNamespace(), module=False) is D.GENERATE_ENVELOPE
    with pytest.raises(ValueError):
        D.envelope_for(types.SimpleNamespace(eos_sets="on"), module=False)


def test_check_eos_sets():
    from videotgb_amd.decode import check_mode
    assert [check_mode("eos_sets", v) for v in ("hf", "graph")] == ["hf", "graph"]
    for bad in ("on", "Graph", "graph+t5", True, False, None, 1):
        with pytest.raises(ValueError):
            check_mode("eos_sets", bad)


def test_decoder_for_builds_the_decoder_with_the_flag(monkeypatch):
    from videotgb_amd import decode as D
    lm, _, _ = _inputs("llama")
    made = []

    class Recorder:
        def __init__(self, lm_, **kw):
            made.append(kw)
            self.lm, self.key, self.eos_sets = lm_, D.weights_key(lm_), kw.get("eos_sets", False)
    monkeypatch.setattr(D, "make_decoder", Recorder)
    owner = types.SimpleNamespace()
    a = D.decoder_for(owner, lm)
    assert made == [{}] and D.decoder_for(owner, lm) is a      # the default modes: the positional lm alone, as today
    owner.eos_sets = "graph"
    b = D.decoder_for(owner, lm)
    assert made[1:] == [dict(eos_sets=True)] and b is not a and D.decoder_for(owner, lm) is b
    owner.eos_sets = "hf"
    assert D.decoder_for(owner, lm) is not b and made[2:] == [{}]
    owner.eos_sets, owner.beam_search, owner.kv_cache, owner.decode_weights = "graph", "graph+kv8", "fp8", "fp8"      # orthogonal to the other modes
    D.decoder_for(owner, lm)
    assert made[3:] == [dict(weights="fp8", kv_cache="fp8", fp8_beams=True, eos_sets=True)]


def test_make_decoder_hands_the_flag_on():
    import test_llama_variants as LV
    import test_t5_beam_decode as TT
    from videotgb_amd import decode as D
    assert D.make_decoder(LV._llama()).eos_sets is False and D.make_decoder(LV._llama(), eos_sets=True).eos_sets is True
    assert D.make_decoder(TT._t5()).eos_sets is False and D.make_decoder(TT._t5(), eos_sets=True).eos_sets is True


def test_graph_generate_serves_the_set_on_the_host_path(monkeypatch):
    """``graph_generate`` of an owner that says eos_sets="graph": the module's configuration with a list reaches a decoder built with the flag
    and the ids are HF's; the same owner without the attribute leaves the request to HF (None)."""
    import test_eos_sets as E
    import test_llama_variants as LV
    from videotgb_amd import decode as D
    ids = E._eos_set("llama")
    x, m = LV._inputs(False)
    cfgs = dict(do_sample=False, max_new_tokens=E.N_LLAMA, eos_token_id=list(ids), pad_token_id=0)

    class OnDevice:      # what plan_decode reads of the embeddings (it serves embeddings on the device only; the decoder runs its torch path here)
        is_cuda, shape = True, x.shape
    real_plan, real_make = D.plan_decode, D.make_decoder
    monkeypatch.setattr(D, "plan_decode", lambda lm, emb, am, gc, env: real_plan(lm, OnDevice, am, gc, env))
    monkeypatch.setattr(D, "make_decoder", lambda lm, **kw: D.GreedyDecoder(lm, fused=False, **kw))
    out = D.graph_generate(types.SimpleNamespace(eos_sets="graph"), LV._llama(), x, m, cfgs)
    assert out is not None and torch.equal(out, E._hf("llama", eos_token_id=list(ids), pad_token_id=0))
    assert D.graph_generate(types.SimpleNamespace(), LV._llama(), x, m, cfgs) is None
    assert D.graph_generate(types.SimpleNamespace(eos_sets="hf"), LV._llama(), x, m, cfgs) is None
    assert real_make is not None


def test_the_constructors_accept_and_store_the_parameter():
    from videotgb_amd import builder_utils, models, modules
    for fn in (models._LSTPBase.__init__, models._LSTPBase.from_cfg.__func__, builder_utils.load_pretrained_model, modules._LSTPLightningBase.__init__):
        p = inspect.signature(fn).parameters
        assert p["eos_sets"].default == "hf" and "beam_search" in p, fn
    assert issubclass(models.LSTP, models._LSTPBase) and issubclass(models.LSTP_blip2, models._LSTPBase)
    assert "__init__" not in vars(models.LSTP) and "__init__" not in vars(models.LSTP_blip2)      # (both take the base's parameters)
    with pytest.raises(ValueError, match="eos_sets"):
        models.LSTP("nowhere", "cpu", eos_sets="on")      # (checked before the path is read)
    with pytest.raises(ValueError, match="eos_sets"):
        builder_utils.load_pretrained_model("ckpt", "instructblip", "sampler", "cpu", load_processors=False, eos_sets="on")
    src = inspect.getsource(modules._LSTPLightningBase.__init__)
    assert 'self.eos_sets = check_mode("eos_sets", eos_sets)' in src and 'self.eos_sets = check_mode("eos_sets", eos_sets)' in inspect.getsource(models._LSTPBase.__init__)
