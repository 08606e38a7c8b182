"""Sampled ``generate_configs`` at the planner (opt-in: sampled_decode="graph" on the LightningModule twins): without the opt-in
``envelope_for`` returns the very objects it returned before; with it the literal ``generate_configs`` of the reference's LSTP_blip2.yaml /
LSTP_instructblip.yaml plan to the Llama graph decoder's sampling path with HF's ``max_length`` / ``min_length`` arithmetic, a T5's sampled
requests and beams with sampling still go to HF generate, and every request that planned before plans identically."""
import inspect
import types

import pytest
import torch

import test_padded_decode as T

# configs/model/LSTP_blip2.yaml, LSTP_blip2_IVT.yaml, LSTP_instructblip.yaml and LSTP_instructblip_IV.yaml: one and the same literal dict
SHIPPED_SAMPLED = dict(length_penalty=1, repetition_penalty=1.0, num_beams=1, min_length=1, max_length=250, top_p=0.9, temperature=1.0, do_sample=True)
MODES = ("hf", "graph", "graph+t5", "graph+kv8", "graph+t5+kv8")


def _owner(**kw):
    return types.SimpleNamespace(**kw)


def test_check_sampled_decode():
    from videotgb_amd.decode import MODES, check_mode
    assert MODES["sampled_decode"] == ("hf", "graph")
    assert check_mode("sampled_decode", "hf") == "hf" and check_mode("sampled_decode", "graph") == "graph"
    for bad in ("torch", "", None, True, 1, ["graph"]):
        with pytest.raises(ValueError):
            check_mode("sampled_decode", bad)


def test_without_the_opt_in_the_envelopes_are_the_same_objects():
    from videotgb_amd import decode as D
    want = {("hf", False): D.GENERATE_ENVELOPE, ("hf", True): D.MODULE_ENVELOPE, ("graph", False): D.GENERATE_ENVELOPE_BEAMS,
            ("graph", True): D.MODULE_ENVELOPE_BEAMS, ("graph+t5", False): D.GENERATE_ENVELOPE_T5_BEAMS, ("graph+t5", True): D.MODULE_ENVELOPE_T5_BEAMS}
    for mode in MODES:
        for module in (False, True):
            for owner in (_owner(beam_search=mode), _owner(beam_search=mode, sampled_decode="hf")):
                assert D.envelope_for(owner, module) is want[(mode.replace("+kv8", ""), module)]
        # LSTP.generate's envelope samples already: the opt-in leaves it the same object
        assert D.envelope_for(_owner(beam_search=mode, sampled_decode="graph"), False) is want[(mode.replace("+kv8", ""), False)]
    assert D.envelope_for(_owner(), True) is D.MODULE_ENVELOPE and D.envelope_for(_owner(), False) is D.GENERATE_ENVELOPE
    assert D.Envelope._fields[-2:] == ("beams", "t5_beams")
    assert D.MODULE_ENVELOPE.sampling is False and "max_length" not in D.MODULE_ENVELOPE.keys
    with pytest.raises(ValueError):
        D.envelope_for(_owner(sampled_decode="yes"), True)


def test_the_module_twin_differs_in_sampling_and_the_length_keys():
    from videotgb_amd import decode as D
    for mode in MODES:
        for sets in ("hf", "graph"):
            base = D.envelope_for(_owner(beam_search=mode, eos_sets=sets), True)
            twin = D.envelope_for(_owner(beam_search=mode, eos_sets=sets, sampled_decode="graph"), True)
            assert twin == base._replace(sampling=True, keys=base.keys | {"max_length", "min_length"})
            assert twin.need_max_new and twin.neutral == base.neutral


def _module_call(model_type, request, owner, monkeypatch, P=5):
    """``graph_generate`` with a recording decoder: "hf" | the decoder call."""
    from videotgb_amd import decode
    lm, emb, am = T._envelope_inputs(model_type, "ones")
    if P != 5:
        am = torch.ones(2, P, dtype=torch.long)
        emb = types.SimpleNamespace(is_cuda=True, shape=(2, P, 8))
    calls = []

    class Recorder:
        def __init__(self, lm_, **kw):
            self.lm, self.key = lm_, decode.weights_key(lm_)

        def generate(self, inputs_embeds, max_new_tokens, **kwargs):
            calls.append(dict(kwargs, max_new_tokens=max_new_tokens))
            return "ids"

    monkeypatch.setattr(decode, "make_decoder", Recorder)
    out = decode.graph_generate(owner, lm, emb, am, request)
    assert (out is None and not calls) or (out == "ids" and len(calls) == 1)
    return "hf" if out is None else T._canonical(calls[0])


@pytest.mark.parametrize("beam_search", ["hf", "graph+t5"])
def test_the_shipped_generate_configs_plan_on_llama(beam_search, monkeypatch):
    from videotgb_amd import decode as D
    yaml = SHIPPED_SAMPLED
    sampled = dict(do_sample=True, temperature=1.0, top_k=50, top_p=0.9, sample_noise=None, generator=None)
    for model_type in ("t5", "llama"):
        assert _module_call(model_type, yaml, _owner(beam_search=beam_search), monkeypatch) == "hf"      # today
    call = _module_call("llama", yaml, _owner(beam_search=beam_search, sampled_decode="graph"), monkeypatch, P=40)
    assert call == dict(sampled, eos_token_id=2, pad_token_id=0, min_new_tokens=0, max_new_tokens=250 - 40)      # Llama: max_length - P
    # the prompt fills max_length: HF generate reports it in its own words
    assert _module_call("llama", yaml, _owner(sampled_decode="graph"), monkeypatch, P=250) == "hf"
    # max_new_tokens / min_new_tokens win over max_length / min_length, as in HF
    call = _module_call("llama", dict(yaml, max_new_tokens=8, min_new_tokens=3), _owner(sampled_decode="graph"), monkeypatch)
    assert call["max_new_tokens"] == 8 and call["min_new_tokens"] == 3
    lm, _, _ = T._envelope_inputs("llama", "ones")
    assert D.generated_length(lm, yaml, 40) == (210, 0)


@pytest.mark.parametrize("beam_search", ["hf", "graph+t5"])
def test_a_t5_keeps_its_sampled_requests_on_hf(beam_search, monkeypatch):
    """T5GreedyDecoder does not sample: HF generate, opt-in or not; a T5's greedy requests may use the length keys the twin knows."""
    owner = _owner(beam_search=beam_search, sampled_decode="graph")
    assert _module_call("t5", SHIPPED_SAMPLED, owner, monkeypatch) == "hf"
    assert _module_call("t5", dict(SHIPPED_SAMPLED, max_new_tokens=8), owner, monkeypatch) == "hf"
    call = _module_call("t5", dict(SHIPPED_SAMPLED, do_sample=False), owner, monkeypatch)
    assert call["max_new_tokens"] == 249 and call["min_new_tokens"] == 0 and "do_sample" not in call      # T5: max_length - 1


@pytest.mark.parametrize("model_type", ["llama", "t5"])
def test_beams_with_sampling_still_go_to_hf(model_type, monkeypatch):
    from videotgb_amd import decode as D
    owner = _owner(beam_search="graph+t5", sampled_decode="graph")
    lm, emb, am = T._envelope_inputs(model_type, "ones1")
    for module in (False, True):
        assert D.plan_decode(lm, emb, am, dict(do_sample=True, temperature=0.2, num_beams=5, max_new_tokens=8), D.envelope_for(owner, module)) is None
    assert _module_call(model_type, dict(SHIPPED_SAMPLED, num_beams=5), owner, monkeypatch) == "hf"


def test_every_request_that_planned_before_plans_identically():
    """The case table of the planner tests, under every beam mode: a request the owner's envelope planned without the opt-in gets the same plan
    with it (only refusals may turn into plans)."""
    from videotgb_amd import decode as D
    seen = 0
    for name, model_type, mask, request, *_ in T.ENVELOPE:
        for mode in MODES:
            for module in (False, True):
                if module and "stopping_criteria" in request:
                    continue
                lm, emb, am = T._envelope_inputs(model_type, mask)
                req = {k: v for k, v in request.items() if module or k not in ("max_new_tokens", "use_cache")}

                def plan(owner):
                    try:
                        p = D.plan_decode(lm, emb, am, req, D.envelope_for(owner, module))
                    except AssertionError:
                        return "AssertionError"
                    return None if p is None else T._canonical(p)
                before, after = plan(_owner(beam_search=mode)), plan(_owner(beam_search=mode, sampled_decode="graph"))
                if before is not None:
                    assert after == before, (name, mode, module)
                    seen += 1
    assert seen > 100


def test_the_module_twins_take_check_and_store_the_parameter():
    from videotgb_amd import decode as D
    from videotgb_amd import modules
    twins = [c for c in vars(modules).values() if inspect.isclass(c) and issubclass(c, modules._LSTPLightningBase) and c is not modules._LSTPLightningBase]
    assert twins
    for c in twins:
        assert inspect.signature(c.__init__).parameters["sampled_decode"].default == "hf", c
        for bad in ("fast", None, True):
            with pytest.raises(ValueError, match="sampled_decode"):      # (checked before any path is read)
                c(model_name_or_path="nowhere", sampler_name_or_path="nowhere", of_extractor_name_or_path="nowhere", sampled_decode=bad)
    # the attribute the constructor stores is the one the planner reads from its owner
    assert 'self.sampled_decode = check_mode("sampled_decode", sampled_decode)' in inspect.getsource(modules._LSTPLightningBase.__init__)
    owner = types.SimpleNamespace(sampled_decode=D.check_mode("sampled_decode", "graph"))
    assert D.envelope_for(owner, True).sampling and not D.envelope_for(types.SimpleNamespace(sampled_decode="hf"), True).sampling
