"""The six owner-level decode modes (decode.MODES) in all 3 x 2 x 5 x 2 x 2 x 2 = 240 combinations, against tests/golden/decode_modes.json:
what the commit named in its "source" field -- the last one with six hand-plumbed switches -- returned for the same owners.  Per combination:
the envelope ``envelope_for`` returns for LSTP.generate and for the module twins, the keywords ``decoder_for`` hands to ``make_decoder`` for a
tiny Llama and a tiny T5, and for every row of the planner tests' request table whether ``plan_decode`` plans it and with which keys; per
mode, the exact words every entry point refuses a bad value with."""
import functools
import itertools
import json
import os
import types

import pytest

import test_beam_decode as TB
import test_padded_decode as T
import test_t5_beam_decode as TT
from conftest import GOLDEN


@functools.lru_cache(maxsize=None)
def _golden():
    with open(os.path.join(GOLDEN, "decode_modes.json")) as f:
        return json.load(f)


NAMES = ("decode_weights", "kv_cache", "beam_search", "eos_sets", "sampled_decode", "penalty_decode")
VALUES = (("bf16", "fp8", "mxfp4"), ("bf16", "fp8"), ("hf", "graph", "graph+t5", "graph+kv8", "graph+t5+kv8"), ("hf", "graph"), ("hf", "graph"),
          ("hf", "graph"))
COMBINATIONS = list(itertools.product(*VALUES))
# the request table's rows as the planner tests run them on the CPU (the stand-in embeddings of ``T._envelope_inputs``: no device tensor):
# LSTP.generate's planner never sees max_new_tokens / use_cache, the modules' configurations carry no criteria objects
ROWS = [(i, module) for i, case in enumerate(T.ENVELOPE) for module in (False, True) if not (module and "stopping_criteria" in case[3])]


def _owner(combination):
    return types.SimpleNamespace(**dict(zip(NAMES, combination)))


def _json(value):
    return json.loads(json.dumps(value))


def _envelope_record(env):
    """Sorted keys, the neutral table and every flag by field name."""
    return dict(keys=sorted(env.keys), neutral={k: list(v) for k, v in env.neutral.items()}, **{f: getattr(env, f) for f in env._fields[2:]})


def _decoder_keywords(combination, lm, monkeypatch):
    from videotgb_amd import decode as D
    made = []

    class Recorder:
        def __init__(self, lm_, **kw):
            made.append(kw)
            self.lm, self.key = lm_, D.weights_key(lm_)
    monkeypatch.setattr(D, "make_decoder", Recorder)
    D.decoder_for(_owner(combination), lm)
    assert len(made) == 1
    return made[0]


def _plan_outcome(combination, i, module):
    from videotgb_amd import decode as D
    _, model_type, mask, request, *_ = T.ENVELOPE[i]
    lm, emb, am = T._envelope_inputs(model_type, mask)
    req = {k: v for k, v in request.items() if module or k not in ("max_new_tokens", "use_cache")}
    try:
        plan = D.plan_decode(lm, emb, am, req, D.envelope_for(_owner(combination), module))
    except AssertionError:
        return "AssertionError"
    return None if plan is None else sorted(plan)


def test_the_fixture_covers_every_combination():
    from videotgb_amd import decode as D
    g = _golden()
    assert tuple(D.MODES) == NAMES == tuple(g["names"]) and tuple(D.MODES.values()) == VALUES
    assert [tuple(c["modes"]) for c in g["combinations"]] == COMBINATIONS and len(COMBINATIONS) == 240
    assert g["rows"] == [[T.ENVELOPE[i][0], module] for i, module in ROWS]
    assert len(g["source"]) == 40


@pytest.mark.parametrize("n", range(len(COMBINATIONS)), ids=["-".join(c) for c in COMBINATIONS])
def test_envelopes_and_decoder_keywords_are_the_sources(n, monkeypatch):
    from videotgb_amd import decode as D
    g, combination = _golden(), COMBINATIONS[n]
    want = g["combinations"][n]
    for module in (False, True):
        assert _json(_envelope_record(D.envelope_for(_owner(combination), module))) == g["envelopes"][want["envelope"][module]], module
    for model, lm in (("llama", TB._llama()), ("t5", TT._t5())):
        assert _json(_decoder_keywords(combination, lm, monkeypatch)) == want["decoder"][model], model


@pytest.mark.parametrize("n", range(len(COMBINATIONS)), ids=["-".join(c) for c in COMBINATIONS])
def test_every_request_plans_as_at_the_source(n):
    g, combination = _golden(), COMBINATIONS[n]
    want = g["combinations"][n]["plans"]
    assert len(want) == len(ROWS)
    for (i, module), w in zip(ROWS, want):
        assert _plan_outcome(combination, i, module) == g["plan_outcomes"][w], (T.ENVELOPE[i][0], module)


@pytest.mark.parametrize("name", NAMES)
def test_bad_values_are_refused_in_the_sources_words(name):
    """An unknown string, None, True, 1 and ["graph"] through ``check_mode``, ``modes_of``, ``LSTP.from_cfg`` and a module twin's constructor
    (``sampled_decode`` is no parameter of ``LSTP``)."""
    from videotgb_amd import decode as D
    from videotgb_amd import models, modules
    twin = modules.TARGETS[sorted(modules.TARGETS)[0]]
    cases = _golden()["errors"][name]
    assert [bad for bad, _ in cases] == ["on", None, True, 1, ["graph"]]
    for bad, message in cases:
        calls = [lambda: D.check_mode(name, bad), lambda: D.modes_of(types.SimpleNamespace(**{name: bad})),
                 lambda: twin(model_name_or_path="nowhere", sampler_name_or_path="nowhere", of_extractor_name_or_path="nowhere", **{name: bad})]
        if name != "sampled_decode":
            calls.append(lambda: models.LSTP.from_cfg(None, "cpu", **{name: bad}))
        for call in calls:
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == message, (bad, str(e.value))
