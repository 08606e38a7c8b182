"""Padded prompt batches on the graph decoders (CPU, eager torch step): the ids must be HF generate's for the same
inputs_embeds + attention_mask -- which pins HF's padding semantics (per-row rotary positions cumsum(mask) - 1 with pads at 0,
decode positions position_ids[b, P-1] + step, pad keys masked for the whole decode; T5: pad keys masked in the encoder's
self-attention and the decoder's cross-attention) against the installed transformers."""
import os
import re
import types

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1      # VTGB_EINVAL (include/vtgb.h)
NEW = ("vtgb_llm_rope_cache_pos", "vtgb_llm_rope_cache_parts_pos", "vtgb_llm_rope_cache_prefill_pos", "vtgb_llm_decode_attention_masked",
       "vtgb_llm_attention_rows_masked")


def _llama(layers=3):
    from videotgb_amd import llm
    return llm.build_llama("tiny", torch.float32, "cpu", seed=3, num_hidden_layers=layers, num_key_value_heads=1)


def _tiny_t5():
    from transformers import T5Config, T5ForConditionalGeneration
    torch.manual_seed(0)
    cfg = T5Config(vocab_size=120, d_model=32, d_kv=16, d_ff=64, num_layers=2, num_decoder_layers=2, num_heads=2, feed_forward_proj="gated-gelu",
                   tie_word_embeddings=False, decoder_start_token_id=0, pad_token_id=0, eos_token_id=1, architectures=["T5ForConditionalGeneration"])
    lm = T5ForConditionalGeneration(cfg).eval()
    for p in lm.parameters():
        p.data.normal_(0, 0.3)
    return lm


def _masks(B, P):
    """left padding, right padding and prefix | right-padded question (pads in the middle of the sequence); every row has tokens"""
    lens = [P - 2 * (b % 3) for b in range(B)]
    left = torch.stack([torch.arange(P) >= P - n for n in lens]).long()
    right = torch.stack([torch.arange(P) < n for n in lens]).long()
    pre = 3
    mid = torch.cat([torch.ones(B, pre, dtype=torch.long), right[:, : P - pre]], 1)
    return dict(left=left, right=right, mid=mid)


def _emb(B, P, H, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, P, H, generator=g) * 0.5


@pytest.mark.parametrize("kind", ["left", "right", "mid"])
def test_llama_padded_ids_equal_hf_generate(kind):
    from videotgb_amd.decode import GreedyDecoder
    lm = _llama()
    B, P = 5, 9
    emb, am = _emb(B, P, 32, 0), _masks(B, P)[kind]
    assert not bool(am.all())
    dec = GreedyDecoder(lm, fused=False)
    ref = lm.generate(inputs_embeds=emb, attention_mask=am, do_sample=False, max_new_tokens=8, min_new_tokens=8)
    out = dec.generate(emb, 8, use_graph=False, attention_mask=am)
    assert out.tolist() == ref.tolist(), (kind, out.tolist(), ref.tolist())
    # the same state on another ragged batch of the same shape (device buffers rewritten, nothing recompiled)
    am2 = am.flip(0)
    ref2 = lm.generate(inputs_embeds=emb * 0.9, attention_mask=am2, do_sample=False, max_new_tokens=8, min_new_tokens=8)
    assert dec.generate(emb * 0.9, 8, use_graph=False, attention_mask=am2).tolist() == ref2.tolist()
    assert sum(1 for k in dec.graphs if k[-1]) == 1


@pytest.mark.parametrize("kind", ["left", "right", "mid"])
def test_llama_padded_eos_and_min_new_tokens_equal_hf(kind):
    from videotgb_amd.decode import GreedyDecoder
    lm = _llama()
    B, P = 5, 7
    emb, am = _emb(B, P, 32, 1), _masks(B, P)[kind]
    free = lm.generate(inputs_embeds=emb, attention_mask=am, do_sample=False, max_new_tokens=9, min_new_tokens=9)
    dec = GreedyDecoder(lm, fused=False)
    for eos in (int(free[0, 2]), int(free[1, 0]), int(free[3, 4])):
        for mn in (0, 4):
            ref = lm.generate(inputs_embeds=emb, attention_mask=am, do_sample=False, max_new_tokens=9, min_new_tokens=mn, eos_token_id=eos,
                              pad_token_id=0)
            out = dec.generate(emb, 9, use_graph=False, eos_token_id=eos, pad_token_id=0, min_new_tokens=mn, attention_mask=am)
            assert out.tolist() == ref.tolist(), (kind, eos, mn, out.tolist(), ref.tolist())


def test_llama_padded_sampling_at_low_temperature_equals_hf_greedy():
    """temperature -> 0: the sampler's inverse CDF lands on the greedy token, padded or not."""
    from videotgb_amd.decode import GreedyDecoder
    lm = _llama()
    B, P = 4, 8
    emb, am = _emb(B, P, 32, 2), _masks(B, P)["right"]
    ref = lm.generate(inputs_embeds=emb, attention_mask=am, do_sample=False, max_new_tokens=6, min_new_tokens=6)
    out = GreedyDecoder(lm, fused=False).generate(emb, 6, use_graph=False, do_sample=True, temperature=1e-4, top_k=0, attention_mask=am,
                                                  sample_noise=torch.full((6, B), 0.5))
    assert out.tolist() == ref.tolist()


def test_left_padded_row_decodes_as_if_alone():
    """Left padding and prefix | pads | question: a row's ids are the ones it gets decoded alone without its pads."""
    from videotgb_amd.decode import GreedyDecoder
    lm = _llama()
    dec = GreedyDecoder(lm, fused=False)
    B, P, pre = 4, 10, 3
    emb = _emb(B, P, 32, 3)
    lens = [10, 7, 5, 8]
    left = torch.stack([torch.arange(P) >= P - n for n in lens]).long()
    mid = torch.stack([(torch.arange(P) < pre) | (torch.arange(P) >= P - (n - pre)) for n in lens]).long()
    for am in (left, mid):
        out = dec.generate(emb, 7, use_graph=False, attention_mask=am)
        for b in range(B):
            alone = dec.generate(emb[b:b + 1, am[b] != 0], 7, use_graph=False)
            assert out[b].tolist() == alone[0].tolist(), (b, am[b].tolist())


def test_t5_padded_ids_equal_hf_generate():
    from videotgb_amd.decode import T5GreedyDecoder
    lm = _tiny_t5()
    B, P = 4, 9
    emb = _emb(B, P, 32, 4)
    dec = T5GreedyDecoder(lm, fused=False)
    for kind, am in _masks(B, P).items():
        ref = lm.generate(inputs_embeds=emb, attention_mask=am, do_sample=False, max_new_tokens=8, min_new_tokens=8)
        out = dec.generate(emb, 8, use_graph=False, attention_mask=am)
        assert out.tolist() == ref.tolist(), (kind, out.tolist(), ref.tolist())
        free = ref
        eos = int(free[1, 3])
        ref = lm.generate(inputs_embeds=emb, attention_mask=am, do_sample=False, max_new_tokens=8, eos_token_id=eos, pad_token_id=0)
        out = dec.generate(emb, 8, use_graph=False, eos_token_id=eos, pad_token_id=0, attention_mask=am)
        assert out.tolist() == ref.tolist(), (kind, "eos", out.tolist(), ref.tolist())


def test_all_ones_mask_takes_the_unpadded_state():
    from videotgb_amd.decode import GreedyDecoder
    lm = _llama(2)
    emb = _emb(3, 6, 32, 5)
    dec = GreedyDecoder(lm, fused=False)
    a = dec.generate(emb, 5, use_graph=False)
    b = dec.generate(emb, 5, use_graph=False, attention_mask=torch.ones(3, 6, dtype=torch.long))
    assert a.tolist() == b.tolist()
    assert len(dec.graphs) == 1 and not next(iter(dec.graphs))[-1]
    assert all("key_valid" not in st for st in dec.graphs.values())


def test_decoders_reject_masks_outside_the_envelope():
    from videotgb_amd.decode import GreedyDecoder
    dec = GreedyDecoder(_llama(1), fused=False)
    emb = _emb(2, 4, 32, 6)
    for bad in (torch.tensor([[1, 1, 2, 1], [1, 1, 1, 1]]), torch.tensor([[0, 0, 0, 0], [1, 1, 1, 1]]), torch.ones(2, 5, dtype=torch.long)):
        with pytest.raises(ValueError):
            dec.generate(emb, 3, use_graph=False, attention_mask=bad)


def test_graph_plan_carries_a_padded_mask():
    from transformers import LlamaConfig
    from videotgb_amd.decode import prompt_padding
    from videotgb_amd.models import _LSTPBase
    lm = types.SimpleNamespace(config=LlamaConfig(model_type="llama"), generation_config=None)
    emb = types.SimpleNamespace(is_cuda=True, shape=(2, 5, 8))          # (the plan reads only these of the embeddings)
    padded = torch.tensor([[1, 1, 1, 0, 0], [1, 1, 1, 1, 1]])
    plan = _LSTPBase._graph_plan(lm, emb, padded, False, 1.0, None, {})
    assert plan is not None and torch.equal(plan["attention_mask"], padded) and plan["attention_mask"].device.type == "cpu"      # (the host copy)
    plan = _LSTPBase._graph_plan(lm, emb, torch.ones(2, 5, dtype=torch.long), False, 1.0, None, {})
    assert plan is not None and "attention_mask" not in plan
    for bad in (torch.tensor([[1, 1, 1, 0, 2], [1, 1, 1, 1, 1]]), torch.tensor([[1, 1, 1, 0, 0], [0, 0, 0, 0, 0]]),
                torch.tensor([[1.0, 0.5, 1.0, 1.0, 1.0], [1.0] * 5])):
        assert _LSTPBase._graph_plan(lm, emb, bad, False, 1.0, None, {}) is None
        assert prompt_padding(bad)[0] is None
    assert prompt_padding(padded)[0] is True and prompt_padding(torch.ones(2, 5))[0] is False


def test_new_symbols_declared_exported_and_bound():
    from videotgb_amd import build
    build.build()
    from videotgb_amd import _lib
    hdr = open(os.path.join(REPO, "include", "vtgb.h")).read()
    declared = set(re.findall(r"\b(vtgb_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS, name
        assert getattr(L, name).argtypes is not None, name
    assert L.vtgb_version() == 601


def test_new_entries_reject_bad_arguments_on_the_host():
    import ctypes as C
    from videotgb_amd import _lib
    L = _lib.lib()
    assert L.vtgb_llm_decode_attention_masked(_lib.F32, None, None, None, None, None, None, 1, 1, 1, 8, 64, 1.0, None) == EINVAL
    assert L.vtgb_llm_rope_cache_pos(_lib.F32, None, None, None, None, None, None, None, None, 1, 1, 1, 8, 64, None) == EINVAL
    assert L.vtgb_llm_rope_cache_prefill_pos(_lib.F32, None, None, None, None, None, None, 1, 4, 1, 1, 8, 64, None) == EINVAL
    a = _lib.LlmAttnRowsArgs(_lib.F32, 4, 2, 16, 4, 4, 4, 1.0, 8, 96, 8, 8, 64, 16, 96, None, 0, 0, None, 8, 32)
    assert L.vtgb_llm_attention_rows_masked(C.byref(a), None, 4, None) == EINVAL


# ------------------------------------------------------------------------------------------------------------- the decode envelope
# Which requests the graph decoders serve and which go to HF generate, for both callers: LSTP.generate (models._LSTPBase._graph_plan: sampling
# and keyword stopping on Llama, greedy on T5) and the LightningModule twins' eval_forward (decode.graph_generate: greedy only, an allow-list
# of keys, max_new_tokens required).  "hf" = HF generate runs the request; a dict = the keyword arguments the decoder's generate receives.
SHIPPED_SAMPLE = dict(length_penalty=1, repetition_penalty=1.0, num_beams=1, min_length=1, max_length=250, top_p=0.9, temperature=1.0, do_sample=True)
SHIPPED_BEAMS = dict(length_penalty=1, repetition_penalty=1.5, num_beams=5, min_length=1, max_length=250, top_p=0.9, temperature=0.8)
ENV_MASKS = {"ones": [[1, 1, 1, 1, 1], [1, 1, 1, 1, 1]], "padded": [[1, 1, 1, 0, 0], [1, 1, 1, 1, 1]], "ones1": [[1, 1, 1, 1, 1]],
             "bad_value": [[1, 1, 1, 0, 2], [1, 1, 1, 1, 1]], "empty_row": [[1, 1, 1, 0, 0], [0, 0, 0, 0, 0]]}
BASE = dict(eos_token_id=2, pad_token_id=0, min_new_tokens=0)      # (the stand-in generation config's defaults)
GREEDY_8 = dict(BASE, max_new_tokens=8)
SAMPLE = dict(BASE, do_sample=True, temperature=0.2, top_k=50, top_p=1.0, sample_noise=None, generator=None)
STOP = dict(BASE, stop_ids=[[5, 6]], text_stop="callable")
PADDED = [[1, 1, 1, 0, 0], [1, 1, 1, 1, 1]]


def _keyword_criteria():
    return types.SimpleNamespace(keyword_ids=[torch.tensor([5, 6])], keywords=["a b"], tokenizer=None, start_len=3, max_keyword_len=2)


# (case, model_type, mask, request, LSTP.generate's decision, eval_forward's decision)
ENVELOPE = [
    ("greedy", "llama", "ones", dict(do_sample=False, max_new_tokens=8), BASE, GREEDY_8),
    ("greedy, settings spelled out", "llama", "ones",
     dict(do_sample=False, max_new_tokens=8, min_new_tokens=4, eos_token_id=7, pad_token_id=3, num_beams=1, repetition_penalty=1.0, use_cache=True),
     dict(eos_token_id=7, pad_token_id=3, min_new_tokens=4), dict(eos_token_id=7, pad_token_id=3, min_new_tokens=4, max_new_tokens=8)),
    ("sampling", "llama", "ones", dict(do_sample=True, temperature=0.2, max_new_tokens=8), SAMPLE, "hf"),
    ("sampling, top_k and top_p", "llama", "ones", dict(do_sample=True, temperature=0.7, top_k=5, top_p=0.8, max_new_tokens=8),
     dict(SAMPLE, temperature=0.7, top_k=5, top_p=0.8), "hf"),
    ("greedy with a temperature and top_p", "llama", "ones", dict(do_sample=False, temperature=0.7, top_p=0.8, max_new_tokens=8), BASE, GREEDY_8),
    ("greedy with top_k", "llama", "ones", dict(do_sample=False, top_k=5, max_new_tokens=8), BASE, "hf"),
    ("num_beams=5", "llama", "ones", dict(do_sample=False, num_beams=5, max_new_tokens=8), "hf", "hf"),
    ("repetition_penalty=1.5", "llama", "ones", dict(do_sample=False, repetition_penalty=1.5, max_new_tokens=8), "hf", "hf"),
    ("repetition_penalty=None", "llama", "ones", dict(do_sample=False, repetition_penalty=None, max_new_tokens=8), BASE, "hf"),
    ("length_penalty=2", "llama", "ones", dict(do_sample=False, length_penalty=2, max_new_tokens=8), "hf", GREEDY_8),
    ("length_penalty=1", "llama", "ones", dict(do_sample=False, length_penalty=1, max_new_tokens=8), BASE, GREEDY_8),
    ("an unknown key", "llama", "ones", dict(do_sample=False, no_repeat_ngram_size=3, max_new_tokens=8), "hf", "hf"),
    ("max_new_tokens missing", "llama", "ones", dict(do_sample=False), BASE, "hf"),
    ("shipped generate_configs, sampling family", "llama", "ones", SHIPPED_SAMPLE, "hf", "hf"),
    ("shipped generate_configs, beam family", "llama", "ones", SHIPPED_BEAMS, "hf", "hf"),
    ("shipped generate_configs, sampling family, its length keys as max_new_tokens", "llama", "ones",
     dict(length_penalty=1, repetition_penalty=1.0, num_beams=1, max_new_tokens=8, top_p=0.9, temperature=1.0, do_sample=True),
     dict(SAMPLE, temperature=1.0, top_p=0.9), "hf"),
    ("shipped generate_configs, sampling family, T5", "t5", "ones", SHIPPED_SAMPLE, "hf", "hf"),
    ("shipped generate_configs, beam family, T5", "t5", "ones", SHIPPED_BEAMS, "hf", "hf"),
    ("keyword stopping, batch 1", "llama", "ones1", dict(do_sample=False, max_new_tokens=8, stopping_criteria=[_keyword_criteria()]), STOP, "hf"),
    ("sampling and keyword stopping, batch 1", "llama", "ones1",
     dict(do_sample=True, temperature=0.2, max_new_tokens=8, stopping_criteria=[_keyword_criteria()]), dict(SAMPLE, stop_ids=[[5, 6]], text_stop="callable"),
     "hf"),
    ("keyword stopping, batch 2", "llama", "ones", dict(do_sample=False, max_new_tokens=8, stopping_criteria=[_keyword_criteria()]), "AssertionError", "hf"),
    ("a foreign criteria object", "llama", "ones1", dict(do_sample=False, max_new_tokens=8, stopping_criteria=[object()]), "hf", "hf"),
    ("no criteria in the list", "llama", "ones", dict(do_sample=False, max_new_tokens=8, stopping_criteria=[]), BASE, "hf"),
    ("padded mask", "llama", "padded", dict(do_sample=False, max_new_tokens=8), dict(BASE, attention_mask=PADDED), dict(GREEDY_8, attention_mask=PADDED)),
    ("padded mask, sampling", "llama", "padded", dict(do_sample=True, temperature=0.2, max_new_tokens=8), dict(SAMPLE, attention_mask=PADDED), "hf"),
    ("a mask value other than 0 / 1", "llama", "bad_value", dict(do_sample=False, max_new_tokens=8), "hf", "hf"),
    ("a row without a token", "llama", "empty_row", dict(do_sample=False, max_new_tokens=8), "hf", "hf"),
    ("T5 greedy", "t5", "ones", dict(do_sample=False, max_new_tokens=8), BASE, GREEDY_8),
    ("T5 greedy, padded mask", "t5", "padded", dict(do_sample=False, max_new_tokens=8), dict(BASE, attention_mask=PADDED), dict(GREEDY_8, attention_mask=PADDED)),
    ("T5 sampling", "t5", "ones", dict(do_sample=True, temperature=0.2, max_new_tokens=8), "hf", "hf"),
    ("T5 keyword stopping", "t5", "ones1", dict(do_sample=False, max_new_tokens=8, stopping_criteria=[_keyword_criteria()]), "hf", "hf"),
    ("T5 num_beams=5", "t5", "ones", dict(do_sample=False, num_beams=5, max_new_tokens=8), "hf", "hf"),
    ("an unsupported model_type", "opt", "ones", dict(do_sample=False, max_new_tokens=8), "hf", "hf"),
    ("an unsupported model_type, sampling", "opt", "ones", dict(do_sample=True, temperature=0.2, max_new_tokens=8), "hf", "hf"),
]


def _envelope_inputs(model_type, mask):
    lm = types.SimpleNamespace(config=types.SimpleNamespace(model_type=model_type), parameters=lambda: iter(()),
                               generation_config=types.SimpleNamespace(eos_token_id=2, pad_token_id=0, top_k=50, top_p=1.0))
    am = torch.tensor(ENV_MASKS[mask])
    return lm, types.SimpleNamespace(is_cuda=True, shape=(am.shape[0], am.shape[1], 8)), am      # (the planners read only these of the embeddings)


def _canonical(kwargs):
    """The decoder call in comparable form: tensors as lists, the text test as "callable", an absent mask = attention_mask=None."""
    out = {k: v.tolist() if isinstance(v, torch.Tensor) else v for k, v in kwargs.items() if not (k == "attention_mask" and v is None)}
    if "text_stop" in out:
        out["text_stop"] = "callable" if callable(out["text_stop"]) else out["text_stop"]
    return out


def _generate_decision(model_type, mask, request):
    """LSTP.generate's planner, called as models._decode calls it: do_sample / temperature / stopping_criteria are generate's own parameters (and
    so are max_new_tokens and use_cache, which the planner never sees); everything else arrives as **gen_kwargs."""
    from videotgb_amd.models import _LSTPBase
    lm, emb, am = _envelope_inputs(model_type, mask)
    kw = {k: v for k, v in request.items() if k not in ("do_sample", "temperature", "stopping_criteria", "max_new_tokens", "use_cache")}
    try:
        plan = _LSTPBase._graph_plan(lm, emb, am, request.get("do_sample", False), request.get("temperature"), request.get("stopping_criteria"), kw)
    except AssertionError:
        return "AssertionError"
    return "hf" if plan is None else _canonical(plan)


def _module_decision(model_type, mask, request, monkeypatch):
    """eval_forward's planner with the request as the module's ``generate_configs``; the decoder is a stand-in that records its call."""
    from videotgb_amd import decode
    lm, emb, am = _envelope_inputs(model_type, mask)
    calls = []

    class Recorder:
        def __init__(self, lm_):
            if lm_.config.model_type != "t5" and "llama" not in lm_.config.model_type:
                raise NotImplementedError(lm_.config.model_type)      # (as decode.make_decoder)
            self.lm, self.key = lm_, decode.weights_key(lm_)

        def generate(self, inputs_embeds, max_new_tokens, **kwargs):
            calls.append(dict(kwargs, max_new_tokens=max_new_tokens))
            return "ids"

    monkeypatch.setattr(decode, "make_decoder", Recorder)
    out = decode.graph_generate(types.SimpleNamespace(), lm, emb, am, request)
    assert (out is None and not calls) or (out == "ids" and len(calls) == 1)
    return "hf" if out is None else _canonical(calls[0])


@pytest.mark.parametrize("case", ENVELOPE, ids=[c[0] for c in ENVELOPE])
def test_decode_envelope_of_both_callers(case, monkeypatch):
    name, model_type, mask, request, want_generate, want_module = case
    assert _generate_decision(model_type, mask, request) == want_generate, name
    if "stopping_criteria" not in request:      # (the modules' generate_configs come from a YAML file: no criteria objects there)
        assert _module_decision(model_type, mask, request, monkeypatch) == want_module, name


# ------------------------------------------------------------------------------------------------------------- the decoder accessor
def test_frame_answers_retires_a_decoder_whose_weights_changed():
    """The decoders hold re-packed COPIES of the weights (q|k|v, gate|up): after an in-place update of the language model (an optimizer step)
    refine.frame_answers must decode with a new decoder -- its ids are a fresh decoder's and HF generate's, not the cached decoder's."""
    from videotgb_amd import refine
    from videotgb_amd.decode import decoder_for
    lm = _llama(2)
    B, num_frames, max_length = 2, 2, 17
    prefix = _emb(B * num_frames, 3, 32, 8)
    model = types.SimpleNamespace(language_model=lm, get_input_embeddings=lm.get_input_embeddings,
                                  config=types.SimpleNamespace(text_config=types.SimpleNamespace(architectures=["LLaMAForCausalLM"])))      # (the 0 -> 2 patch applies)

    def owner():
        return types.SimpleNamespace(model=model, prefix=lambda *a: prefix)      # (the visual prefix is not what is tested here)
    frames = torch.zeros(B * num_frames, 3, 8, 8)
    q = torch.randint(3, 120, (B, 5), generator=torch.Generator().manual_seed(9))
    qm = torch.ones_like(q)
    emb = torch.cat([prefix, lm.get_input_embeddings()(torch.repeat_interleave(q, num_frames, 0))], 1)
    n_new = max_length - emb.shape[1]

    def hf():
        out = lm.generate(inputs_embeds=emb, attention_mask=torch.ones(emb.shape[:2], dtype=torch.long), do_sample=False, max_new_tokens=n_new)
        out[out == 0] = 2
        return out.tolist()
    lstp = owner()
    assert refine.frame_answers(lstp, frames, B, None, None, q, qm, max_length=max_length).tolist() == hf()
    old = lstp._decoder
    assert decoder_for(lstp, lm) is old                                           # unchanged weights: the cached decoder
    with torch.no_grad():
        for p in lm.model.layers.parameters():
            if p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())) * 0.3)
    with torch.no_grad():
        emb = torch.cat([prefix, lm.get_input_embeddings()(torch.repeat_interleave(q, num_frames, 0))], 1)
    stale = old.generate(emb, n_new, eos_token_id=2, pad_token_id=0)
    stale[stale == 0] = 2
    got = refine.frame_answers(lstp, frames, B, None, None, q, qm, max_length=max_length).tolist()
    assert lstp._decoder is not old
    assert got == refine.frame_answers(owner(), frames, B, None, None, q, qm, max_length=max_length).tolist() == hf()
    assert got != stale.tolist()
