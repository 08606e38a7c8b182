"""Beam search over the fp8 K/V cache of the Llama graph decoder (opt-in: beam_search="graph+kv8" / "graph+t5+kv8" with kv_cache="fp8";
``GreedyDecoder(fp8_beams=True)``), the part that needs no GPU.  The decoder's torch statement (``fused=False``, fp32) against a reference
that shares none of its code: HF ``generate`` (transformers' ``_beam_search``) over a cache that rounds every K and V row through
``ops.fp8_kv_round`` as it is stored -- token for token, on the tiny Llama of test_beam_decode.py (lm_head x 40: unscaled random-init
logits are nearly flat and every beam ties).  Then the keyword and the two ``beam_search`` values from the decoder up to the public
constructors, and the proof that nothing changes without them."""
import functools
import types
import warnings

import pytest
import torch

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
def _decoder(kv_cache="fp8", fp8_beams=True):
    from videotgb_amd.decode import GreedyDecoder
    return GreedyDecoder(_llama(), fused=False, kv_cache=kv_cache, fp8_beams=fp8_beams)


@functools.lru_cache(maxsize=None)
def _inputs(B):
    g = torch.Generator().manual_seed(3 + B)
    x = torch.randn(B, P, 32, generator=g)
    m = torch.ones(B, P, dtype=torch.long)
    if B > 1:
        m[1, :3] = 0      # a padded row (leading pads)
    return x, m


def _rounding_cache():
    """A DynamicCache whose ``update`` stores -- and so hands to the attention -- K (after rotary) and V as the fp8 cache holds them."""
    from transformers import DynamicCache
    from videotgb_amd import ops

    class RoundingCache(DynamicCache):
        def update(self, key_states, value_states, *args, **kwargs):
            return super().update(ops.fp8_kv_round(key_states), ops.fp8_kv_round(value_states), *args, **kwargs)
    return RoundingCache(config=_llama().config)


@functools.lru_cache(maxsize=None)
def _hf(B, **kw):
    x, m = _inputs(B)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return _llama().generate(inputs_embeds=x, attention_mask=m, do_sample=False, pad_token_id=0, past_key_values=_rounding_cache(), **kw)


@functools.lru_cache(maxsize=None)
def _ours(B, kv_cache="fp8", fp8_beams=True, **kw):
    x, m = _inputs(B)
    return _decoder(kv_cache, fp8_beams).generate(x, N_NEW, attention_mask=m, pad_token_id=0, **kw)


@functools.lru_cache(maxsize=None)
def _eos_ids(B, K):
    """eos ids chosen from what the model emits: tokens of the unconstrained search's output from the third position on."""
    free = _hf(B, num_beams=K, repetition_penalty=1.5, max_new_tokens=N_NEW, eos_token_id=None)
    seen = []
    for t in free[:, 2:].flatten().tolist():
        if t not in seen and t != 0:
            seen.append(t)
    return tuple(seen[:4])


def test_the_reference_cache_rounds():
    """The reference is what it claims: the K/V it stored (R = 9 rows) are fixed points of the rounding."""
    from videotgb_amd import ops
    x, m = _inputs(3)
    cache = _rounding_cache()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = _llama().generate(inputs_embeds=x, attention_mask=m, do_sample=False, pad_token_id=0, past_key_values=cache, num_beams=3,
                                repetition_penalty=1.5, max_new_tokens=N_NEW, eos_token_id=None, return_dict_in_generate=True)
    layer = out.past_key_values.layers[0]
    assert layer.keys.shape[0] == 9 and layer.keys.shape[2] >= P
    assert torch.equal(ops.fp8_kv_round(layer.keys), layer.keys) and torch.equal(ops.fp8_kv_round(layer.values), layer.values)


CASES = [(B, K) for B in (1, 3) for K in (2, 3, 5)]


@pytest.mark.parametrize("B,K", CASES)
def test_ids_equal_hf_generate_over_a_rounding_cache(B, K):
    for eos in (None,) + _eos_ids(B, K):
        kw = dict(num_beams=K, repetition_penalty=1.5, length_penalty=1.0, eos_token_id=eos)
        ref, out = _hf(B, max_new_tokens=N_NEW, **kw), _ours(B, **kw)
        assert torch.equal(out, ref), (B, K, eos, out.tolist(), ref.tolist())
        if eos is not None:
            n = (ref == eos).int().argmax(-1)
            has = (ref == eos).any(-1)
            for b in range(B):      # pad_token_id = 0: a finished row is filled with EOS (HF: ``pad_token_id or eos_token_id``)
                if has[b]:
                    assert (ref[b, n[b]:] == eos).all() and (out[b, n[b]:] == eos).all()


def test_the_eos_ids_end_rows_early_and_leave_rows_running():
    """What the cases above cover (the references are shared with them): for each batch size some eos id ends a row before the last
    position and some row runs to the end.  (Per case it need not hold: at B = 1, K = 5 the best beam avoids every one of the ids.)"""
    for B in (1, 3):
        ended = full = False
        for K in (2, 3, 5):
            for eos in _eos_ids(B, K):
                ref = _hf(B, max_new_tokens=N_NEW, num_beams=K, repetition_penalty=1.5, length_penalty=1.0, eos_token_id=eos)
                n, has = (ref == eos).int().argmax(-1), (ref == eos).any(-1)
                ended |= bool((has & (n < ref.shape[1] - 1)).any()) or ref.shape[1] < N_NEW
                full |= bool((~has).any())
        assert ended and full, B


def test_the_shipped_sf_generate_configs():
    B = 3
    ref = _hf(B, **dict(SHIPPED_SF, max_length=P + N_NEW))      # over embeddings HF generates max_length - P tokens, min_length - P < 0: no block
    out = _ours(B, num_beams=5, repetition_penalty=1.5, length_penalty=1, eos_token_id=2, min_new_tokens=max(1 - P, 0))
    assert ref.shape[1] <= N_NEW and torch.equal(out, ref)


@pytest.mark.parametrize("length_penalty", [0.0, 2.0])
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


@pytest.mark.parametrize("K", [3, 5])
def test_the_switch_matters(K):
    """At B = 3 the fp8 cache's beams are not the bf16 cache's: a decoder that ignored kv_cache under beams could not pass the tests above."""
    kw = dict(num_beams=K, repetition_penalty=1.5, length_penalty=1.0, eos_token_id=None)
    assert not torch.equal(_ours(3, **kw), _ours(3, "bf16", False, **kw))


def test_defaults_are_unchanged():
    from videotgb_amd.decode import GreedyDecoder
    x, m = _inputs(1)
    for dec in (GreedyDecoder(_llama(), fused=False, kv_cache="fp8"), GreedyDecoder(_llama(), fused=False, kv_cache="fp8", fp8_beams=False)):
        assert dec.fp8_beams is False
        with pytest.raises(NotImplementedError, match="kv_cache='fp8'"):
            dec.generate(x, 4, num_beams=2)
    # still refused under the flag
    dec = _decoder()
    with pytest.raises(NotImplementedError):
        dec.generate(x, 4, num_beams=2, do_sample=True)
    with pytest.raises(NotImplementedError):
        dec.generate(x, 4, num_beams=2, stop_ids=[[5, 6]])
    with pytest.raises(NotImplementedError):
        dec.generate(x, 4, num_beams=2, eos_token_id=[4, 5])
    # the flag is inert with a bf16 cache: the plain beam decoder's ids, the plain decoder's greedy ids
    for B in (1, 3):
        kw = dict(num_beams=3, repetition_penalty=1.5, length_penalty=1.0, eos_token_id=None)
        assert torch.equal(_ours(B, "bf16", True, **kw), _ours(B, "bf16", False, **kw))
        assert torch.equal(_ours(B, "bf16", True), _ours(B, "bf16", False)) and torch.equal(_ours(B, "fp8", True), _ours(B, "fp8", False))


def test_check_beam_search():
    from videotgb_amd import decode
    assert decode.MODES["beam_search"] == ("hf", "graph", "graph+t5", "graph+kv8", "graph+t5+kv8")
    for good in decode.MODES["beam_search"]:
        assert decode.check_mode("beam_search", good) == good
    for bad in ("on", "t5", "graph+T5", "kv8", True, None):
        with pytest.raises(ValueError):
            decode.check_mode("beam_search", bad)


def test_envelope_for():
    from videotgb_amd import decode as D
    for module in (False, True):
        def env(mode):
            return D.envelope_for(types.SimpleNamespace(beam_search=mode), module=module)
        assert env("graph+kv8") == env("graph") and env("graph+t5+kv8") == env("graph+t5")
        assert env("graph+kv8").beams and not env("graph+kv8").t5_beams and env("graph+t5+kv8").t5_beams and not env("hf").beams
        with pytest.raises(ValueError):
            env("kv8")


def test_decoder_for_follows_the_owners_beam_search(monkeypatch):
    from transformers import T5Config, T5ForConditionalGeneration
    from videotgb_amd import decode, llm
    lm = llm.build_llama("tiny", torch.bfloat16, "cpu", seed=7, num_hidden_layers=3, num_key_value_heads=1)
    owner = types.SimpleNamespace(kv_cache="fp8", beam_search="graph")
    d0 = decode.decoder_for(owner, lm)
    assert d0.kv_cache == "fp8" and d0.fp8_beams is False and decode.decoder_for(owner, lm) is d0
    owner.beam_search = "graph+kv8"
    d1 = decode.decoder_for(owner, lm)
    assert d1 is not d0 and d1.kv_cache == "fp8" and d1.fp8_beams is True and d1.weights == "bf16" and decode.decoder_for(owner, lm) is d1
    owner.beam_search = "graph+t5+kv8"
    assert decode.decoder_for(owner, lm) is d1
    owner.beam_search = "graph"
    d2 = decode.decoder_for(owner, lm)
    assert d2 is not d1 and d2.fp8_beams is False
    owner.beam_search = "kv8"
    with pytest.raises(ValueError):
        decode.decoder_for(owner, lm)
    # a T5 owner: the decoder does not take the keyword, is built once and kept
    t5 = T5ForConditionalGeneration(T5Config(vocab_size=50, d_model=32, d_kv=8, d_ff=64, num_layers=1, num_decoder_layers=1, num_heads=2,
                                             feed_forward_proj="gated-gelu", decoder_start_token_id=0, pad_token_id=0, eos_token_id=1))
    t5_owner = types.SimpleNamespace(beam_search="graph+t5+kv8")
    dt = decode.decoder_for(t5_owner, t5)
    assert isinstance(dt, decode.T5GreedyDecoder) and decode.decoder_for(t5_owner, t5) is dt and not hasattr(dt, "fp8_beams")
    with pytest.raises(TypeError):
        decode.T5GreedyDecoder(t5, fp8_beams=True)
    # without "kv8" make_decoder is called as before: the positional lm alone in the default modes
    calls = []

    def one_argument(lm_):
        calls.append(lm_)
        return types.SimpleNamespace(lm=lm_, key=decode.weights_key(lm_))

    monkeypatch.setattr(decode, "make_decoder", one_argument)
    fresh = types.SimpleNamespace(beam_search="graph+t5")
    dec = decode.decoder_for(fresh, lm)
    assert calls == [lm] and decode.decoder_for(fresh, lm) is dec and calls == [lm]


def test_public_constructors(tmp_path):
    from transformers import T5Config, T5ForConditionalGeneration
    from videotgb_amd import builder_utils, decode, llm, models, modules, synth
    lm = llm.build_llama("tiny", torch.bfloat16, "cpu", seed=9, num_hidden_layers=3, num_key_value_heads=1)
    cfg = synth.tiny_cfg("instructblip")
    for mode in ("graph+kv8", "graph+t5+kv8"):
        m = models.LSTP.from_cfg(cfg, "cpu", language_model=lm, kv_cache="fp8", beam_search=mode)
        assert m.kv_cache == "fp8" and m.beam_search == mode
        dec = decode.decoder_for(m, lm)
        assert dec.kv_cache == "fp8" and dec.fp8_beams is True
    assert decode.decoder_for(models.LSTP.from_cfg(cfg, "cpu", language_model=lm, kv_cache="fp8", beam_search="graph"), lm).fp8_beams is False
    with pytest.raises(ValueError, match="beam_search"):
        models.LSTP.from_cfg(cfg, "cpu", language_model=lm, beam_search="kv8")
    with pytest.raises(ValueError, match="beam_search"):
        models.LSTP(str(tmp_path / "no-such-instructblip"), "cpu", beam_search="graph+kv")       # (before the config is looked for)
    with pytest.raises(ValueError, match="beam_search"):
        builder_utils.load_pretrained_model(str(tmp_path / "x.ckpt"), str(tmp_path / "instructblip"), None, "cpu", load_processors=False,
                                            beam_search="kv8")
    for cls in (modules.LSTPModule, modules.LSTPBlip2Module):
        with pytest.raises(ValueError, match="beam_search"):
            cls(str(tmp_path / "m"), str(tmp_path / "s"), str(tmp_path / "r"), beam_search="graph+t5+KV8")
    t5 = T5ForConditionalGeneration(T5Config(vocab_size=50, d_model=32, d_kv=8, d_ff=64, num_layers=1, num_decoder_layers=1, num_heads=2,
                                             feed_forward_proj="gated-gelu", decoder_start_token_id=0, pad_token_id=0, eos_token_id=1))
    with pytest.raises(NotImplementedError):
        models.LSTP_blip2.from_cfg(synth.tiny_cfg("blip2"), "cpu", language_model=t5, kv_cache="fp8", beam_search="graph+t5+kv8")
    b2 = models.LSTP_blip2.from_cfg(synth.tiny_cfg("blip2"), "cpu", language_model=t5, beam_search="graph+t5+kv8")
    assert b2.beam_search == "graph+t5+kv8" and b2.kv_cache == "bf16"
