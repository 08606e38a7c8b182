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
