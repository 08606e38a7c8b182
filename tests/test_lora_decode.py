"""LoRA-adapted Llama models on the graph decoder, on the host (the torch statement of the model, ``fused=False``): the decoder applies
the adapters unmerged, as train.LoraLinear.forward does, so its greedy ids are HF generate's over the LoraLinear model; and an adapter
set the decoders do not serve is never decoded as the base model -- ``lora_state`` names the reason, the decoders raise, ``plan_decode``
hands the request to HF generate."""
import types

import pytest
import torch
from torch import nn

from lora_refs import nonzero_lora_

B, P, N = 3, 9, 12


def _lm(lora=True, seed=3, **apply_kw):
    from videotgb_amd import llm, train
    lm = llm.build_llama("tiny", torch.float32, "cpu", seed=seed, num_hidden_layers=3, num_key_value_heads=1)
    if lora:
        train.apply_lora(lm, **apply_kw)
        nonzero_lora_(lm, seed=5)
        lm.eval()
    return lm


def _emb(seed=0):
    return torch.randn(B, P, 32, generator=torch.Generator().manual_seed(seed)) * 0.5


def _hf(lm, emb, mask):
    return lm.generate(inputs_embeds=emb, attention_mask=mask, do_sample=False, max_new_tokens=N, min_new_tokens=N, use_cache=True)


PADDED = torch.tensor([[1] * 9, [0, 0, 0] + [1] * 6, [1, 1, 0, 1, 1, 1, 0, 1, 1]])


@pytest.mark.parametrize("padded", [False, True])
def test_decoder_ids_equal_hf_generate_over_the_lora_model(padded):
    from videotgb_amd.decode import GreedyDecoder, lora_state
    lm, emb = _lm(), _emb()
    assert lora_state(lm) == "ok"
    mask = PADDED if padded else torch.ones(B, P, dtype=torch.long)
    ref = _hf(lm, emb, mask)
    dec = GreedyDecoder(lm, fused=False)
    assert dec.lora is not None and [len(s) for s in dec.lora] == [2, 2, 2]      # q_proj and v_proj of every layer
    out = dec.generate(emb, N, use_graph=False, attention_mask=mask if padded else None)
    assert out.tolist() == ref.tolist()


def test_the_adapters_change_the_ids():
    """(Otherwise the equality above would hold for a decoder that ignored them.)  Same base weights, same prompts."""
    from videotgb_amd.decode import GreedyDecoder, lora_state
    emb = _emb()
    base = _lm(lora=False)
    assert lora_state(base) is None and GreedyDecoder(base, fused=False).lora is None
    with_lora = GreedyDecoder(_lm(), fused=False).generate(emb, N, use_graph=False)
    without = GreedyDecoder(base, fused=False).generate(emb, N, use_graph=False)
    assert without.tolist() == _hf(base, emb, torch.ones(B, P, dtype=torch.long)).tolist()
    assert with_lora.tolist() != without.tolist()


def test_an_adapter_on_k_proj_is_served_too():
    from videotgb_amd.decode import GreedyDecoder
    lm, emb = _lm(target_modules=("q_proj", "k_proj", "v_proj"), r=4, lora_alpha=6), _emb(1)
    dec = GreedyDecoder(lm, fused=False)
    assert [len(s) for s in dec.lora] == [3, 3, 3] and [s[0] for s in dec.lora[0]] == [0, 32, 48]      # 2 heads of 16, 1 K/V head
    assert dec.generate(emb, N, use_graph=False).tolist() == _hf(lm, emb, torch.ones(B, P, dtype=torch.long)).tolist()


def test_zero_adapters_decode_as_the_base_model():
    """apply_lora's initial state (B = 0): the update is exactly zero."""
    from videotgb_amd import train
    from videotgb_amd.decode import GreedyDecoder
    lm = _lm(lora=False)
    emb = _emb(2)
    want = GreedyDecoder(lm, fused=False).generate(emb, N, use_graph=False)
    train.apply_lora(lm)
    lm.eval()
    assert GreedyDecoder(lm, fused=False).generate(emb, N, use_graph=False).tolist() == want.tolist()


# ------------------------------------------------------------------------------------------------------------------------------- routing
class _PeftLikeLinear(nn.Linear):
    """Adapters in peft's layout on a module that is not train.LoraLinear."""

    def __init__(self, base):
        super().__init__(base.in_features, base.out_features, bias=False)
        self.lora_A = nn.ModuleDict({"default": nn.Linear(base.in_features, 4, bias=False)})
        self.lora_B = nn.ModuleDict({"default": nn.Linear(4, base.out_features, bias=False)})


def _foreign():
    lm = _lm(lora=False)
    a = lm.model.layers[0].self_attn
    a.q_proj = _PeftLikeLinear(a.q_proj)
    return lm


def _other_projection(name):
    def make():
        return _lm(target_modules=("q_proj", name))
    return make


def _not_fp32():
    lm = _lm()
    lm.model.layers[1].self_attn.v_proj.lora_B.to(torch.bfloat16)
    return lm


def _with_bias():
    from videotgb_amd import train
    lm = _lm(lora=False)
    a = lm.model.layers[0].self_attn
    q = nn.Linear(32, 32, bias=True)
    a.q_proj = train.LoraLinear(q)
    return lm.eval()


def _training_with_dropout():
    return _lm().train()


UNSERVABLE = {"a module that is not a LoraLinear": (_foreign, "not a videotgb_amd.train.LoraLinear"),
              "o_proj": (_other_projection("o_proj"), "outside q_proj"), "the MLP": (_other_projection("down_proj"), "outside q_proj"),
              "lm_head": (_other_projection("lm_head"), "outside q_proj"), "adapters that are not fp32": (_not_fp32, "not fp32"),
              "a bias": (_with_bias, "bias"), "training mode with dropout": (_training_with_dropout, "dropout")}


class _OnDevice:
    """What plan_decode reads of ``inputs_embeds`` (its placement and batch size), claiming a device: the host has none."""
    is_cuda = True
    shape = (B, P, 32)


def _plan(lm):
    from videotgb_amd.decode import MODULE_ENVELOPE, plan_decode
    return plan_decode(lm, _OnDevice(), torch.ones(B, P, dtype=torch.long), dict(max_new_tokens=N, do_sample=False), MODULE_ENVELOPE)


@pytest.mark.parametrize("case", sorted(UNSERVABLE))
def test_unservable_adapters_are_named_refused_and_left_to_hf_generate(case):
    from videotgb_amd.decode import GreedyDecoder, lora_state
    make, word = UNSERVABLE[case]
    lm = make()
    state = lora_state(lm)
    assert state not in (None, "ok") and word in state, state
    with pytest.raises(NotImplementedError, match="LoRA"):
        GreedyDecoder(lm, fused=False)
    assert _plan(lm) is None


def test_servable_models_are_planned():
    """(The plans above are None because of the adapters, not because of the stand-in for a device tensor.)"""
    assert _plan(_lm()) is not None and _plan(_lm(lora=False)) is not None


def test_eval_mode_or_zero_dropout_makes_a_training_model_servable():
    from videotgb_amd.decode import lora_state
    lm = _lm().train()
    assert lora_state(lm) != "ok"
    assert lora_state(lm.eval()) == "ok"
    assert lora_state(_lm(lora_dropout=0.0).train()) == "ok"


def test_a_t5_with_an_adapter_is_refused():
    from videotgb_amd import train
    from videotgb_amd.decode import T5GreedyDecoder, lora_state

    class T5ish(nn.Module):
        def __init__(self):
            super().__init__()
            self.config = types.SimpleNamespace(model_type="t5")
            self.q = train.LoraLinear(nn.Linear(8, 8, bias=False))
    lm = T5ish().eval()
    state = lora_state(lm)
    assert state not in (None, "ok") and "T5" in state
    with pytest.raises(NotImplementedError, match="T5"):
        T5GreedyDecoder(lm)
    assert _plan(lm) is None
