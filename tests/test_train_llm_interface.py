"""The ``train_lm`` switch at the public interface, without a GPU: the constructors accept and check it, it stays out of the decoders' modes, and
``train.llama_train_state`` names what the own training graph does not state -- construction with ``train_lm="own"`` raises that reason."""
import inspect

import pytest
import torch
from torch import nn

SEVEN = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


class _Holder:                       # the attribute layout LoraTrainStep expects of an LSTP twin
    def __init__(self, lm):
        self.model = type("M", (), {})()
        self.model.language_model = lm


def _tiny(**kw):
    from videotgb_amd import llm
    return llm.build_llama("tiny", torch.float32, "cpu", **kw)


def test_the_keyword_and_its_values():
    from videotgb_amd import decode, modules, train
    assert train.TRAIN_LM == ("hf", "own")
    for fn in (train.LoraTrainStep.__init__, modules._LSTPLightningBase.__init__):
        assert inspect.signature(fn).parameters["train_lm"].default == "hf"
    assert "train_lm" not in decode.MODES and "train_lm" not in decode.DecodeModes._fields      # the decoders' six stay six
    assert train.check_train_lm("hf") == "hf" and train.check_train_lm("own") == "own"
    with pytest.raises(ValueError, match="train_lm='x'"):
        train.check_train_lm("x")
    with pytest.raises(ValueError, match="train_lm='x'"):
        train.LoraTrainStep(_Holder(_tiny()), 0, train_prefix=False, train_lm="x")


def test_construction_states_the_model_or_raises_the_reason():
    from videotgb_amd import train
    for kw in ({}, dict(num_key_value_heads=1), dict(attention_bias=True, mlp_bias=True)):
        step = train.LoraTrainStep(_Holder(_tiny(**kw)), 0, train_prefix=False, train_lm="own")
        assert step.train_lm == "own" and train.llama_train_state(step.lm) is None
    step = train.LoraTrainStep(_Holder(_tiny()), 0, train_prefix=False, train_lm="own", lora_target_modules=SEVEN)
    assert train.llama_train_state(step.lm) is None and len(step.params) == 2 * 7 * step.lm.config.num_hidden_layers
    assert train.LoraTrainStep(_Holder(_tiny()), 0, train_prefix=False).train_lm == "hf"
    refused = _tiny(attention_dropout=0.1)
    with pytest.raises(NotImplementedError, match="attention_dropout 0.1"):
        train.LoraTrainStep(_Holder(refused), 0, train_prefix=False, train_lm="own")
    assert not any(isinstance(m, train.LoraLinear) for m in refused.modules()) and all(p.requires_grad for p in refused.parameters())      # untouched
    train.LoraTrainStep(_Holder(_tiny(attention_dropout=0.1)), 0, train_prefix=False, train_lm="hf")      # HF's path takes any model, as today


def test_a_seq2seq_language_model_is_refused():
    from transformers import T5Config, T5ForConditionalGeneration
    from videotgb_amd import train
    t5 = T5ForConditionalGeneration(T5Config(vocab_size=64, d_model=16, d_kv=8, d_ff=32, num_layers=1, num_heads=2))
    with pytest.raises(NotImplementedError, match="Llama language model only"):
        train.LoraTrainStep(_Holder(t5), 0, train_prefix=False, train_lm="own")
    assert "model_type 't5'" in train.llama_train_state(t5)
    assert not any(isinstance(m, train.LoraLinear) for m in t5.modules())      # refused before anything was changed


def test_llama_train_state_names_each_reason():
    from videotgb_amd import train

    def state(lm, lora=True, **kw):
        if lora:
            train.apply_lora(lm, **kw)
        return train.llama_train_state(lm)

    assert state(_tiny()) is None
    frozen = _tiny()
    for p in frozen.parameters():
        p.requires_grad = False
    assert state(frozen, lora=False) is None                     # no adapter at all: the gradient of the inputs alone (the non-LoRA flavours)
    lm = _tiny()
    train.apply_lora(lm)
    lm.model.layers[1].mlp.down_proj.weight.requires_grad = True
    assert "model.layers.1.mlp.down_proj.weight: a trainable parameter that is no adapter" in train.llama_train_state(lm)
    fresh = _tiny()                                              # a freshly built model's weights are trainable
    assert all(p.requires_grad for p in fresh.parameters())
    assert "a trainable parameter that is no adapter" in train.llama_train_state(fresh)
    assert "rope_type 'dynamic'" in state(_tiny(rope_parameters=dict(rope_type="dynamic", factor=2.0, rope_theta=10000.0)))
    assert state(_tiny(rope_parameters=dict(rope_type="linear", factor=2.0, rope_theta=10000.0))) is None
    assert "hidden_act 'gelu'" in state(_tiny(hidden_act="gelu"))
    assert "attention_dropout 0.1" in state(_tiny(attention_dropout=0.1))
    assert "pretraining_tp 2" in state(_tiny(pretraining_tp=2))
    assert "head_dim 256" in state(_tiny(hidden_size=512, num_attention_heads=2, num_key_value_heads=2))
    assert "head_dim 7" in state(_tiny(hidden_size=28, num_attention_heads=4, num_key_value_heads=4))
    wide = _tiny()
    wide.config.hidden_size, wide.config.head_dim = 8320, 16     # (the state reads the configuration: no need to build 8320-wide weights)
    assert "hidden_size 8320" in state(wide)

    class Foreign(nn.Linear):                                    # an adapter of another library's shape
        def __init__(self, base):
            super().__init__(base.in_features, base.out_features, bias=False)
            self.lora_A, self.lora_B = nn.Linear(base.in_features, 2, bias=False), nn.Linear(2, base.out_features, bias=False)
    lm = _tiny()
    train.apply_lora(lm)
    lm.model.layers[0].self_attn.k_proj = Foreign(lm.model.layers[0].self_attn.k_proj)
    for p in lm.model.layers[0].self_attn.k_proj.parameters():
        p.requires_grad = False
    assert "model.layers.0.self_attn.k_proj: an adapter that is not a train.LoraLinear (Foreign)" in train.llama_train_state(lm)
    lm = _tiny()
    train.apply_lora(lm, target_modules=("q_proj", "lm_head"))
    assert "lm_head: an adapter outside the layers' seven projections" in train.llama_train_state(lm)


def test_the_graph_raises_the_reason_before_any_launch():
    from videotgb_amd import train
    lm = _tiny(attention_dropout=0.1)
    train.apply_lora(lm)
    with pytest.raises(NotImplementedError, match="attention_dropout 0.1"):
        train.llama_with_grad(lm, torch.zeros(1, 3, lm.config.hidden_size), None)
    lm = _tiny()
    train.apply_lora(lm)
    lm.model.norm.weight.requires_grad = True
    with pytest.raises(NotImplementedError, match="model.norm.weight: a trainable parameter"):
        train.llama_with_grad(lm, torch.zeros(1, 3, lm.config.hidden_size), None)
