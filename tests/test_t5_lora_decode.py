"""LoRA-adapted Flan-T5 models on the T5 graph decoder, on the host (the torch statement of the model, ``fused=False``): ``apply_lora``
with no targets puts peft's default adapters on a T5 (q and v of every SelfAttention of both stacks and of every EncDecAttention); the
decoder applies them unmerged, as train.LoraLinear.forward does, so its ids are HF generate's over the LoraLinear model, greedy and under
beam search; an adapter set it does not serve is named, refused and left to HF generate; and a state dict keyed as a reference LoRA
checkpoint loads strictly into ``LSTP_blip2(lora=True)`` and the SEQ_2_SEQ_LM LightningModule twin."""
import functools
import warnings

import pytest
import torch
from torch import nn

from conftest import full_state_dict, write_hf_config
from lora_refs import nonzero_lora_

B, P, D, N = 3, 7, 64, 12
L_E = L_D = 3


def _t5(dk=16):
    """The tiny T5 of tests/test_gpu_t5_beam_decode.py, fp32."""
    from transformers import T5Config, T5ForConditionalGeneration
    torch.manual_seed(0)
    cfg = T5Config(vocab_size=200, d_model=D, d_kv=dk, d_ff=96, num_layers=L_E, num_decoder_layers=L_D, num_heads=4, feed_forward_proj="gated-gelu",
                   tie_word_embeddings=False, decoder_start_token_id=0, pad_token_id=0, eos_token_id=1)
    lm = T5ForConditionalGeneration(cfg).eval()
    for p in lm.parameters():
        p.data.normal_(0, 0.3 if dk == 16 else 0.15)
    with torch.no_grad():
        lm.lm_head.weight.mul_(4.0)
    return lm


def _lm(dk=16, lora=True, **apply_kw):
    from videotgb_amd import train
    lm = _t5(dk)
    if lora:
        train.apply_lora(lm, **apply_kw)
        nonzero_lora_(lm, seed=5, std=0.3)
        lm.eval()
    return lm


def _inputs(padded=True):
    x = torch.randn(B, P, D, generator=torch.Generator().manual_seed(5 + B)) * 0.5
    m = torch.ones(B, P, dtype=torch.long)
    if padded:
        m[1, -2:] = 0
    return x, m


def _hf(lm, x, m, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return lm.generate(inputs_embeds=x, attention_mask=m, do_sample=False, pad_token_id=0, **kw)


GREEDY = dict(max_new_tokens=N, min_new_tokens=N)
BEAMS = dict(max_new_tokens=N, num_beams=3, repetition_penalty=1.5)


def _decode(lm, x, m, padded, beams):
    from videotgb_amd.decode import T5GreedyDecoder
    kw = dict(num_beams=3, repetition_penalty=1.5, eos_token_id=1) if beams else dict(min_new_tokens=N, eos_token_id=1)
    return T5GreedyDecoder(lm, fused=False).generate(x, N, use_graph=False, pad_token_id=0, attention_mask=m if padded else None, **kw)


# ------------------------------------------------------------------------------------------------------------------------------ creation
def _expected_keys():
    keys = []
    for stack, n, atts in (("encoder", L_E, ("layer.0.SelfAttention",)), ("decoder", L_D, ("layer.0.SelfAttention", "layer.1.EncDecAttention"))):
        for i in range(n):
            for att in atts:
                for proj in ("q", "v"):
                    for ab in ("lora_A", "lora_B"):
                        keys.append(f"{stack}.block.{i}.{att}.{proj}.{ab}.default.weight")
    return sorted(keys)


def test_apply_lora_without_targets_creates_pefts_adapters_on_a_t5():
    from videotgb_amd import train
    lm = _t5()
    params = train.apply_lora(lm)
    got = sorted(k for k in lm.state_dict() if "lora_" in k)
    assert len(got) == 2 * (2 * L_E + 4 * L_D) == 36 and got == _expected_keys()
    assert "decoder.block.0.layer.1.EncDecAttention.q.lora_A.default.weight" in got
    assert len(params) == 36 and all(p.requires_grad for p in params)
    assert [n for n, p in lm.named_parameters() if p.requires_grad and "lora_" not in n] == []
    a = lm.decoder.block[0].layer[1].EncDecAttention.q
    assert (a.r, a.lora_alpha, a.scaling) == (8, 32, 4.0) and tuple(a.lora_A["default"].weight.shape) == (8, D)


def test_apply_lora_on_a_llama_creates_what_it_created():
    from videotgb_amd import llm, train
    made = []
    for kw in ({}, dict(target_modules=("q_proj", "v_proj"))):
        lm = llm.build_llama("tiny", torch.float32, "cpu", seed=3, num_hidden_layers=3, num_key_value_heads=1)
        train.apply_lora(lm, **kw)
        made.append(sorted(k for k in lm.state_dict() if "lora_" in k))
    assert made[0] == made[1] and len(made[0]) == 3 * 2 * 2
    assert all(".self_attn.q_proj." in k or ".self_attn.v_proj." in k for k in made[0])


def test_an_explicit_tuple_behaves_as_before_on_a_t5():
    from videotgb_amd import train
    lm = _t5()
    assert train.apply_lora(lm, target_modules=("q_proj", "v_proj")) == []


# --------------------------------------------------------------------------------------------------------------------------------- the ids
@pytest.mark.parametrize("dk", [16, 64])
@pytest.mark.parametrize("padded", [False, True])
def test_greedy_ids_equal_hf_generate_over_the_lora_model(dk, padded):
    from videotgb_amd.decode import T5GreedyDecoder, lora_state
    lm = _lm(dk)
    x, m = _inputs(padded)
    assert lora_state(lm) == "ok"
    dec = T5GreedyDecoder(lm, fused=False)
    assert [[len(s) for s in dec.lora[k]] for k in ("enc", "sa", "cq", "ckv")] == [[2] * L_E, [2] * L_D, [1] * L_D, [1] * L_D]
    assert [s[0] for s in dec.lora["sa"][0]] == [0, 2 * 4 * dk] and dec.lora["ckv"][0][0][0] == 4 * dk      # q and v of q|k|v; v of k|v
    ref = _hf(lm, x, m, eos_token_id=1, **GREEDY)
    assert _decode(lm, x, m, padded, False).tolist() == ref.tolist()


@pytest.mark.parametrize("dk", [16, 64])
def test_beam_ids_equal_hf_generate_over_the_lora_model(dk):
    lm = _lm(dk)
    x, m = _inputs()
    ref = _hf(lm, x, m, eos_token_id=1, **BEAMS)
    assert _decode(lm, x, m, True, True).tolist() == ref.tolist()


@pytest.mark.parametrize("dk", [16, 64])
@pytest.mark.parametrize("beams", [False, True])
def test_the_adapters_change_the_ids(dk, beams):
    """(Otherwise the equalities above would hold for a decoder that ignored them.)  Same base weights, same inputs: every row differs."""
    from videotgb_amd.decode import T5GreedyDecoder, lora_state
    base = _lm(dk, lora=False)
    assert lora_state(base) is None and T5GreedyDecoder(base, fused=False).lora is None
    x, m = _inputs()
    with_lora, without = _decode(_lm(dk), x, m, True, beams), _decode(base, x, m, True, beams)
    assert without.tolist() == _hf(base, x, m, eos_token_id=1, **(BEAMS if beams else GREEDY)).tolist()
    n = min(with_lora.shape[1], without.shape[1])
    assert all(with_lora[b, :n].tolist() != without[b, :n].tolist() or with_lora.shape[1] != without.shape[1] for b in range(B))


def test_an_adapter_on_k_is_served_too():
    from videotgb_amd.decode import T5GreedyDecoder
    lm = _lm(target_modules=("q", "k", "v"), r=4, lora_alpha=6)
    dec = T5GreedyDecoder(lm, fused=False)
    assert [[len(s) for s in dec.lora[k]] for k in ("enc", "sa", "cq", "ckv")] == [[3] * L_E, [3] * L_D, [1] * L_D, [2] * L_D]
    assert [s[0] for s in dec.lora["sa"][0]] == [0, 64, 128] and [s[0] for s in dec.lora["ckv"][0]] == [0, 64] and dec.lora["sa"][0][0][3] == 1.5
    x, m = _inputs()
    assert _decode(lm, x, m, True, False).tolist() == _hf(lm, x, m, eos_token_id=1, **GREEDY).tolist()
    assert _decode(lm, x, m, True, True).tolist() == _hf(lm, x, m, eos_token_id=1, **BEAMS).tolist()


def test_zero_adapters_decode_as_the_base_model():
    """apply_lora's initial state (B = 0): the update is exactly zero."""
    from videotgb_amd import train
    lm = _lm(lora=False)
    x, m = _inputs()
    want = _decode(lm, x, m, True, False)
    train.apply_lora(lm)
    lm.eval()
    assert _decode(lm, x, m, True, False).tolist() == want.tolist()


def test_the_decoder_reads_the_models_own_adapter_parameters():
    """The segments reference the parameters: an in-place update of lora_B (a training step) is what the next step applies."""
    from videotgb_amd.decode import T5GreedyDecoder
    lm = _lm()
    dec = T5GreedyDecoder(lm, fused=False)
    q = lm.decoder.block[0].layer[1].EncDecAttention.q
    assert dec.lora["cq"][0][0][2].data_ptr() == q.lora_B["default"].weight.data_ptr()
    assert dec.lora["cq"][0][0][1].data_ptr() == q.lora_A["default"].weight.data_ptr()


# ------------------------------------------------------------------------------------------------------------------------------- routing
def _also_on(name):
    return lambda: _lm(target_modules=("q", "v", name))


def _not_fp32():
    lm = _lm()
    lm.decoder.block[1].layer[1].EncDecAttention.v.lora_B.to(torch.bfloat16)
    return lm


def _with_bias():
    from videotgb_amd import train
    lm = _lm(lora=False)
    a = lm.encoder.block[0].layer[0].SelfAttention
    a.q = train.LoraLinear(nn.Linear(D, 64, bias=True))
    return lm.eval()


def _training_with_dropout():
    return _lm().train()


UNSERVABLE = {"o": (_also_on("o"), "outside q / k / v"), "wi_0": (_also_on("wi_0"), "outside q / k / v"), "lm_head": (_also_on("lm_head"), "outside q / k / v"),
              "adapters that are not fp32": (_not_fp32, "not fp32"), "a bias": (_with_bias, "bias"),
              "training mode with dropout": (_training_with_dropout, "dropout")}


class _OnDevice:
    """What plan_decode reads of ``inputs_embeds`` (its placement and batch size), claiming a device: the host has none."""
    is_cuda = True
    shape = (B, P, D)


def _plan(lm):
    from videotgb_amd.decode import MODULE_ENVELOPE, plan_decode
    return plan_decode(lm, _OnDevice(), torch.ones(B, P, dtype=torch.long), dict(max_new_tokens=N, do_sample=False), MODULE_ENVELOPE)


@pytest.mark.parametrize("case", sorted(UNSERVABLE))
def test_unservable_adapters_are_named_refused_and_left_to_hf_generate(case):
    from videotgb_amd.decode import T5GreedyDecoder, lora_state
    make, word = UNSERVABLE[case]
    lm = make()
    state = lora_state(lm)
    assert state not in (None, "ok") and word in state and "T5" in state, state
    with pytest.raises(NotImplementedError, match="T5"):
        T5GreedyDecoder(lm, fused=False)
    assert _plan(lm) is None


def test_servable_models_are_planned():
    """(The plans above are None because of the adapters, not because of the stand-in for a device tensor.)"""
    assert _plan(_lm()) is not None and _plan(_lm(lora=False)) is not None


# ------------------------------------------------------------------------------------------------------------------------- strict loading
@functools.lru_cache(maxsize=None)
def _tiny_blip2(tmp):
    from videotgb_amd import models
    from videotgb_amd.synth import tiny_cfg
    cfg = tiny_cfg("blip2")
    base = write_hf_config(tmp + "/blip2-tiny", "blip2", cfg, "t5")
    return cfg, base, full_state_dict(cfg, models.build_language_model(models.load_hf_config(base, "blip2")))


def _reference_lora_state_dict(sd, lm):
    """``sd`` as a reference LoRA checkpoint keys it: the language model below peft's ``base_model.model.`` level, with the adapter tensors
    peft creates on a T5 (q and v of every attention block) under peft's names."""
    lp = "model.language_model."
    out = {(lp + "base_model.model." + k[len(lp):] if k.startswith(lp) else k): v for k, v in sd.items()}
    g = torch.Generator().manual_seed(11)
    n = 0
    for name, mod in lm.named_modules():
        if name.rsplit(".", 1)[-1] in ("q", "v") and isinstance(mod, nn.Linear) and ("SelfAttention" in name or "EncDecAttention" in name):
            out[f"{lp}base_model.model.{name}.lora_A.default.weight"] = torch.randn(8, mod.in_features, generator=g)
            out[f"{lp}base_model.model.{name}.lora_B.default.weight"] = torch.randn(mod.out_features, 8, generator=g)
            n += 2
    return out, n


def test_a_reference_lora_checkpoint_loads_strictly_into_lstp_blip2(tmp_path):
    from videotgb_amd import models
    from videotgb_amd.decode import lora_state
    cfg, base, sd = _tiny_blip2(str(tmp_path))
    m = models.LSTP_blip2(base, "cpu", True, compute_dtype="f32", tgb_cfg=cfg.tgb)
    lm = m.model.language_model
    ref_sd, n = _reference_lora_state_dict(sd, models.build_language_model(models.load_hf_config(base, "blip2")))
    assert n == 2 * (2 * 2 + 4 * 2) and sum("lora_" in k for k in m.state_dict()) == n
    res = m.load_state_dict(ref_sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    key = "model.language_model.base_model.model.decoder.block.1.layer.1.EncDecAttention.q.lora_B.default.weight"
    assert torch.equal(lm.decoder.block[1].layer[1].EncDecAttention.q.lora_B["default"].weight, ref_sd[key])
    assert not lm.training and lora_state(lm) == "ok"


def test_a_reference_lora_checkpoint_loads_strictly_into_the_seq2seq_twin(tmp_path):
    from videotgb_amd import models, modules
    from videotgb_amd.decode import lora_state
    cfg, base, sd = _tiny_blip2(str(tmp_path))
    raft_pth = str(tmp_path / "raft-things.pth")
    torch.save({"module." + k[len("of_extractor."):]: v for k, v in sd.items() if k.startswith("of_extractor.")}, raft_pth)
    sampler_pth = str(tmp_path / "sampler.pth")      # (the IV / IVT modules load a trained sampler's DataParallel state dict)
    torch.save({"module." + k[len("temporal_encoder."):]: v for k, v in sd.items() if k.startswith("temporal_encoder.")}, sampler_pth)
    assert modules.LSTPBlip2IVTModule.LORA == "SEQ_2_SEQ_LM"
    m = modules.LSTPBlip2IVTModule(model_name_or_path=base, sampler_name_or_path=sampler_pth, of_extractor_name_or_path=raft_pth,
                                   generate_configs=dict(max_new_tokens=4), compute_dtype="f32", processor=object(), tgb_cfg=cfg.tgb)
    lm = m.model.language_model
    ref_sd, n = _reference_lora_state_dict(sd, models.build_language_model(models.load_hf_config(base, "blip2")))
    assert sum("lora_" in k for k in m.state_dict()) == n == 24
    res = m.load_state_dict(ref_sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    # the reference's freeze_weights leaves the language model to peft: the adapters train, the T5's own weights do not; the optimizer
    # takes exactly the trainable parameters
    lora = [p for k, p in lm.named_parameters() if "lora_" in k]
    assert len(lora) == n and all(p.requires_grad for p in lora)
    assert not any(p.requires_grad for k, p in lm.named_parameters() if "lora_" not in k)
    assert not any(p.requires_grad for p in m.temporal_encoder.parameters()) and not any(p.requires_grad for p in m.of_extractor.parameters())
    m.hparams.optimizer = lambda params: torch.optim.SGD(params, lr=0.1)
    m.hparams.scheduler = None
    opt_ids = {id(p) for gr in m.configure_optimizers()["optimizer"].param_groups for p in gr["params"]}
    assert {id(p) for p in lora} <= opt_ids and opt_ids == {id(p) for p in m.parameters() if p.requires_grad}
    assert lora_state(lm.eval()) == "ok"
