"""The opt-in fp8 K/V cache of the Llama graph decoder (kv_cache="fp8"), the part that needs no GPU: the row format
(ops.quantize_fp8_kv: e4m3 codes and one power-of-two scale per cache row), its agreement with the weight recipe, and the keyword
from the decoders up to the public constructors.  The torch path (``fused=False``) is the kernel-independent statement of the model:
k and v pass through dq(q(.)) as they are produced."""
import types

import pytest
import torch


def _rows(seed=0, shape=(2, 3, 17, 128), std=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * std


# ------------------------------------------------------------------------------------------------------------- the recipe
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("std", [1.0, 0.02, 37.0])
def test_rows_are_bf16_numbers_with_power_of_two_scales_and_a_fixed_point(hd, std):
    from videotgb_amd import ops
    x = _rows(1, (2, 3, 17, hd), std).bfloat16()
    q, scale = ops.quantize_fp8_kv(x)
    assert q.dtype == torch.float8_e4m3fn and q.shape == x.shape and scale.dtype == torch.float32 and scale.shape == x.shape[:-1]
    m, _ = torch.frexp(scale)
    assert torch.equal(m, torch.full_like(m, 0.5))                                  # scale = 2^e
    qf = q.float()
    assert not torch.isnan(qf).any() and qf.abs().max().item() <= 448
    dq = ops.dequantize_fp8_kv(q, scale, torch.float32)
    assert torch.equal(dq.bfloat16().float(), dq)                                   # q * scale is exactly a bf16 number
    assert torch.equal(ops.dequantize_fp8_kv(q, scale).float(), dq)
    q2, scale2 = ops.quantize_fp8_kv(dq)                                            # dq(q(dq(q(x)))) == dq(q(x))
    assert torch.equal(ops.dequantize_fp8_kv(q2, scale2, torch.float32), dq)
    assert torch.equal(ops.fp8_kv_round(x).float(), dq) and ops.fp8_kv_round(x).dtype == x.dtype
    # the amax element of every row is reproduced within one e4m3 step (its scaled value lies in (224, 448]: steps of 32)
    xf = x.float()
    idx = xf.abs().argmax(-1, keepdim=True)
    amax, got = xf.gather(-1, idx)[..., 0], dq.gather(-1, idx)[..., 0]
    assert ((amax / scale).abs() > 224).all() and ((amax / scale).abs() <= 448).all()      # e is the SMALLEST exponent that fits
    assert ((got - amax).abs() <= 32 * scale).all()


def test_zero_rows_tiny_rows_and_the_exponent_clamp():
    from videotgb_amd import ops
    x = torch.zeros(5, 64)
    x[1, 3] = 448.0                     # e = 0
    x[2, 5] = -449.0                    # just above: e = 1
    x[3] = 2.0 ** -120 * torch.linspace(-1, 1, 64)      # e would be about -128: clamped to -100
    x[4, 7] = 448.0 * 2.0 ** -100       # exactly at the clamp
    q, scale = ops.quantize_fp8_kv(x)
    assert scale.tolist() == [1.0, 1.0, 2.0, 2.0 ** -100, 2.0 ** -100]
    assert not q.view(torch.uint8)[0].any()                                         # a zero row: scale 1 and zero codes
    assert q[1, 3].float().item() == 448.0 and q[2, 5].float().item() == -224.0 and q[4, 7].float().item() == 448.0
    dq = ops.dequantize_fp8_kv(q, scale, torch.float32)
    assert torch.isfinite(dq).all() and torch.isfinite(q.float()).all()
    assert not dq[3].any()                                                          # 2^-120 * 2^100 = 2^-20: below half the smallest code (2^-10)
    assert torch.equal(dq.bfloat16().float(), dq)
    assert dq[4, 7].item() == 448.0 * 2.0 ** -100
    nz = dq[dq != 0].abs()
    assert (nz >= 2.0 ** -126).all()                                                # normal bf16 numbers


@pytest.mark.parametrize("hd", [64, 128])
def test_the_recipe_is_the_weight_recipe_on_the_last_dimension(hd):
    from videotgb_amd import ops
    x = (_rows(2, (300, hd)) * torch.logspace(-6, 6, 300, base=2.0)[:, None]).bfloat16()
    x[7] = 0
    (q, s), (qw, sw) = ops.quantize_fp8_kv(x), ops.quantize_fp8_rows(x)
    assert torch.equal(q.view(torch.uint8), qw.view(torch.uint8)) and torch.equal(s, sw)
    q3, s3 = ops.quantize_fp8_kv(x.view(3, 100, hd))
    assert torch.equal(q3.view(torch.uint8).view(300, hd), qw.view(torch.uint8)) and torch.equal(s3.view(300), sw)


# ------------------------------------------------------------------------------------------------------------- the keyword
def _llama(seed=3, dtype=torch.float32, **kw):
    from videotgb_amd import llm
    return llm.build_llama("tiny", dtype, "cpu", seed=seed, num_hidden_layers=3, num_key_value_heads=1, **kw)


def test_check_kv_cache():
    from videotgb_amd import decode
    assert decode.MODES["kv_cache"] == ("bf16", "fp8")
    assert decode.check_mode("kv_cache", "bf16") == "bf16" and decode.check_mode("kv_cache", "fp8") == "fp8"
    for bad in ("int8", "FP8", "e4m3", None, 8):
        with pytest.raises(ValueError):
            decode.check_mode("kv_cache", bad)
        with pytest.raises(ValueError):
            decode.GreedyDecoder(_llama(), fused=False, kv_cache=bad)
        with pytest.raises(ValueError):
            decode.make_decoder(_llama(), kv_cache=bad)


def _first_logits(dec, emb, n):
    rec, pick = [], dec._pick
    dec._pick = lambda st, logits, step: rec.append(logits.float().clone()) or pick(st, logits, step)
    try:
        ids = dec.generate(emb, n, use_graph=False)
    finally:
        del dec._pick
    return ids, rec


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_torch_path_generates_over_a_rounded_cache(dtype):
    """fused=False: the decoder generates, its logits differ from the bf16-cache decoder's (the switch is not ignored), and after
    generate every written cache row is a fixed point of dq(q(.)); rows never written are still zero."""
    from videotgb_amd import ops
    from videotgb_amd.decode import GreedyDecoder
    lm = _llama(4, dtype)
    B, P, N = 3, 9, 6
    emb = (torch.randn(B, P, 32, generator=torch.Generator().manual_seed(4)) * 0.5).to(dtype)
    dec8, dec16 = GreedyDecoder(lm, fused=False, kv_cache="fp8"), GreedyDecoder(lm, fused=False)
    assert dec8.kv_cache == "fp8" and dec16.kv_cache == "bf16"
    (ids8, rec8), (ids16, rec16) = _first_logits(dec8, emb, N), _first_logits(dec16, emb, N)
    assert ids8.shape == (B, N) and len(rec8) == N
    assert not torch.equal(rec8[0], rec16[0]) and not torch.equal(rec8[1], rec16[1])
    (st,) = dec8.graphs.values()
    assert st["attn"] is None and "kc8" not in st
    for cache in st["kc"] + st["vc"]:
        written = cache[:, :, : P + N - 1]
        assert written.float().abs().sum() > 0 and torch.equal(ops.fp8_kv_round(written), written)
        assert not cache[:, :, P + N - 1:].any()
    (st16,) = dec16.graphs.values()
    assert not torch.equal(ops.fp8_kv_round(st16["kc"][0]), st16["kc"][0])           # (the bf16 cache is not such a fixed point)
    assert GreedyDecoder(lm, fused=False, kv_cache="fp8").generate(emb, N, use_graph=False).tolist() == ids8.tolist()


def test_padded_prompts_and_both_fp8_modes_together_on_the_torch_path():
    from videotgb_amd.decode import GreedyDecoder
    lm = _llama(5, torch.bfloat16)
    emb = (torch.randn(2, 7, 32, generator=torch.Generator().manual_seed(5)) * 0.5).bfloat16()
    am = torch.ones(2, 7, dtype=torch.long)
    am[0, :3] = 0
    dec = GreedyDecoder(lm, fused=False, weights="fp8", kv_cache="fp8")
    assert dec.weights == "fp8" and dec.kv_cache == "fp8"
    assert dec.generate(emb, 4, use_graph=False, attention_mask=am).shape == (2, 4)


def test_bad_models_and_the_t5_decoder():
    from transformers import T5Config, T5ForConditionalGeneration
    from videotgb_amd.decode import GreedyDecoder, T5GreedyDecoder, make_decoder
    with pytest.raises(ValueError):
        GreedyDecoder(_llama(6), kv_cache="fp8")                                    # an fp32 model on the fused path
    with pytest.raises(ValueError):
        GreedyDecoder(_llama(6, torch.float16), fused=False, kv_cache="fp8")
    lm = _llama(6, torch.bfloat16)
    assert make_decoder(lm, kv_cache="fp8").kv_cache == "fp8" and make_decoder(lm).kv_cache == "bf16"
    t5 = T5ForConditionalGeneration(T5Config(vocab_size=50, d_model=32, d_kv=8, d_ff=64, num_layers=1, num_decoder_layers=1, num_heads=2,
                                             feed_forward_proj="gated-gelu", decoder_start_token_id=0, pad_token_id=0, eos_token_id=1))
    with pytest.raises(NotImplementedError, match="kv_cache='fp8' is implemented for the Llama decoder only"):
        T5GreedyDecoder(t5, kv_cache="fp8")
    with pytest.raises(NotImplementedError):
        make_decoder(t5, kv_cache="fp8")
    with pytest.raises(ValueError):
        T5GreedyDecoder(t5, kv_cache="int8")
    assert T5GreedyDecoder(t5).kv_cache == "bf16"


def test_decoder_for_follows_the_owners_kv_cache(monkeypatch):
    from videotgb_amd import decode
    lm = _llama(7, torch.bfloat16)
    owner = types.SimpleNamespace()
    d0 = decode.decoder_for(owner, lm)
    assert d0.kv_cache == "bf16" and decode.decoder_for(owner, lm) is d0
    owner.kv_cache = "fp8"
    d1 = decode.decoder_for(owner, lm)
    assert d1 is not d0 and d1.kv_cache == "fp8" and d1.weights == "bf16" and decode.decoder_for(owner, lm) is d1
    owner.decode_weights = "fp8"
    d2 = decode.decoder_for(owner, lm)
    assert d2 is not d1 and d2.kv_cache == "fp8" and d2.weights == "fp8" and decode.decoder_for(owner, lm) is d2
    owner.kv_cache = "bf16"
    d3 = decode.decoder_for(owner, lm)
    assert d3 is not d2 and d3.kv_cache == "bf16" and d3.weights == "fp8"
    owner.kv_cache = "int4"
    with pytest.raises(ValueError):
        decode.decoder_for(owner, lm)
    # the default mode keeps calling make_decoder with the positional lm alone
    calls = []

    def one_argument(lm_):
        calls.append(lm_)
        return types.SimpleNamespace(lm=lm_, key=decode.weights_key(lm_))

    monkeypatch.setattr(decode, "make_decoder", one_argument)
    fresh = types.SimpleNamespace(kv_cache="bf16", decode_weights="bf16")
    dec = decode.decoder_for(fresh, lm)
    assert calls == [lm] and decode.decoder_for(fresh, lm) is dec and calls == [lm]


def test_public_constructors_validate_before_loading_anything(tmp_path):
    from transformers import T5Config, T5ForConditionalGeneration
    from videotgb_amd import builder_utils, decode, models, modules, synth
    lm = _llama(9, torch.bfloat16)
    cfg = synth.tiny_cfg("instructblip")
    with pytest.raises(ValueError, match="kv_cache"):
        models.LSTP.from_cfg(cfg, "cpu", language_model=lm, kv_cache="fp4")
    with pytest.raises(ValueError, match="kv_cache"):
        models.LSTP(str(tmp_path / "no-such-instructblip"), "cpu", kv_cache="fp4")       # (before the config is looked for)
    with pytest.raises(ValueError, match="kv_cache"):
        builder_utils.load_pretrained_model(str(tmp_path / "x.ckpt"), str(tmp_path / "instructblip"), None, "cpu", load_processors=False, kv_cache="int8")
    for cls in (modules.LSTPModule, modules.LSTPBlip2Module):
        with pytest.raises(ValueError, match="kv_cache"):
            cls(str(tmp_path / "m"), str(tmp_path / "s"), str(tmp_path / "r"), kv_cache="int8")
    t5 = T5ForConditionalGeneration(T5Config(vocab_size=50, d_model=32, d_kv=8, d_ff=64, num_layers=1, num_decoder_layers=1, num_heads=2,
                                             feed_forward_proj="gated-gelu", decoder_start_token_id=0, pad_token_id=0, eos_token_id=1))
    with pytest.raises(NotImplementedError):
        models.LSTP_blip2.from_cfg(synth.tiny_cfg("blip2"), "cpu", language_model=t5, kv_cache="fp8")
    m = models.LSTP.from_cfg(cfg, "cpu", language_model=lm, kv_cache="fp8")
    assert m.kv_cache == "fp8" and m.decode_weights == "bf16" and models.LSTP.from_cfg(cfg, "cpu", language_model=lm).kv_cache == "bf16"
    assert decode.decoder_for(m, lm).kv_cache == "fp8"
