"""The opt-in fp8 weight stream of the Llama graph decoder (decode_weights="fp8"), the part that needs no GPU: the quantised format
(ops.quantize_fp8_rows: per-row power-of-two scale, OCP e4m3 codes), the decoder's identity with HF generate on the dequantised model,
the decoder accessor and the argument checks of the new library entries."""
import copy
import ctypes as C
import types

import pytest
import torch


def _rows(seed=0, n=256, k=512, std=1.0):
    return torch.randn(n, k, generator=torch.Generator().manual_seed(seed)) * std


# ------------------------------------------------------------------------------------------------------------- the recipe
@pytest.mark.parametrize("std", [1.0, 0.02, 37.0])
def test_quantised_rows_are_bf16_numbers_with_power_of_two_scales(std):
    """``row max of |q|``: the scaled amax lies in (224, 448] by the choice of e, but e4m3 has no number between 224 and 240, so a scaled amax
    in (224, 232] rounds DOWN to 224: the codes' row maximum is >= 224 (> 224 holds for the scaled weights before rounding, asserted too)."""
    from videotgb_amd import ops
    w = _rows(1, std=std).bfloat16()
    q, scale = ops.quantize_fp8_rows(w)
    assert q.dtype == torch.float8_e4m3fn and q.shape == w.shape and scale.dtype == torch.float32 and scale.shape == (w.shape[0],)
    dq = ops.dequantize_fp8_rows(q, scale, torch.float32)
    assert torch.equal(dq.bfloat16().float(), dq)                                   # q * scale is exactly a bf16 number
    assert torch.equal(ops.dequantize_fp8_rows(q, scale).float(), dq)
    qf = q.float()
    assert not torch.isnan(qf).any() and qf.abs().max().item() <= 448
    m, e = torch.frexp(scale)
    assert torch.equal(m, torch.full_like(m, 0.5))                                  # scale = 2^(e - 1)
    scaled = w.float() / scale[:, None]                                             # exact (power of two)
    amax = scaled.abs().amax(1)
    assert (amax > 224).all() and (amax <= 448).all()                               # e is the SMALLEST exponent that fits
    assert (qf.abs().amax(1) >= 224).all()
    # element error: half an ulp of 3 mantissa bits wherever the scaled weight is in e4m3's normal range
    normal = scaled.abs() >= 2.0 ** -6
    assert normal.float().mean() > 0.9
    assert ((qf - scaled).abs() <= 2.0 ** -4 * scaled.abs())[normal].all()
    rel = ((dq - w.float()).pow(2).mean().sqrt() / w.float().pow(2).mean().sqrt()).item()
    print(f"std {std}: weight rel-RMS {rel:.4f}")
    assert 0.015 < rel < 0.04                                                       # (3 mantissa bits: 2^-4 / sqrt(3) = 3.6 % at worst)


def test_documented_exponents_and_bad_values():
    from videotgb_amd import ops
    w = torch.zeros(8, 64)
    w[1, 3] = 448.0                     # e = 0
    w[2, 5] = -448.0 * 2.0 ** 7         # e = 7
    w[3, 0] = 448.0 * 2.0 ** -20        # e = -20
    w[4, 9] = 449.0                     # just above: e = 1
    w[5, 1] = 224.0                     # 224 * 2 = 448 fits: e = -1
    w[6, 2] = 1.0                       # 2^8 = 256 <= 448 < 2^9: e = -8
    w[7, 4] = 2.0 ** -30
    q, scale = ops.quantize_fp8_rows(w)
    assert scale.tolist() == [1.0, 1.0, 2.0 ** 7, 2.0 ** -20, 2.0, 0.5, 2.0 ** -8, 2.0 ** -38]
    assert torch.equal(q[0].float(), torch.zeros(64))                               # a zero row: e = 0, codes 0
    assert q[1, 3].float().item() == 448.0 and q[2, 5].float().item() == -448.0 and q[3, 0].float().item() == 448.0
    assert q[4, 9].float().item() == 224.0 and q[5, 1].float().item() == 448.0 and q[6, 2].float().item() == 256.0
    assert torch.equal(ops.dequantize_fp8_rows(q, scale, torch.float32)[[1, 2, 3, 5, 6, 7]], w[[1, 2, 3, 5, 6, 7]])
    for bad in (float("inf"), float("-inf"), float("nan")):
        w2 = _rows(2, 4, 64)
        w2[2, 7] = bad
        with pytest.raises(ValueError):
            ops.quantize_fp8_rows(w2)
        with pytest.raises(ValueError):
            ops.quantize_fp8_rows(w2.bfloat16())


def test_rounding_is_to_nearest_even_including_subnormal_codes():
    from videotgb_amd import ops
    w = torch.zeros(1, 64)
    w[0, 0] = 448.0                                                                 # pins e = 0
    vals = [17.0, 19.0, 18.0, 2.0 ** -6 + 2.0 ** -10, 2.0 ** -9 * 2.5, 2.0 ** -9 * 3.5, 2.0 ** -10, 2.0 ** -10 * 1.01, -2.0 ** -9 * 0.4]
    want = [16.0, 20.0, 18.0, 2.0 ** -6, 2.0 ** -9 * 2, 2.0 ** -9 * 4, 0.0, 2.0 ** -9, -0.0]      # ties to even: 17 -> 16, 19 -> 20 (spacing 2)
    w[0, 1:1 + len(vals)] = torch.tensor(vals)
    q, scale = ops.quantize_fp8_rows(w)
    assert scale.item() == 1.0 and q[0, 1:1 + len(vals)].float().tolist() == want


# ------------------------------------------------------------------------------------------------------------- the decoder
PROJ = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


def _llama(seed=3, dtype=torch.float32):
    from videotgb_amd import llm
    return llm.build_llama("tiny", dtype, "cpu", seed=seed, num_hidden_layers=3, num_key_value_heads=1)


def _dequantised_copy(lm):
    """A deep copy of ``lm`` whose seven projection weights per layer and lm_head are q * scale (quantised from the weights' bf16 cast)."""
    from videotgb_amd import ops
    ref = copy.deepcopy(lm)
    with torch.no_grad():
        mods = [getattr(part, n) for l in ref.model.layers for part in (l.self_attn, l.mlp) for n in PROJ if hasattr(part, n)] + [ref.lm_head]
        assert len(mods) == 7 * len(ref.model.layers) + 1
        for m in mods:
            m.weight.copy_(ops.dequantize_fp8_rows(*ops.quantize_fp8_rows(m.weight.bfloat16()), dtype=m.weight.dtype))
    return ref


def test_fp8_decoder_ids_equal_hf_generate_on_the_dequantised_model_cpu():
    """fp32 arithmetic, as tests/test_decode.py: the helper model is fp32, so the decoder (torch path, ``fused=False``) quantises from the
    bf16 cast of its weights, and so does the reference copy -- the ids must be HF generate's on that copy, token for token.  For at
    least one seed they differ from the unquantised model's (otherwise the comparison would show nothing)."""
    from videotgb_amd.decode import GreedyDecoder
    differs = 0
    for seed in (3, 4, 5):
        lm = _llama(seed)
        emb = torch.randn(3, 9, 32, generator=torch.Generator().manual_seed(seed)) * 0.5
        am = torch.ones(3, 9, dtype=torch.long)
        ref = _dequantised_copy(lm).generate(inputs_embeds=emb, attention_mask=am, do_sample=False, max_new_tokens=12, min_new_tokens=12, use_cache=True)
        dec = GreedyDecoder(lm, fused=False, weights="fp8")
        out = dec.generate(emb, 12, use_graph=False)
        assert out.tolist() == ref.tolist(), seed
        plain = lm.generate(inputs_embeds=emb, attention_mask=am, do_sample=False, max_new_tokens=12, min_new_tokens=12, use_cache=True)
        assert GreedyDecoder(lm, fused=False).generate(emb, 12, use_graph=False).tolist() == plain.tolist()      # the default mode is untouched
        differs += plain.tolist() != ref.tolist()
        # embeddings and norms are the model's own; the held matrices are the dequantised ones
        assert dec.layers[0][0] is lm.model.layers[0].input_layernorm.weight
        assert not torch.equal(dec.head_w, lm.lm_head.weight)
    assert differs >= 1


def test_fp8_decoder_on_a_bf16_cpu_model_holds_the_dequantised_weights():
    from videotgb_amd import ops
    from videotgb_amd.decode import GreedyDecoder
    lm = _llama(6, torch.bfloat16)
    dec = GreedyDecoder(lm, weights="fp8")
    l0 = lm.model.layers[0]
    wqkv = torch.cat([l0.self_attn.q_proj.weight, l0.self_attn.k_proj.weight, l0.self_attn.v_proj.weight], 0)
    assert dec.layers[0][1].dtype == torch.bfloat16 and torch.equal(dec.layers[0][1], ops.dequantize_fp8_rows(*ops.quantize_fp8_rows(wqkv)))
    assert torch.equal(dec.head_w, ops.dequantize_fp8_rows(*ops.quantize_fp8_rows(lm.lm_head.weight)))
    emb = (torch.randn(2, 5, 32, generator=torch.Generator().manual_seed(0)) * 0.5).bfloat16()
    assert dec.generate(emb, 4, use_graph=False).shape == (2, 4)


# ------------------------------------------------------------------------------------------------------------- accessor and arguments
def test_decoder_for_follows_the_owners_decode_weights(monkeypatch):
    from videotgb_amd import decode
    lm = _llama(7, torch.bfloat16)
    owner = types.SimpleNamespace()
    d0 = decode.decoder_for(owner, lm)
    assert d0.weights == "bf16" and decode.decoder_for(owner, lm) is d0
    owner.decode_weights = "fp8"
    d1 = decode.decoder_for(owner, lm)
    assert d1 is not d0 and d1.weights == "fp8" and decode.decoder_for(owner, lm) is d1
    owner.decode_weights = "bf16"
    d2 = decode.decoder_for(owner, lm)
    assert d2 is not d1 and d2.weights == "bf16"
    owner.decode_weights = "int4"
    with pytest.raises(ValueError):
        decode.decoder_for(owner, lm)
    # the default mode keeps calling make_decoder with one argument
    calls = []

    def one_argument(lm_):
        calls.append(lm_)
        return types.SimpleNamespace(lm=lm_, key=decode.weights_key(lm_))

    monkeypatch.setattr(decode, "make_decoder", one_argument)
    fresh = types.SimpleNamespace()
    dec = decode.decoder_for(fresh, lm)
    assert calls == [lm] and decode.decoder_for(fresh, lm) is dec and calls == [lm]


def test_fp8_decoder_retires_with_the_weights():
    """After an in-place update the accessor builds a new fp8 decoder, whose matrices are re-quantised from the new weights."""
    from videotgb_amd import decode, ops
    lm = _llama(8, torch.bfloat16)
    owner = types.SimpleNamespace(decode_weights="fp8")
    d0 = decode.decoder_for(owner, lm)
    with torch.no_grad():
        lm.lm_head.weight.mul_(1.5).add_(0.01)
    d1 = decode.decoder_for(owner, lm)
    assert d1 is not d0 and d1.weights == "fp8"
    assert torch.equal(d1.head_w, ops.dequantize_fp8_rows(*ops.quantize_fp8_rows(lm.lm_head.weight))) and not torch.equal(d1.head_w, d0.head_w)


def test_bad_modes_raise():
    from videotgb_amd import decode, models, synth
    from videotgb_amd.decode import GreedyDecoder, T5GreedyDecoder, make_decoder
    from transformers import T5Config, T5ForConditionalGeneration
    lm = _llama(9, torch.bfloat16)
    for bad in ("int8", "FP8", None, 8):
        with pytest.raises(ValueError):
            GreedyDecoder(lm, weights=bad)
        with pytest.raises(ValueError):
            make_decoder(lm, weights=bad)
    with pytest.raises(ValueError):
        GreedyDecoder(_llama(9), weights="fp8")                                     # an fp32 model on the fused path
    with pytest.raises(ValueError):
        GreedyDecoder(_llama(9, torch.float16), fused=False, weights="fp8")
    assert make_decoder(lm, weights="fp8").weights == "fp8" and make_decoder(lm).weights == "bf16"
    t5 = T5ForConditionalGeneration(T5Config(vocab_size=50, d_model=32, d_kv=8, d_ff=64, num_layers=1, num_decoder_layers=1, num_heads=2,
                                             feed_forward_proj="gated-gelu", decoder_start_token_id=0, pad_token_id=0, eos_token_id=1))
    with pytest.raises(NotImplementedError):
        T5GreedyDecoder(t5, weights="fp8")
    with pytest.raises(NotImplementedError):
        make_decoder(t5, weights="fp8")
    with pytest.raises(ValueError):
        T5GreedyDecoder(t5, weights="int8")
    assert T5GreedyDecoder(t5).weights == "bf16"
    # the public switch validates at construction
    cfg = synth.tiny_cfg("instructblip")
    with pytest.raises(ValueError):
        models.LSTP.from_cfg(cfg, "cpu", language_model=lm, decode_weights="fp4")
    with pytest.raises(NotImplementedError):
        models.LSTP_blip2.from_cfg(synth.tiny_cfg("blip2"), "cpu", language_model=t5, decode_weights="fp8")
    m = models.LSTP.from_cfg(cfg, "cpu", language_model=lm, decode_weights="fp8")
    assert m.decode_weights == "fp8" and models.LSTP.from_cfg(cfg, "cpu", language_model=lm).decode_weights == "bf16"
    assert decode.decoder_for(m, lm).weights == "fp8"


# ------------------------------------------------------------------------------------------------------------- ABI
def test_fp8_entries_reject_bad_arguments_on_the_host():
    from videotgb_amd import _lib as L
    lib = L.lib()
    EINVAL = -1      # VTGB_EINVAL
    for n, k in ((4096, 4096), (100, 128), (32000, 4096), (640, 448)):
        assert lib.vtgb_pack_skinny_weight_fp8_bytes(n, k) * 2 == lib.vtgb_pack_skinny_weight_bytes(n, k) > 0
    assert lib.vtgb_pack_skinny_weight_fp8_bytes(128, 100) == 0 and lib.vtgb_pack_skinny_weight_fp8_bytes(0, 64) == 0
    buf = (C.c_char * 65536)()
    p = C.addressof(buf)
    assert lib.vtgb_pack_skinny_weight_fp8(None, 64, 16, 64, p, p, None) != 0
    assert lib.vtgb_pack_skinny_weight_fp8(p, 64, 16, 64, None, p, None) != 0
    assert lib.vtgb_pack_skinny_weight_fp8(p, 64, 16, 64, p, None, None) != 0
    assert lib.vtgb_pack_skinny_weight_fp8(p, 64, 16, 100, p, p, None) != 0          # K not a multiple of 64

    def args(x=p, w=p, out=p, tiled=1):
        return L.GemmSkinnyArgs(4, 16, 64, 0, x, 64, w, 64, out, 16, L.BF16, tiled, None, 0, 0)
    for a, scale in ((args(x=None), p), (args(w=None), p), (args(out=None), p), (args(), None), (args(tiled=0), p)):
        assert lib.vtgb_gemm_skinny_fp8(C.byref(a), scale, None) == EINVAL, lib.vtgb_last_error()
    assert lib.vtgb_gemm_skinny_fp8(None, p, None) == EINVAL
    assert lib.vtgb_version() == 601
