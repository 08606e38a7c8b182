"""The opt-in MXFP4 weight stream of the Llama graph decoder (decode_weights="mxfp4"), the part that needs no GPU: the format
(ops.quantize_mxfp4_rows: OCP MX v1.0 -- one E8M0 scale per 32 weights along K, e2m1 codes), its two properties (code * 2^e is exactly a
bf16 number; re-quantising the dequantised matrix returns the same codes and scale bytes), the decoder's identity with HF generate on
the dequantised model, the decoder accessor and the argument checks of the new library entries."""
import copy
import ctypes as C
import types

import pytest
import torch

E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


def _rows(seed=0, n=256, k=512, std=1.0):
    return torch.randn(n, k, generator=torch.Generator().manual_seed(seed)) * std


def _unpack(codes):
    """codes [N, K / 2] -> one code per weight [N, K] (the lower k in the low nibble)."""
    return torch.stack((codes & 15, codes >> 4), dim=2).view(codes.shape[0], -1)


# ------------------------------------------------------------------------------------------------------------- the recipe
@pytest.mark.parametrize("std", [1.0, 0.02, 37.0])
def test_dequantised_rows_are_bf16_numbers_and_requantise_to_themselves(std):
    from videotgb_amd import ops
    w = _rows(1, std=std).bfloat16()
    codes, scales = ops.quantize_mxfp4_rows(w)
    N, K = w.shape
    assert codes.dtype == torch.uint8 and codes.shape == (N, K // 2) and scales.dtype == torch.uint8 and scales.shape == (N, K // 32)
    dq = ops.dequantize_mxfp4_rows(codes, scales, torch.float32)
    assert torch.isfinite(dq).all() and torch.equal(dq.bfloat16().float(), dq)      # exactness: code * 2^e is a bf16 number
    assert torch.equal(ops.dequantize_mxfp4_rows(codes, scales).float(), dq)
    nz = dq[dq != 0].abs()
    assert nz.min().item() >= 2.0 ** -126                                            # ... and a normal one
    e = scales.int() - 127
    assert e.min().item() >= -120 and e.max().item() <= 125                          # the clamp
    c = _unpack(codes)
    assert (c & 7).max().item() == 7                                                 # no code beyond 6 (three magnitude bits: 7 = 6.0) ...
    scaled = w.float().view(N, K // 32, 32) * torch.ldexp(torch.ones(()), -e)[:, :, None]
    amax = scaled.abs().amax(2)
    assert (amax >= 4).all() and (amax < 8).all()                                    # e = floor(log2(amax)) - 2
    assert dq.view(N, K // 32, 32).abs().amax(2).div(torch.ldexp(torch.ones(()), e)).max().item() <= 6      # ... and none past +-6 * 2^e
    # idempotence: the decoder re-packs from its dequantised copy
    codes2, scales2 = ops.quantize_mxfp4_rows(dq.bfloat16())
    assert torch.equal(codes2, codes) and torch.equal(scales2, scales)
    # the element error: at most half a grid step (1 between 4 and 6 and in saturation, where the scaled weight is < 8)
    assert ((dq.view(N, K // 32, 32) * torch.ldexp(torch.ones(()), -e)[:, :, None] - scaled).abs() <= 1.0 + (scaled.abs() > 6).float()).all()
    rel = ((dq - w.float()).pow(2).mean().sqrt() / w.float().pow(2).mean().sqrt()).item()
    print(f"std {std}: weight rel-RMS {rel:.4f}")
    assert 0.08 < rel < 0.15                                                         # (one mantissa bit: 2^-2 / sqrt(3) = 14.4 % at worst)


def test_documented_exponents():
    from videotgb_amd import ops
    w = torch.zeros(10, 64)
    w[1, 3] = 4.0                        # floor(log2) = 2: e = 0, code 4.0
    w[2, 5] = -6.0                       # e = 0, code -6.0
    w[3, 0] = 7.9 * 2.0 ** 11            # still below 8 * 2^11: e = 11, and 7.9 saturates to 6
    w[4, 9] = 8.0 * 2.0 ** 11            # e = 12, code 4.0
    w[5, 40] = 7.9 * 2.0 ** -30          # second block of the row: e = -30; the first block is all zero
    w[6, 1] = 8.0 * 2.0 ** -30           # e = -29
    w[7, :32] = 2.0 ** -130              # bf16 subnormals: floor(log2) - 2 = -132, clamped to -120; every element rounds to 0
    w[8, 2] = 1.5 * 2.0 ** -121          # under the lower clamp with a non-zero code: 1.5 * 2^-121 * 2^120 = 0.75 -> 1.0 (tie to the even code)
    w[9, 7] = 1.75 * 2.0 ** 127          # the largest exponent, floor(log2) = 127: e = 125 (the upper clamp), 1.75 * 4 = 7 saturates to 6
    for ww in (w, w.bfloat16()):
        codes, scales = ops.quantize_mxfp4_rows(ww)
        e = (scales.int() - 127).tolist()
        assert e[0] == [0, 0] and not codes[0].any()                                 # all-zero blocks: e = 0 (byte 127), codes 0
        assert e[1] == [0, 0] and e[2] == [0, 0] and e[3] == [11, 0] and e[4] == [12, 0]
        assert e[5] == [0, -30] and e[6] == [-29, 0] and e[7] == [-120, 0] and e[8] == [-120, 0] and e[9] == [125, 0]
        dq = ops.dequantize_mxfp4_rows(codes, scales, torch.float32)
        assert dq[1, 3].item() == 4.0 and dq[2, 5].item() == -6.0 and dq[3, 0].item() == 6.0 * 2.0 ** 11 and dq[4, 9].item() == 4.0 * 2.0 ** 12
        assert dq[5, 40].item() == 6.0 * 2.0 ** -30 and dq[6, 1].item() == 4.0 * 2.0 ** -29
        assert not codes[7].any() and not dq[7].any()
        assert dq[8, 2].item() == 2.0 ** -120 and dq[9, 7].item() == 6.0 * 2.0 ** 125 and torch.isfinite(dq).all()
        assert torch.equal(dq.bfloat16().float(), dq)
        assert (dq != 0).sum().item() == 8


def test_rounding_is_to_nearest_with_ties_to_the_even_code_and_saturates():
    from videotgb_amd import ops
    # (value, expected e2m1 magnitude) under e = 0, pinned by an element of 4.0: every midpoint of the grid, a value on either side of
    # each, and the saturating range (6, 8)
    cases = [(0.25, 0.0), (0.75, 1.0), (1.25, 1.0), (1.75, 2.0), (2.5, 2.0), (3.5, 4.0), (5.0, 4.0),
             (0.2, 0.0), (0.3, 0.5), (0.7, 0.5), (0.8, 1.0), (1.2, 1.0), (1.3, 1.5), (1.7, 1.5), (1.8, 2.0), (2.4, 2.0), (2.6, 3.0), (3.4, 3.0),
             (3.6, 4.0), (4.9, 4.0), (5.1, 6.0), (6.0, 6.0), (6.5, 6.0), (7.0, 6.0), (7.75, 6.0), (0.0, 0.0), (0.5, 0.5), (1.5, 1.5), (3.0, 3.0)]
    w = torch.zeros(2, 64)
    w[:, 31] = 4.0
    vals = torch.tensor([c[0] for c in cases])
    w[0, :len(cases)] = vals
    w[1, :len(cases)] = -vals
    w[1, 31] = 7.75                                                                  # a block whose amax itself saturates: e stays 0
    codes, scales = ops.quantize_mxfp4_rows(w)
    assert scales[:, 0].tolist() == [127, 127]
    c = _unpack(codes)
    want = [E2M1.index(m) for _, m in cases]
    assert c[0, :len(cases)].tolist() == want
    assert c[1, :len(cases)].tolist() == [8 | x for x in want]                       # the sign bit is the weight's own (-0.0 and -0.2 keep it)
    assert c[1, 31].item() == 7
    dq = ops.dequantize_mxfp4_rows(codes, scales, torch.float32)
    assert dq[0, :len(cases)].tolist() == [m for _, m in cases] and dq[1, :len(cases)].tolist() == [-m for _, m in cases]
    # the same grid under another scale: bf16-exact multiples
    codes2, scales2 = ops.quantize_mxfp4_rows((w * 2.0 ** -9).bfloat16())
    assert torch.equal(codes2, codes) and scales2[:, 0].tolist() == [118, 118]


def test_nibble_order_and_block_boundaries():
    from videotgb_amd import ops
    w = torch.zeros(1, 128)
    w[0, 0], w[0, 1], w[0, 2] = 4.0, -1.0, 0.5                                       # block 0, e = 0
    w[0, 32], w[0, 33] = 64.0, 16.0                                                  # block 1, e = 4: codes 4.0, 1.0
    w[0, 127] = -3.0                                                                 # block 3, e = -1: code -6.0
    codes, scales = ops.quantize_mxfp4_rows(w)
    assert scales.tolist() == [[127, 131, 127, 126]]
    assert codes[0, 0].item() == (6 | (8 | 2) << 4) and codes[0, 1].item() == 1      # k = 0 in the low nibble, k = 1 in the high one
    assert codes[0, 16].item() == (6 | 2 << 4) and codes[0, 63].item() == (8 | 7) << 4
    assert torch.equal(ops.dequantize_mxfp4_rows(codes, scales, torch.float32), w)


def test_bad_values_and_shapes_raise():
    from videotgb_amd import ops
    for bad in (float("inf"), float("-inf"), float("nan")):
        w2 = _rows(2, 4, 64)
        w2[2, 7] = bad
        with pytest.raises(ValueError):
            ops.quantize_mxfp4_rows(w2)
        with pytest.raises(ValueError):
            ops.quantize_mxfp4_rows(w2.bfloat16())
    with pytest.raises(ValueError):
        ops.quantize_mxfp4_rows(torch.zeros(64))
    with pytest.raises(ValueError):
        ops.quantize_mxfp4_rows(torch.zeros(2, 2, 64))
    for k in (32, 96, 100):
        with pytest.raises(NotImplementedError):
            ops.quantize_mxfp4_rows(torch.zeros(4, k))


# ------------------------------------------------------------------------------------------------------------- the decoder
PROJ = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


def _llama(seed=3, dtype=torch.float32):
    """hidden 64 / intermediate 128: every K is a multiple of the format's 64."""
    from videotgb_amd import llm
    return llm.build_llama("tiny", dtype, "cpu", seed=seed, num_hidden_layers=3, num_key_value_heads=1, hidden_size=64, intermediate_size=128)


def _dq(w):
    from videotgb_amd import ops
    return ops.dequantize_mxfp4_rows(*ops.quantize_mxfp4_rows(w.bfloat16()), dtype=w.dtype)


def _dequantised_copy(lm):
    """A deep copy of ``lm`` whose seven projection weights per layer and lm_head are code * 2^e."""
    ref = copy.deepcopy(lm)
    with torch.no_grad():
        mods = [getattr(part, n) for l in ref.model.layers for part in (l.self_attn, l.mlp) for n in PROJ if hasattr(part, n)] + [ref.lm_head]
        assert len(mods) == 7 * len(ref.model.layers) + 1
        for m in mods:
            m.weight.copy_(_dq(m.weight))
    return ref


def test_mxfp4_decoder_ids_equal_hf_generate_on_the_dequantised_model_cpu():
    """A bf16 Llama on the CPU, unfused (the torch statement of the model): the ids are HF generate's on a copy of the model that carries the
    dequantised weights, token for token; the decoder's matrices are those weights; the default mode is untouched."""
    from videotgb_amd.decode import GreedyDecoder
    differs = 0
    for seed in (3, 4, 5):
        lm = _llama(seed, torch.bfloat16)
        with torch.no_grad():      # (N(0, 0.02) leaves near-uniform logits, which bf16 rounding in a different order of operations -- HF's three
            lm.lm_head.weight.mul_(30.0)      # projections against the decoder's fused q|k|v, in the DEFAULT mode too -- turns into other ids)
            lm.model.embed_tokens.weight.mul_(50.0)
        H = lm.config.hidden_size
        emb = (torch.randn(3, 9, H, generator=torch.Generator().manual_seed(seed)) * 0.5).bfloat16()
        am = torch.ones(3, 9, dtype=torch.long)
        kw = dict(inputs_embeds=emb, attention_mask=am, do_sample=False, max_new_tokens=12, min_new_tokens=12, use_cache=True)
        ref = _dequantised_copy(lm).generate(**kw)
        dec = GreedyDecoder(lm, fused=False, weights="mxfp4")
        assert dec.weights == "mxfp4"
        out = dec.generate(emb, 12, use_graph=False)
        assert out.tolist() == ref.tolist(), seed
        assert out.tolist() == GreedyDecoder(_dequantised_copy(lm), fused=False).generate(emb, 12, use_graph=False).tolist()      # the same arithmetic: always
        plain = lm.generate(**kw)
        assert GreedyDecoder(lm, fused=False).generate(emb, 12, use_graph=False).tolist() == plain.tolist()
        differs += plain.tolist() != ref.tolist()
        l0 = lm.model.layers[0]
        wqkv = torch.cat([l0.self_attn.q_proj.weight, l0.self_attn.k_proj.weight, l0.self_attn.v_proj.weight], 0)
        assert dec.layers[0][0] is l0.input_layernorm.weight                         # embeddings and norms are the model's own
        assert dec.layers[0][1].dtype == torch.bfloat16 and torch.equal(dec.layers[0][1], _dq(wqkv)) and not torch.equal(dec.layers[0][1], wqkv)
        assert torch.equal(dec.layers[0][5], _dq(l0.mlp.down_proj.weight))
        assert torch.equal(dec.head_w, _dq(lm.lm_head.weight)) and not torch.equal(dec.head_w, lm.lm_head.weight)
    assert differs >= 1


def test_mxfp4_decoder_on_an_fp32_model_quantises_from_the_bf16_cast():
    from videotgb_amd.decode import GreedyDecoder
    lm = _llama(6)
    dec = GreedyDecoder(lm, fused=False, weights="mxfp4")
    assert dec.head_w.dtype == torch.float32 and torch.equal(dec.head_w, _dq(lm.lm_head.weight))
    emb = torch.randn(2, 5, lm.config.hidden_size, generator=torch.Generator().manual_seed(0)) * 0.5
    ref = _dequantised_copy(lm).generate(inputs_embeds=emb, attention_mask=torch.ones(2, 5, dtype=torch.long), do_sample=False, max_new_tokens=6,
                                         min_new_tokens=6, use_cache=True)
    assert dec.generate(emb, 6, use_graph=False).tolist() == ref.tolist()


# ------------------------------------------------------------------------------------------------------------- accessor and arguments
def test_decoder_for_follows_the_owners_mode_and_retires_with_the_weights():
    from videotgb_amd import decode
    lm = _llama(7, torch.bfloat16)
    owner = types.SimpleNamespace()
    d0 = decode.decoder_for(owner, lm)
    assert d0.weights == "bf16"
    owner.decode_weights = "mxfp4"
    d1 = decode.decoder_for(owner, lm)
    assert d1 is not d0 and d1.weights == "mxfp4" and decode.decoder_for(owner, lm) is d1
    owner.decode_weights = "fp8"
    d2 = decode.decoder_for(owner, lm)
    assert d2 is not d1 and d2.weights == "fp8"
    owner.decode_weights = "mxfp4"
    d3 = decode.decoder_for(owner, lm)
    assert d3 is not d2 and d3.weights == "mxfp4"
    with torch.no_grad():
        lm.lm_head.weight.mul_(1.5).add_(0.01)
    d4 = decode.decoder_for(owner, lm)
    assert d4 is not d3 and d4.weights == "mxfp4"
    assert torch.equal(d4.head_w, _dq(lm.lm_head.weight)) and not torch.equal(d4.head_w, d3.head_w)
    owner.kv_cache = "fp8"
    d5 = decode.decoder_for(owner, lm)
    assert d5 is not d4 and d5.weights == "mxfp4" and d5.kv_cache == "fp8"


def test_modes_that_are_accepted_and_modes_that_raise():
    from videotgb_amd import decode, models, synth
    from videotgb_amd.decode import GreedyDecoder, T5GreedyDecoder, make_decoder
    from transformers import T5Config, T5ForConditionalGeneration
    assert decode.MODES["decode_weights"] == ("bf16", "fp8", "mxfp4") and decode.check_mode("decode_weights", "mxfp4") == "mxfp4"
    lm = _llama(9, torch.bfloat16)
    for bad in ("fp4", "MXFP4", "mxfp8", "nvfp4"):
        with pytest.raises(ValueError):
            GreedyDecoder(lm, weights=bad)
    with pytest.raises(ValueError, match="decode_weights='mxfp4' needs a bf16 language model"):
        GreedyDecoder(_llama(9), weights="mxfp4")                                    # an fp32 model on the fused path
    with pytest.raises(ValueError, match="mxfp4"):
        GreedyDecoder(_llama(9, torch.float16), fused=False, weights="mxfp4")
    assert make_decoder(lm, weights="mxfp4").weights == "mxfp4"
    t5 = T5ForConditionalGeneration(T5Config(vocab_size=50, d_model=32, d_kv=8, d_ff=64, num_layers=1, num_decoder_layers=1, num_heads=2,
                                             feed_forward_proj="gated-gelu", decoder_start_token_id=0, pad_token_id=0, eos_token_id=1))
    with pytest.raises(NotImplementedError, match="decode_weights='mxfp4' is implemented for the Llama decoder only"):
        T5GreedyDecoder(t5, weights="mxfp4")
    with pytest.raises(NotImplementedError, match="mxfp4"):
        make_decoder(t5, weights="mxfp4")
    with pytest.raises(NotImplementedError, match="decode_weights='fp8'"):          # the message names the mode that was asked for
        T5GreedyDecoder(t5, weights="fp8")
    # the public switch
    cfg = synth.tiny_cfg("instructblip")
    m = models.LSTP.from_cfg(cfg, "cpu", language_model=lm, decode_weights="mxfp4")
    assert m.decode_weights == "mxfp4" and decode.decoder_for(m, lm).weights == "mxfp4"
    m2 = models.LSTP.from_cfg(cfg, "cpu", language_model=lm, decode_weights="mxfp4", kv_cache="fp8", beam_search="graph")
    assert (m2.decode_weights, m2.kv_cache, m2.beam_search) == ("mxfp4", "fp8", "graph")
    with pytest.raises(NotImplementedError, match="decode_weights='mxfp4'"):
        models.LSTP_blip2.from_cfg(synth.tiny_cfg("blip2"), "cpu", language_model=t5, decode_weights="mxfp4")


# ------------------------------------------------------------------------------------------------------------- ABI
def test_mxfp4_entries_reject_bad_arguments_on_the_host():
    from videotgb_amd import _lib as L
    lib = L.lib()
    EINVAL = -1      # VTGB_EINVAL
    for n, k in ((4096, 4096), (100, 128), (32000, 4096), (640, 448)):
        # per (128-row tile, k-tile): 4096 bytes of codes + 256 of scales against fp8's 8192
        assert lib.vtgb_pack_skinny_weight_mxfp4_bytes(n, k) == ((n + 127) // 128) * (k // 64) * (4096 + 256)
        assert lib.vtgb_pack_skinny_weight_mxfp4_bytes(n, k) * 32 == lib.vtgb_pack_skinny_weight_fp8_bytes(n, k) * 17 > 0
    assert lib.vtgb_pack_skinny_weight_mxfp4_bytes(128, 100) == 0 and lib.vtgb_pack_skinny_weight_mxfp4_bytes(0, 64) == 0
    assert lib.vtgb_pack_skinny_weight_mxfp4_bytes(128, 0) == 0 and lib.vtgb_pack_skinny_weight_mxfp4_bytes(-5, 64) == 0
    buf = (C.c_char * 65536)()
    p = C.addressof(buf)
    assert lib.vtgb_pack_skinny_weight_mxfp4(None, 64, 16, 64, p, None) == EINVAL
    assert lib.vtgb_pack_skinny_weight_mxfp4(p, 64, 16, 64, None, None) == EINVAL
    assert lib.vtgb_pack_skinny_weight_mxfp4(p, 64, 16, 100, p, None) == EINVAL      # K not a multiple of 64
    assert lib.vtgb_pack_skinny_weight_mxfp4(p, 60, 16, 64, p, None) == EINVAL       # row pitch below K
    assert lib.vtgb_pack_skinny_weight_mxfp4(p, 68, 16, 64, p, None) == EINVAL       # row pitch no multiple of 8
    assert lib.vtgb_pack_skinny_weight_mxfp4(p, 64, 0, 64, p, None) == EINVAL

    def args(x=p, w=p, out=p, tiled=1, M=4, K=64):
        return L.GemmSkinnyArgs(M, 16, K, 0, x, 64, w, 64, out, 16, L.BF16, tiled, None, 0, 0)
    for a in (args(x=None), args(w=None), args(out=None), args(tiled=0)):
        assert lib.vtgb_gemm_skinny_mxfp4(C.byref(a), None, None) == EINVAL, lib.vtgb_last_error()
        assert lib.vtgb_gemm_skinny_mxfp4(C.byref(a), p, None) == EINVAL
    assert lib.vtgb_gemm_skinny_mxfp4(None, None, None) == EINVAL
    assert lib.vtgb_gemm_skinny_mxfp4(C.byref(args(M=129)), None, None) not in (0, EINVAL)      # the shape checks are vtgb_gemm_skinny's, first
    assert lib.vtgb_gemm_skinny_mxfp4(C.byref(args(K=100)), None, None) not in (0, EINVAL)
    assert lib.vtgb_gemm_skinny_mxfp4(C.byref(args()), p + 2, None) not in (0, EINVAL)          # a bias that is not 4-byte aligned
    assert lib.vtgb_version() == 601
