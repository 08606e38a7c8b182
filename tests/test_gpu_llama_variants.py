"""-m gpu: rope-scaled and biased Llama models on the graph decoder, on the device.  fp32: ids against HF ``generate`` token for token (one
case per rope type, biases on; unpadded, padded, three beams), each after showing on HF alone that the switch moves the ids.  bf16, on a
llama3-scaled model with attention and MLP biases: the decoder against itself (replay = eager steps, a batch = its rows alone, two runs),
fp8 weights against the bf16 decoder over the dequantised weights with the same biases, the fp8 K/V cache against the reference decoder of
tests/test_gpu_kv_fp8.py, a 2100-token prompt through the chunked prefill against the torch prefill, and the first logits against HF's
fp32 forward next to the same figure of the twin without biases.  A plain Llama never reaches vtgb_gemm_skinny_bias.  A LightningModule
twin decodes a scaled, biased LM on the graph decoder and a ``dynamic`` one through HF.

The language model is the tiny Llama at head_dim 64 (hidden 256, four query heads on two K/V heads, two layers) with q_proj / k_proj x 8 (the
attention then depends on the positions) and lm_head x 40 (random-init logits are nearly flat); ``build_llama`` zeroes 1-D parameters, so
the biases are drawn here (std 0.2, next to activations of order 1)."""
import copy
import functools
import warnings

import pytest
import torch

from conftest import full_state_dict, load_golden, write_hf_config
from test_gpu_kv_fp8 import _reference_decoder, _steps      # the fp8 K/V cache's reference decoder; generate + the eagerly picked tokens' logits

pytestmark = pytest.mark.gpu

H, P, N_NEW, B = 256, 70, 12, 3
BIAS_STD = 0.2
ROPE = {
    "default": dict(rope_type="default", rope_theta=10000.0),
    "linear": dict(rope_type="linear", factor=4.0, rope_theta=10000.0),
    "llama3": dict(rope_type="llama3", factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0, original_max_position_embeddings=32, rope_theta=10000.0),
    "yarn": dict(rope_type="yarn", factor=4.0, original_max_position_embeddings=64, rope_theta=10000.0),
    "dynamic": dict(rope_type="dynamic", factor=4.0, rope_theta=10000.0),
}
BIAS = {"none": {}, "attention": dict(attention_bias=True), "mlp": dict(mlp_bias=True), "both": dict(attention_bias=True, mlp_bias=True)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return "cuda:0"


def _dress(lm, qk: float, head: float, zero_bias: bool):
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for l in lm.model.layers:
            l.self_attn.q_proj.weight.mul_(qk)
            l.self_attn.k_proj.weight.mul_(qk)
        lm.lm_head.weight.mul_(head)
        for n, p in lm.named_parameters():
            if n.endswith("proj.bias") and not zero_bias:
                p.copy_((torch.randn(p.shape, generator=g) * BIAS_STD).to(p.device, p.dtype))
    return lm.eval()


@functools.lru_cache(maxsize=None)
def _lm(dev, dtype, rope="default", bias="none", zero_bias=False):
    from videotgb_amd import llm
    lm = llm.build_llama("tiny", dtype, dev, seed=3, hidden_size=H, intermediate_size=512, num_attention_heads=4, num_key_value_heads=2,
                         num_hidden_layers=2, vocab_size=320, max_position_embeddings=4096, rope_parameters=dict(ROPE[rope]), **BIAS[bias])
    return _dress(lm, 8.0, 40.0, zero_bias)


@functools.lru_cache(maxsize=None)
def _inputs(dev, dtype, padded=False, n=B, p=P):
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(n, p, H, generator=g) * 0.5).to(dev, dtype)
    m = torch.ones(n, p, dtype=torch.long)
    if padded:
        m[1, :5] = 0      # one padded row (leading pads)
    return x, m.to(dev)


@functools.lru_cache(maxsize=None)
def _hf(dev, rope, bias, zero_bias=False, padded=False, num_beams=1):
    x, m = _inputs(dev, torch.float32, padded)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return _lm(dev, torch.float32, rope, bias, zero_bias).generate(inputs_embeds=x, attention_mask=m, do_sample=False, pad_token_id=0, eos_token_id=None,
                                                                      max_new_tokens=N_NEW, num_beams=num_beams)


# ------------------------------------------------------------------------------------------------------------------------- fp32: HF's ids
@pytest.mark.parametrize("rope,bias,padded,beams", [
    ("linear", "none", False, 1), ("llama3", "both", True, 1), ("yarn", "attention", True, 3), ("default", "mlp", False, 1), ("llama3", "none", False, 3),
])
def test_fp32_ids_equal_hf_generate(dev, rope, bias, padded, beams):
    from videotgb_amd.decode import GreedyDecoder
    ref = _hf(dev, rope, bias, padded=padded, num_beams=beams)
    # the switch matters, on HF alone: against the default rope type / against the biases zeroed
    if rope != "default":
        assert not torch.equal(ref, _hf(dev, "default", bias, padded=padded, num_beams=beams))
    if bias != "none":
        assert not torch.equal(ref, _hf(dev, rope, bias, zero_bias=True, padded=padded, num_beams=beams))
    x, m = _inputs(dev, torch.float32, padded)
    dec = GreedyDecoder(_lm(dev, torch.float32, rope, bias))
    out = dec.generate(x, N_NEW, attention_mask=m, pad_token_id=0, eos_token_id=None, num_beams=beams)
    st = next(reversed(dec.graphs.values()))
    assert st["attn"] is not None and st["graph"] is not None            # the fused step, replayed
    assert out.tolist() == ref.tolist(), (rope, bias, padded, beams)


# ------------------------------------------------------------------------------------------------------- bf16: a biased and scaled model
def _bf16(dev, zero_bias=False, rope="llama3"):
    return _lm(dev, torch.bfloat16, rope, "both", zero_bias)


def test_bf16_replay_eager_batch_and_repeat(dev):
    from videotgb_amd.decode import GreedyDecoder
    dec = GreedyDecoder(_bf16(dev))
    assert dec.bias is not None and dec.rope_scaled is not None
    x, m = _inputs(dev, torch.bfloat16, padded=True)
    out = dec.generate(x, N_NEW)
    (st,) = dec.graphs.values()
    assert st["graph"] is not None and "sk_ws" in st                      # the skinny weight stream, captured
    assert torch.equal(dec.generate(x, N_NEW), out)                       # two runs
    assert torch.equal(dec.generate(x, N_NEW, use_graph=False), out)      # eager stepping
    for b in range(B):
        assert torch.equal(dec.generate(x[b: b + 1].contiguous(), N_NEW)[0], out[b]), b      # a row alone
    outp = dec.generate(x, N_NEW, attention_mask=m)                       # a ragged batch
    assert torch.equal(dec.generate(x, N_NEW, attention_mask=m, use_graph=False), outp)
    kw = dict(num_beams=3, eos_token_id=None, attention_mask=m)           # beams: replay = eager steps
    assert torch.equal(dec.generate(x, N_NEW, **kw), dec.generate(x, N_NEW, use_graph=False, **kw))
    # (the biases and the scaling reach the bf16 step: other ids than the plain model's)
    plain = GreedyDecoder(_lm(dev, torch.bfloat16)).generate(x, N_NEW)
    assert not torch.equal(out, plain) and not torch.equal(out, GreedyDecoder(_bf16(dev, zero_bias=True)).generate(x, N_NEW))


def test_a_batch_beyond_the_skinny_kernel(dev):
    """130 rows: the decode step's projections go through vtgb_gemm with the bias; rows of the batch equal the same rows decoded in a
    skinny-sized batch of their own up to the two kernels' arithmetic, so only self-consistency is asserted: replay = eager steps."""
    from videotgb_amd.decode import GreedyDecoder
    dec = GreedyDecoder(_bf16(dev))
    x, _ = _inputs(dev, torch.bfloat16, False, 130, 9)
    out = dec.generate(x, 4)
    (st,) = dec.graphs.values()
    assert "sk_ws" not in st and st["graph"] is not None
    assert torch.equal(dec.generate(x, 4, use_graph=False), out)


def test_fp8_weights_equal_the_bf16_decoder_over_the_dequantised_weights(dev):
    from videotgb_amd import ops
    from videotgb_amd.decode import GreedyDecoder
    lm = _bf16(dev)
    ref = copy.deepcopy(lm)
    with torch.no_grad():
        for l in ref.model.layers:
            for part, names in ((l.self_attn, ("q_proj", "k_proj", "v_proj", "o_proj")), (l.mlp, ("gate_proj", "up_proj", "down_proj"))):
                for n in names:
                    w = getattr(part, n).weight
                    w.copy_(ops.dequantize_fp8_rows(*ops.quantize_fp8_rows(w)))      # (the biases stay as they are: never quantised)
        ref.lm_head.weight.copy_(ops.dequantize_fp8_rows(*ops.quantize_fp8_rows(ref.lm_head.weight)))
    x, m = _inputs(dev, torch.bfloat16, padded=True)
    dec8 = GreedyDecoder(lm, weights="fp8")
    (ids8, rec8), (ids, rec) = _steps(dec8, x, N_NEW, use_graph=True, attention_mask=m), _steps(GreedyDecoder(ref), x, N_NEW, use_graph=True, attention_mask=m)
    assert torch.equal(dec8.bias[0][0], torch.cat([getattr(lm.model.layers[0].self_attn, n).bias for n in ("q_proj", "k_proj", "v_proj")]).float())
    assert torch.equal(rec8[0], rec[0]) and torch.equal(ids8, ids)


@pytest.mark.parametrize("kind", ["unpadded", "padded"])
def test_fp8_kv_cache_equals_the_reference_decoder(dev, monkeypatch, kind):
    from videotgb_amd.decode import GreedyDecoder
    lm = _bf16(dev)
    x, m = _inputs(dev, torch.bfloat16, padded=True)
    kw = dict(attention_mask=m) if kind == "padded" else {}
    dec = GreedyDecoder(lm, kv_cache="fp8")
    ids, rec = _steps(dec, x, N_NEW, use_graph=True, **kw)
    (st,) = dec.graphs.values()
    assert st["attn"] == "split_fp8" and st["graph"] is not None and "kc" not in st
    ref = _reference_decoder(monkeypatch, lm)
    ids_r, rec_r = _steps(ref, x, N_NEW, **kw)
    (st_r,) = ref.graphs.values()
    assert st_r["attn"] == "split" and "kc" in st_r
    assert torch.equal(rec[0], rec_r[0]) and torch.equal(ids, ids_r)


def _first_logits(dec, x, **kw):
    return _steps(dec, x, 1, **kw)[1][0]


def _rel(a, ref):
    return ((a.double() - ref.double()).abs().max() / ref.double().abs().max()).item()


def test_chunked_prefill_of_2100_tokens_against_the_torch_prefill(dev):
    """The first logits behind a 2100-token prompt, chunked prefill (vtgb_gemm with the bias, tables advanced by 2048 rows for the second
    chunk) against the torch prefill of the same decoder, max |difference| over max |logits|.  The bound is what the plain twin (default
    rope, no biases) shows between the same two routes here, x 2: the bias adds one fp32 addition per output and the tables are operands,
    so the two routes differ as they did; a second chunk rotated from row 0, or a bias dropped by one route, would differ by the logits'
    own size.  Both figures are printed."""
    from videotgb_amd.decode import GreedyDecoder
    x, _ = _inputs(dev, torch.bfloat16, False, 1, 2100)
    err = {}
    for name, lm in (("biased llama3", _bf16(dev)), ("plain", _lm(dev, torch.bfloat16))):
        dec = GreedyDecoder(lm)
        chunked = _first_logits(dec, x)
        (st,) = dec.graphs.values()
        assert dec._use_chunked_prefill(st, x, 2100) and not dec._use_hip_prefill(x, 2100)
        tor = GreedyDecoder(lm)
        tor.PREFILL_MAX_TOKENS = 0
        assert not tor._use_chunked_prefill(st, x, 2100)
        err[name] = _rel(chunked, _first_logits(tor, x))
        print(f"2100-token prompt, {name}: first logits, chunked vs torch prefill: max |diff| / max |logits| = {err[name]:.3e}")
    assert err["biased llama3"] <= 2.0 * err["plain"], err
    # (and the routes are not trivially equal because the scaling is ignored by both: the biased, scaled logits are other logits)
    assert _rel(_first_logits(GreedyDecoder(_bf16(dev)), x), _first_logits(GreedyDecoder(_lm(dev, torch.bfloat16)), x)) > 0.1


def test_bf16_accuracy_against_hf_fp32_next_to_the_unbiased_twin(dev):
    """max |fused first logits - HF fp32 logits| / max |HF logits| for the biased model and for its twin with the biases zeroed:
    biased <= 2 x unbiased (one fp32 addition per output; a dropped or misrouted bias of std 0.2 moves the logits by their own size)."""
    from videotgb_amd.decode import GreedyDecoder
    x, _ = _inputs(dev, torch.bfloat16)
    err = {}
    for name, zero in (("biased", False), ("unbiased", True)):
        lm = _bf16(dev, zero_bias=zero)
        ref = copy.deepcopy(lm).float()
        with torch.no_grad():
            want = ref(inputs_embeds=x.float()).logits[:, -1]
        err[name] = _rel(_first_logits(GreedyDecoder(lm), x), want)
        print(f"bf16 fused first logits vs HF fp32, {name}: max |diff| / max |logits| = {err[name]:.3e}")
    assert err["biased"] <= 2.0 * err["unbiased"], err


def test_a_plain_llama_never_reaches_the_bias_entry(dev, monkeypatch):
    from videotgb_amd import _lib as L
    from videotgb_amd.decode import GreedyDecoder
    calls, entry = [], L.lib().vtgb_gemm_skinny_bias

    def spy(*a):
        calls.append(1)
        return entry(*a)
    monkeypatch.setattr(L.lib(), "vtgb_gemm_skinny_bias", spy)
    x, m = _inputs(dev, torch.bfloat16, padded=True)
    for kw in (dict(), dict(weights="fp8"), dict(kv_cache="fp8")):
        dec = GreedyDecoder(_lm(dev, torch.bfloat16), **kw)
        assert dec.bias is None and dec.rope_scaled is None
        dec.generate(x, 4, attention_mask=m)
        if "kv_cache" not in kw:      # (beams keep the bf16 K/V cache)
            dec.generate(x, 4, num_beams=2)
    assert not calls
    GreedyDecoder(_bf16(dev)).generate(x, 4, attention_mask=m)
    assert calls      # (the spy sees the entry: a biased model goes through it)


# ------------------------------------------------------------------------------------------------------------------------ a module twin
class BE(dict):
    __getattr__ = dict.get


def up4(q):
    return q.float().repeat_interleave(4, -2).repeat_interleave(4, -1)


def test_module_twin_decodes_a_scaled_biased_lm_on_the_graph_decoder_and_a_dynamic_one_through_hf(dev, tmp_path):
    from videotgb_amd import llm, models, modules
    from videotgb_amd.synth import tiny_cfg
    cfg = tiny_cfg("instructblip")
    base = write_hf_config(str(tmp_path / "instructblip-tiny"), "instructblip", cfg, "llama")
    built = models.build_language_model(models.load_hf_config(base, "instructblip"))
    sd = full_state_dict(cfg, built)
    raft_pth = str(tmp_path / "raft-things.pth")
    torch.save({"module." + k[len("of_extractor."):]: v for k, v in sd.items() if k.startswith("of_extractor.")}, raft_pth)
    proc = BE(tokenizer=BE(pad_token_id=0), batch_decode=lambda ids, skip_special_tokens=True: [" ".join(map(str, r)) for r in ids.tolist()])
    m = modules.LSTPModule(model_name_or_path=base, sampler_name_or_path=str(tmp_path / "no-bert-weights"), of_extractor_name_or_path=raft_pth,
                           temperature=1.0, generate_configs=dict(do_sample=False, max_new_tokens=8), compute_dtype="f32", processor=proc, tgb_cfg=cfg.tgb)
    m.load_state_dict(sd, strict=True)
    m.to(dev)
    g = load_golden("tiny_modules")
    batch = dict(frames=(up4(g["frames_q8"]) / 48).to(dev), nframe=int(g["nframe"]), of_lengths=g["of_lengths"].tolist(),
                 answer=torch.zeros(2, 1, dtype=torch.long, device=dev), text_answer=[""] * 2,
                 sampler_question=g["ib_sampler_ids"].to(dev), sampler_question_attention_mask=g["ib_sampler_mask"].to(dev),
                 qformer_text=g["ib_qformer_ids"].to(dev), qformer_text_attention_mask=g["ib_qformer_mask"].to(dev),
                 question=g["ib_question"].to(dev), question_attention_mask=g["ib_question_mask"].to(dev))
    noise = g["ib_noise"].to(dev) if "ib_noise" in g else None
    geometry = {k: getattr(built.config, k) for k in ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "num_key_value_heads",
                                                       "vocab_size")}

    def swap(rope, **bias):      # the twin's language model, replaced by one of the same geometry with the switches on
        lm = llm.build_llama("tiny", torch.float32, dev, seed=3, max_position_embeddings=256, rope_parameters=dict(ROPE[rope]), **geometry, **bias)
        m.model.language_model = _dress(lm, 16.0, 1.0, False)
        m._decoder = None

    def both_ways():
        m.fast_decode = False
        ref = m.eval_forward(batch, noise=noise)
        assert getattr(m, "_decoder", None) is None
        m.fast_decode = True
        return m.eval_forward(batch, noise=noise), ref
    swap("default")
    _, plain = both_ways()
    swap("llama3", attention_bias=True, mlp_bias=True)
    ids, ref = both_ways()
    assert m._decoder is not None and m._decoder.bias is not None and m._decoder.rope_scaled is not None      # the graph decoder served it
    assert ids.tolist() == ref.tolist() and ref.tolist() != plain.tolist()
    swap("dynamic")
    ids, ref = both_ways()
    assert getattr(m, "_decoder", None) is None and ids.tolist() == ref.tolist()                                # HF generate served it
