"""-m gpu: beam search on the Llama graph decoder (opt-in: beam_search="graph") on the device -- the fused step over
vtgb_llm_decode_attention_beam and vtgb_llm_beam_candidates.  fp32 ids against HF ``generate`` (transformers' ``_beam_search``) on the device,
token for token, for the cases of tests/test_beam_decode.py; at bf16 the decoder against itself (replay = eager steps, a batch = its rows
alone, two runs); fp8 weights against the bf16 decoder over the dequantised weights; LoRA adapters against HF; and a LightningModule twin
with the shipped SF ``generate_configs``, with and without the opt-in.  The language model is the tiny Llama at head_dim 64 (hidden 128, two
query heads on one K/V head) with lm_head x 40: unscaled, random-init logits are nearly flat and every beam ties."""
import copy
import functools
import warnings

import pytest
import torch
from torch.profiler import ProfilerActivity, profile

from conftest import full_state_dict, load_golden, write_hf_config

pytestmark = pytest.mark.gpu

N_NEW, P, H = 24, 9, 128
SHIPPED_SF = dict(length_penalty=1, repetition_penalty=1.5, num_beams=5, min_length=1, max_length=250, top_p=0.9, temperature=0.8)
BEAM_KERNEL, CAND_KERNEL = "llm_decode_attn_beam_kernel", "beam_row_kernel"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return "cuda:0"


@functools.lru_cache(maxsize=None)
def _lm(dev, dtype, lora=False):
    from videotgb_amd import llm
    lm = llm.build_llama("tiny", dtype, dev, seed=3, hidden_size=H, num_hidden_layers=3, num_key_value_heads=1).eval()
    with torch.no_grad():
        lm.lm_head.weight.mul_(40.0)
    if lora:
        import lora_refs
        from videotgb_amd import train
        train.apply_lora(lm)
        lora_refs.nonzero_lora_(lm, seed=5, std=0.3)
        lm.eval()
    return lm


@functools.lru_cache(maxsize=None)
def _decoder(dev, dtype, lora=False, **kw):
    from videotgb_amd.decode import GreedyDecoder
    return GreedyDecoder(_lm(dev, dtype, lora), **kw)


@functools.lru_cache(maxsize=None)
def _inputs(dev, dtype, B):
    g = torch.Generator().manual_seed(3 + B)
    x = torch.randn(B, P, H, generator=g).to(dev, dtype)
    m = torch.ones(B, P, dtype=torch.long)
    if B > 1:
        m[1, :3] = 0      # a padded row (leading pads)
    return x, m.to(dev)


def _hf(lm, x, m, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return lm.generate(inputs_embeds=x, attention_mask=m, do_sample=False, pad_token_id=0, **kw)


@functools.lru_cache(maxsize=None)
def _eos_ids(dev, B, K):
    """eos ids chosen from what the model emits (the unconstrained search's output from the third position on)."""
    x, m = _inputs(dev, torch.float32, B)
    free = _hf(_lm(dev, torch.float32), x, m, num_beams=K, repetition_penalty=1.5, max_new_tokens=N_NEW, eos_token_id=None)
    seen = []
    for t in free[:, 2:].flatten().tolist():
        if t not in seen and t != 0:
            seen.append(t)
    return tuple(seen[:3])


def _beam_state(dec):
    st = next(reversed(dec.graphs.values()))
    assert st["attn"] == "beam" and st["beam"]["kernel"]
    return st


@pytest.mark.parametrize("K", [2, 3, 5])
@pytest.mark.parametrize("B", [1, 3])
def test_fp32_ids_equal_hf_generate(dev, B, K):
    lm, dec = _lm(dev, torch.float32), _decoder(dev, torch.float32)
    x, m = _inputs(dev, torch.float32, B)
    ended = full = False
    for eos in (None,) + _eos_ids(dev, B, K):
        kw = dict(num_beams=K, repetition_penalty=1.5, length_penalty=1.0, eos_token_id=eos)
        ref = _hf(lm, x, m, max_new_tokens=N_NEW, **kw)
        out = dec.generate(x, N_NEW, attention_mask=m, pad_token_id=0, **kw)
        st = _beam_state(dec)
        assert st["graph"] is not None                                    # the fused step, replayed
        assert out.tolist() == ref.tolist(), (B, K, eos)
        if eos is not None:
            has = (ref == eos).any(-1)
            ended |= bool(has.any())
            full |= bool((~has).any())
        else:
            full |= ref.shape[1] == N_NEW
    assert ended and full, "over these requests at least one row ends early and at least one runs to the end"
    if K == 5 and B == 3:      # the winning beams were re-ordered: the ancestry table is not the identity
        bi = st["beam_bi"][:, 0]
        assert ((bi % K)[:, 1:] != 0).any()


@pytest.mark.parametrize("length_penalty", [0.0, 2.0])
def test_fp32_length_penalty_min_new_tokens_and_the_shipped_dict(dev, length_penalty):
    lm, dec = _lm(dev, torch.float32), _decoder(dev, torch.float32)
    B, K = 3, 3
    x, m = _inputs(dev, torch.float32, B)
    eos = _eos_ids(dev, B, K)[0]
    kw = dict(num_beams=K, repetition_penalty=1.5, length_penalty=length_penalty, eos_token_id=eos)
    assert dec.generate(x, N_NEW, attention_mask=m, pad_token_id=0, **kw).tolist() == _hf(lm, x, m, max_new_tokens=N_NEW, **kw).tolist()
    kw = dict(kw, min_new_tokens=12)
    ref = _hf(lm, x, m, max_new_tokens=N_NEW, **kw)
    assert dec.generate(x, N_NEW, attention_mask=m, pad_token_id=0, **kw).tolist() == ref.tolist() and not (ref[:, :12] == eos).any()
    if length_penalty == 0.0:
        ref = _hf(lm, x, m, **dict(SHIPPED_SF, max_length=P + N_NEW))
        out = dec.generate(x, N_NEW, attention_mask=m, pad_token_id=0, eos_token_id=2, num_beams=5, repetition_penalty=1.5, length_penalty=1)
        assert out.tolist() == ref.tolist()


def test_bf16_replay_eager_batch_and_repeat(dev):
    dec = _decoder(dev, torch.bfloat16)
    kw = dict(num_beams=5, repetition_penalty=1.5, eos_token_id=2, pad_token_id=0)
    x, m = _inputs(dev, torch.bfloat16, 3)
    x2, m2 = x[:2].contiguous(), torch.ones(2, P, dtype=torch.long, device=dev)
    out = dec.generate(x2, N_NEW, **kw)
    st = _beam_state(dec)
    assert st["graph"] is not None and "sk_ws" in st                      # the skinny weight stream at B * K = 10 rows
    assert torch.equal(dec.generate(x2, N_NEW, **kw), out)                # two runs
    assert torch.equal(dec.generate(x2, N_NEW, use_graph=False, **kw), out)      # eager stepping
    rows = [dec.generate(x2[b: b + 1].contiguous(), N_NEW, **kw) for b in range(2)]
    n = out.shape[1]
    for b in range(2):                                                    # (a row alone is cropped to its own length: the batch pads it with the fill value)
        r = rows[b][0]
        assert torch.equal(out[b, : r.numel()], r) and (out[b, r.numel():] == 2).all() and r.numel() <= n
    outp = dec.generate(x, N_NEW, attention_mask=m, **kw)                 # a ragged batch: replay = eager steps
    assert torch.equal(dec.generate(x, N_NEW, attention_mask=m, use_graph=False, **kw), outp)


def test_fp8_weights_equal_the_bf16_decoder_over_the_dequantised_weights(dev):
    from videotgb_amd import ops
    from videotgb_amd.decode import GreedyDecoder
    lm = _lm(dev, torch.bfloat16)
    ref = copy.deepcopy(lm)
    with torch.no_grad():
        for l in ref.model.layers:
            for part, names in ((l.self_attn, ("q_proj", "k_proj", "v_proj", "o_proj")), (l.mlp, ("gate_proj", "up_proj", "down_proj"))):
                for n in names:
                    w = getattr(part, n).weight
                    w.copy_(ops.dequantize_fp8_rows(*ops.quantize_fp8_rows(w)))
        ref.lm_head.weight.copy_(ops.dequantize_fp8_rows(*ops.quantize_fp8_rows(ref.lm_head.weight)))
    x, m = _inputs(dev, torch.bfloat16, 3)
    kw = dict(num_beams=5, repetition_penalty=1.5, eos_token_id=2, pad_token_id=0, attention_mask=m)
    dec8 = GreedyDecoder(lm, weights="fp8")
    out8 = dec8.generate(x, N_NEW, **kw)
    _beam_state(dec8)
    assert torch.equal(out8, GreedyDecoder(ref).generate(x, N_NEW, **kw))


def test_lora_fp32_ids_equal_hf_generate(dev):
    lm, dec = _lm(dev, torch.float32, True), _decoder(dev, torch.float32, True)
    x, m = _inputs(dev, torch.float32, 3)
    kw = dict(num_beams=3, repetition_penalty=1.5, eos_token_id=None)
    ref = _hf(lm, x, m, max_new_tokens=N_NEW, **kw)
    out = dec.generate(x, N_NEW, attention_mask=m, pad_token_id=0, **kw)
    _beam_state(dec)
    assert out.tolist() == ref.tolist()
    assert out.tolist() != _decoder(dev, torch.float32).generate(x, N_NEW, attention_mask=m, pad_token_id=0, **kw).tolist()      # (the adapters matter)


def test_what_the_device_path_refuses(dev):
    from videotgb_amd import llm
    from videotgb_amd.decode import GreedyDecoder
    lm = llm.build_llama("tiny", torch.float32, dev, seed=3)      # head_dim 16
    with pytest.raises(NotImplementedError, match="head_dim"):
        GreedyDecoder(lm).generate(torch.zeros(1, 4, 32, device=dev), 4, num_beams=2)
    with pytest.raises(NotImplementedError):
        GreedyDecoder(_lm(dev, torch.bfloat16), kv_cache="fp8").generate(torch.zeros(1, 4, H, device=dev, dtype=torch.bfloat16), 4, num_beams=2)


# ------------------------------------------------------------------------------------------------------------------- a module twin
class BE(dict):
    __getattr__ = dict.get


def _kernel_names(fn):
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, {e.key for e in prof.key_averages()}


def _sf_module(dev, tmp_path, **kw):
    from videotgb_amd import models, modules
    from videotgb_amd.synth import tiny_cfg
    cfg = tiny_cfg("instructblip")
    cfg.llm_hidden = H      # two heads: head_dim 64
    base = write_hf_config(str(tmp_path / "instructblip-tiny"), "instructblip", cfg, "llama")
    sd = full_state_dict(cfg, models.build_language_model(models.load_hf_config(base, "instructblip")))
    raft_pth = str(tmp_path / "raft-things.pth")
    torch.save({"module." + k[len("of_extractor."):]: v for k, v in sd.items() if k.startswith("of_extractor.")}, raft_pth)
    proc = BE(tokenizer=BE(pad_token_id=0), batch_decode=lambda ids, skip_special_tokens=True: [" ".join(map(str, r)) for r in ids.tolist()])
    m = modules.LSTPSFModule(model_name_or_path=base, sampler_name_or_path=str(tmp_path / "no-bert-weights"), of_extractor_name_or_path=raft_pth,
                             temperature=1.0, generate_configs=dict(SHIPPED_SF), compute_dtype="f32", processor=proc, tgb_cfg=cfg.tgb, **kw)
    m.load_state_dict(sd, strict=True)
    m.to(dev)
    with torch.no_grad():
        m.model.language_model.lm_head.weight.mul_(40.0)
    g = load_golden("tiny_modules")
    up4 = lambda q: q.float().repeat_interleave(4, -2).repeat_interleave(4, -1)      # noqa: E731
    B = 2
    batch = dict(frames=(up4(g["frames_q8"]) / 48).to(dev), nframe=int(g["nframe"]), of_lengths=g["of_lengths"].tolist(),
                 answer=torch.zeros(B, 1, dtype=torch.long, device=dev), text_answer=[""] * B,
                 sampler_question=g["sf_sampler_ids"].to(dev), sampler_question_attention_mask=g["sf_sampler_mask"].to(dev),
                 qformer_text=g["sf_qformer_ids"].to(dev), qformer_text_attention_mask=g["sf_qformer_mask"].to(dev),
                 question=g["sf_question"].to(dev), question_attention_mask=g["sf_question_mask"].to(dev),
                 of=(up4(g["of_q8"]) / 127).to(dev), of_mask=g["of_mask"].to(dev))
    return m, batch, g["sf_noise"].to(dev)


def test_sf_module_eval_forward_with_the_shipped_generate_configs(dev, tmp_path):
    """Without the opt-in: HF generate, and neither new kernel is launched.  beam_search="graph": the same ids at fp32, on the beam kernels
    and without a BLAS kernel."""
    m, batch, noise = _sf_module(dev, tmp_path)
    assert m.beam_search == "hf"
    ref, names = _kernel_names(lambda: m.eval_forward(batch, noise=noise))      # the default: HF generate
    assert getattr(m, "_decoder", None) is None and ref.shape[1] > 1
    assert not any(BEAM_KERNEL in n or CAND_KERNEL in n or "beam_merge_kernel" in n for n in names)
    m.beam_search = "graph"
    ids, names = _kernel_names(lambda: m.eval_forward(batch, noise=noise))
    assert getattr(m, "_decoder", None) is not None and _beam_state(m._decoder)["beam"]["K"] == 5
    assert ids.tolist() == ref.tolist()
    assert any(BEAM_KERNEL in n for n in names) and any(CAND_KERNEL in n for n in names), sorted(names)[:60]
    blas = sorted(n for n in names if "Cijk_" in n)
    assert not blas, blas
