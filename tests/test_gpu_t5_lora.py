"""-m gpu: LoRA adapters on the T5 graph decoder, on the device.  fp32: the fused decoder's ids equal HF ``generate`` over the
train.LoraLinear model, token for token -- greedy, a padded encoder row, and beam search under beam_search="graph+t5" with the shipped
``generate_configs`` at 5 beams -- at d_kv 16 and 64.  bf16 at a geometry the skinny GEMM splits along K (d_model 1024: 16 k-tiles, two
splits), the decoder against itself: replay = eager steps, a batch = its rows alone, and the one-launch form (vtgb_llm_lora_parts over the
deferred fragments, ``LORA_PARTS``) = the two-launch form, bit for bit on every step's logits; the parts entry is really launched when on,
and neither LoRA entry for an adapter-free T5.  Through the top: ``LSTP_blip2(lora=True).generate`` and the SEQ_2_SEQ_LM LightningModule
twin's ``eval_forward`` equal HF ``generate`` without falling back."""
import functools
import warnings

import pytest
import torch

import lora_refs as R
from conftest import full_state_dict, write_hf_config

pytestmark = pytest.mark.gpu

N_NEW, P, B = 12, 7, 3
L_E = L_D = 3
SHIPPED_SF = dict(length_penalty=1, repetition_penalty=1.5, num_beams=5, min_length=1, max_length=250)      # LSTP_SF_blip2.yaml / LSTP_TG_blip2.yaml


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return "cuda:0"


@functools.lru_cache(maxsize=None)
def _lm(dev, dtype, dk, lora=True, wide=False):
    """The tiny T5 of tests/test_gpu_t5_beam_decode.py (d_model 64); ``wide``: d_model 1024, 2 + 2 layers -- K = 1024 is what the skinny
    GEMM splits in two for the 192-column q|k|v and the 64-column cross q.  Adapters: apply_lora's defaults for a T5, lora_B ~ N(0, 0.3)."""
    from transformers import T5Config, T5ForConditionalGeneration
    from videotgb_amd import train
    torch.manual_seed(0)
    D, layers = (1024, 2) if wide else (64, L_E)
    cfg = T5Config(vocab_size=200, d_model=D, d_kv=dk, d_ff=96, num_layers=layers, num_decoder_layers=layers, num_heads=4, feed_forward_proj="gated-gelu",
                   tie_word_embeddings=False, decoder_start_token_id=0, pad_token_id=0, eos_token_id=1)
    lm = T5ForConditionalGeneration(cfg).eval()
    for p in lm.parameters():
        p.data.normal_(0, 0.05 if wide else 0.3 if dk == 16 else 0.15)      # (scores grow with d_kv and d_model: T5 does not scale them)
    with torch.no_grad():
        lm.lm_head.weight.mul_(4.0)
    if lora:
        train.apply_lora(lm)
        R.nonzero_lora_(lm, seed=5, std=0.3)
        lm.eval()
    return lm.to(device=dev, dtype=dtype) if not lora else _cast_base(lm, dev, dtype)


def _cast_base(lm, dev, dtype):
    """The model on the device in ``dtype`` with the adapters kept in fp32 (peft's layout: the base weights take the model's dtype)."""
    lm.to(device=dev, dtype=dtype)
    for n, p in lm.named_parameters():
        if "lora_" in n:
            p.data = p.data.float()
    return lm


@functools.lru_cache(maxsize=None)
def _inputs(dev, dtype, D=64, rows=B):
    g = torch.Generator().manual_seed(5 + rows)
    x = (torch.randn(rows, P, D, generator=g) * 0.5).to(dev, dtype)
    m = torch.ones(rows, P, dtype=torch.long)
    if rows > 1:
        m[1, -2:] = 0      # a padded encoder row
    return x, m.to(dev)


def _hf(lm, x, m, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return lm.generate(inputs_embeds=x, attention_mask=m, do_sample=False, pad_token_id=0, **kw)


# ------------------------------------------------------------------------------------------------------------------------------------ fp32
@pytest.mark.parametrize("dk", [16, 64])
@pytest.mark.parametrize("padded", [False, True])
def test_fp32_fused_greedy_ids_equal_hf_generate_over_the_lora_model(dev, dk, padded):
    from videotgb_amd.decode import T5GreedyDecoder, lora_state
    lm = _lm(dev, torch.float32, dk)
    assert lora_state(lm) == "ok"
    x, m = _inputs(dev, torch.float32)
    if not padded:
        m = torch.ones_like(m)
    ref = _hf(lm, x, m, max_new_tokens=N_NEW, min_new_tokens=N_NEW, eos_token_id=1)
    dec = T5GreedyDecoder(lm)
    out = dec.generate(x, N_NEW, eos_token_id=1, pad_token_id=0, min_new_tokens=N_NEW, attention_mask=m if padded else None)
    (st,) = dec.graphs.values()
    assert st["hip"] and st["graph"] is not None and dec.lora is not None      # the fused step, replayed
    assert out.tolist() == ref.tolist()
    base = T5GreedyDecoder(_lm(dev, torch.float32, dk, lora=False)).generate(x, N_NEW, eos_token_id=1, pad_token_id=0, min_new_tokens=N_NEW,
                                                                            attention_mask=m if padded else None)
    assert all(base[b].tolist() != out[b].tolist() for b in range(B))      # the adapters change every row


@pytest.mark.parametrize("dk", [16, 64])
def test_fp32_beams_with_the_shipped_generate_configs_equal_hf_generate(dev, dk):
    from videotgb_amd import decode
    lm = _lm(dev, torch.float32, dk)
    x, m = _inputs(dev, torch.float32)
    cfgs = dict(SHIPPED_SF, max_length=1 + N_NEW)
    owner = type("Owner", (), dict(beam_search="graph+t5"))()
    out = decode.graph_generate(owner, lm, x, m, cfgs)
    assert out is not None and owner._decoder.lora is not None
    st = next(reversed(owner._decoder.graphs.values()))
    assert st["attn"] == "beam" and st["beam"]["K"] == 5 and st["graph"] is not None
    assert out.tolist() == _hf(lm, x, m, **cfgs).tolist()


# ------------------------------------------------------------------------------------------------------------------------------------ bf16
DK_W = 16      # the wide model's d_kv: q|k|v has 192 columns, the cross q 64


def _wide(dev, lora=True):
    return _lm(dev, torch.bfloat16, DK_W, lora, True)


def _steps(dec, x, m, n=6):
    """(ids, every eager step's logits) of a greedy call without the graph."""
    rec, emit = [], dec._emit

    def spy(st, logits):
        rec.append(logits.float().clone())
        return emit(st, logits)
    dec._emit = spy
    try:
        ids = dec.generate(x, n, use_graph=False, eos_token_id=1, pad_token_id=0, min_new_tokens=n, attention_mask=m)
    finally:
        del dec._emit
    return ids, rec


def test_the_wide_geometry_is_split(dev):
    """(The premise of the bf16 tests: both adapted projections of a decode step come as K-split fragments.)"""
    from videotgb_amd import ops
    x = torch.zeros(B, 1024, dtype=torch.bfloat16, device=dev)
    for n_cols in (3 * 4 * DK_W, 4 * DK_W):
        _, S, part = ops.gemm_skinny(x, torch.zeros(n_cols, 1024, dtype=torch.bfloat16, device=dev), defer_reduce=True)
        assert S > 1 and part is not None


def test_bf16_replay_eager_rows_and_the_two_forms(dev):
    from videotgb_amd.decode import T5GreedyDecoder
    lm = _wide(dev)
    x, m = _inputs(dev, torch.bfloat16, 1024)
    kw = dict(eos_token_id=1, pad_token_id=0, min_new_tokens=N_NEW)
    dec = T5GreedyDecoder(lm)
    assert dec.LORA_PARTS in (True, False)
    outs = {}
    for parts in (True, False):
        dec = T5GreedyDecoder(lm)
        dec.LORA_PARTS = parts
        out = dec.generate(x, N_NEW, attention_mask=m, **kw)
        (st,) = dec.graphs.values()
        assert st["hip"] and st["graph"] is not None and "sk_ws" in st
        assert torch.equal(dec.generate(x, N_NEW, attention_mask=m, use_graph=False, **kw), out)      # replay = eager steps
        for b in range(B):                                                                            # a batch = its rows alone
            mb = m[b: b + 1] if b == 1 else None
            assert torch.equal(dec.generate(x[b: b + 1].contiguous(), N_NEW, attention_mask=mb, **kw)[0], out[b]), (parts, b)
        outs[parts] = (out, _steps(dec, x, m)[1])
    assert torch.equal(outs[True][0], outs[False][0])
    assert len(outs[True][1]) == len(outs[False][1]) == 6
    for a, b in zip(outs[True][1], outs[False][1]):      # the one-launch form = the two-launch form, on every step's logits
        assert torch.equal(a, b)
    base = T5GreedyDecoder(_wide(dev, lora=False)).generate(x, N_NEW, attention_mask=m, **kw)
    assert not torch.equal(base, outs[True][0])


def _count(monkeypatch):
    from videotgb_amd import _lib as L, ops
    calls = []
    for name in ("vtgb_llm_lora", "vtgb_llm_lora_parts"):
        entry = getattr(L.lib(), name)
        monkeypatch.setattr(L.lib(), name, lambda *a, _e=entry, _n=name: (calls.append(_n), _e(*a))[1])
    for name in ("lora_update", "lora_update_parts"):
        fn = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _f=fn, _n=name: (calls.append(_n), _f(*a))[1])
    return calls


def test_the_parts_entry_is_launched_when_on_and_nothing_without_adapters(dev, monkeypatch):
    """Per generate call the encoder's q|k|v (one vtgb_llm_lora per encoder layer) and the cross-attention K | V (one per decoder layer) are
    updated once; every decode step that runs on the host -- the eager ones and the captured one -- updates q|k|v and the cross q of every
    decoder layer: through vtgb_llm_lora_parts when LORA_PARTS is on (bf16, split projections), through vtgb_llm_lora otherwise.  An
    adapter-free T5 reaches neither entry (encoder, eager steps, capture, replay), at fp32 and at bf16."""
    from videotgb_amd.decode import T5GreedyDecoder
    calls = _count(monkeypatch)
    for dtype, wide in ((torch.float32, False), (torch.bfloat16, True)):
        D = 1024 if wide else 64
        x, m = _inputs(dev, dtype, D)
        dec = T5GreedyDecoder(_lm(dev, dtype, DK_W, False, wide))
        assert dec.lora is None
        dec.generate(x, 4, attention_mask=m)
        dec.generate(x, 4, attention_mask=m, use_graph=False)
        dec.generate(x, 4, num_beams=2)
        assert calls == []
    x, m = _inputs(dev, torch.bfloat16, 1024)
    lm = _wide(dev)
    layers = 2
    once = 2 * layers      # encoder q|k|v + cross K | V
    n = {}
    for parts in (True, False):
        dec = T5GreedyDecoder(lm)
        dec.LORA_PARTS = parts
        dec.generate(x, 4, attention_mask=m)
        n[parts] = {k: calls.count(k) for k in ("vtgb_llm_lora", "vtgb_llm_lora_parts", "lora_update", "lora_update_parts")}
        calls.clear()
    on, off = n[True], n[False]
    steps = on["vtgb_llm_lora_parts"] // (2 * layers)
    assert steps >= 1 and on["vtgb_llm_lora_parts"] == on["lora_update_parts"] == steps * 2 * layers, n
    assert on["vtgb_llm_lora"] == on["lora_update"] == once, n
    assert off["vtgb_llm_lora_parts"] == off["lora_update_parts"] == 0 and off["vtgb_llm_lora"] == off["lora_update"] == once + steps * 2 * layers, n
    dec = T5GreedyDecoder(_lm(dev, torch.float32, DK_W))      # fp32: the exactness mode has no fragments
    x32, m32 = _inputs(dev, torch.float32)
    dec.generate(x32, 4, attention_mask=m32)
    assert calls.count("vtgb_llm_lora_parts") == 0 and calls.count("vtgb_llm_lora") > L_E + L_D


# ---------------------------------------------------------------------------------------------------------------------- through the top
class BE(dict):
    __getattr__ = dict.get


def _refuse_hf(lm, monkeypatch):
    def no(*a, **k):
        raise AssertionError("the request fell back to HF generate")
    monkeypatch.setattr(lm, "generate", no)


def test_lstp_blip2_generate_with_adapters(dev, tiny_sd):
    """models.LSTP_blip2(..., lora=True) at fp32 with nonzero lora_B: generate on the graph decoder (fast_decode=True insists: a request
    outside the envelope raises instead of falling back) equals HF generate over the LoraLinear model (fast_decode=False)."""
    from test_gpu_session import clip, questions
    from transformers import T5Config, T5ForConditionalGeneration
    from videotgb_amd import models
    from videotgb_amd.decode import lora_state
    from videotgb_amd.synth import synth_tensor
    cfg, sd = tiny_sd["blip2"]
    torch.manual_seed(0)
    lm = T5ForConditionalGeneration(T5Config(vocab_size=120, d_model=cfg.llm_hidden, d_kv=16, d_ff=64, num_layers=2, num_decoder_layers=2, num_heads=2,
                                             feed_forward_proj="gated-gelu", tie_word_embeddings=False, decoder_start_token_id=0, pad_token_id=0,
                                             eos_token_id=1)).to(dev).eval()
    lm.load_state_dict({k: synth_tensor("model.language_model." + k, tuple(v.shape)).to(dev) for k, v in lm.state_dict().items()}, strict=True)
    with torch.no_grad():
        lm.lm_head.weight.mul_(4.0)
    T, nframe = 12, 4
    frames, flow_frames = clip(cfg, dev, T)
    (te, se, noise), = questions("blip2", cfg, dev, [(5, 7, 4)], T)
    kw = dict(do_sample=False, temperature=None, max_new_tokens=12, min_new_tokens=12, noise=noise)
    m = models.LSTP_blip2(cfg, dev, False, language_model=lm, compute_dtype="f32")
    m.load_state_dict(sd, strict=False)
    m.to(dev)
    base_ids, _ = m.generate(frames, flow_frames, nframe, te, se, fast_decode=True, **kw)
    m = models.LSTP_blip2(cfg, dev, True, language_model=lm, compute_dtype="f32")      # wraps q / v of the same lm
    m.load_state_dict(sd, strict=False)
    m.to(dev)
    assert sum("lora_" in k for k in m.state_dict()) == 2 * (2 * 2 + 4 * 2)
    R.nonzero_lora_(m.model.language_model, seed=9)
    assert lora_state(m.model.language_model) == "ok"
    ref, cand_ref = m.generate(frames, flow_frames, nframe, te, se, fast_decode=False, **kw)
    ids, cand = m.generate(frames, flow_frames, nframe, te, se, fast_decode=True, **kw)
    assert m._decoder.lora is not None and m.fell_back is False
    assert torch.equal(ids, ref) and torch.equal(cand, cand_ref), (ids.tolist(), ref.tolist())
    auto, _ = m.generate(frames, flow_frames, nframe, te, se, **kw)
    assert torch.equal(auto, ref)
    assert not torch.equal(ids, base_ids)


def test_the_seq2seq_twin_eval_forward_with_adapters(dev, tmp_path, monkeypatch):
    """modules.LSTPBlip2IVTModule (LORA = "SEQ_2_SEQ_LM") at fp32, in eval mode, nonzero lora_B: eval_forward through the graph decoder equals
    HF generate (fast_decode = False), and the fast path does not reach HF generate at all."""
    from videotgb_amd import models, modules
    from videotgb_amd.decode import lora_state
    from videotgb_amd.synth import tiny_cfg
    cfg = tiny_cfg("blip2")
    base = write_hf_config(str(tmp_path / "blip2-tiny"), "blip2", cfg, "t5")
    sd = full_state_dict(cfg, models.build_language_model(models.load_hf_config(base, "blip2")))
    raft_pth, sampler_pth = str(tmp_path / "raft-things.pth"), str(tmp_path / "sampler.pth")
    torch.save({"module." + k[len("of_extractor."):]: v for k, v in sd.items() if k.startswith("of_extractor.")}, raft_pth)
    torch.save({"module." + k[len("temporal_encoder."):]: v for k, v in sd.items() if k.startswith("temporal_encoder.")}, sampler_pth)
    proc = BE(tokenizer=BE(pad_token_id=0), batch_decode=lambda ids, skip_special_tokens=True: [" ".join(map(str, r)) for r in ids.tolist()])
    m = modules.LSTPBlip2IVTModule(model_name_or_path=base, sampler_name_or_path=sampler_pth, of_extractor_name_or_path=raft_pth,
                                   generate_configs=dict(max_new_tokens=10, min_new_tokens=10, do_sample=False), compute_dtype="f32", processor=proc,
                                   tgb_cfg=cfg.tgb)
    m.load_state_dict(sd, strict=False)
    m.to(dev).eval()
    lm = m.model.language_model
    with torch.no_grad():
        lm.lm_head.weight.mul_(4.0)
    R.nonzero_lora_(lm, seed=9)
    assert lora_state(lm) == "ok"
    g = torch.Generator().manual_seed(3)
    widths = [2, 3]
    q = torch.randint(3, 120, (2, 6), generator=g)
    qm = torch.ones(2, 6, dtype=torch.long)
    qm[1, -2:] = 0
    batch = dict(frames=torch.randn(sum(widths), 3, cfg.vit.image, cfg.vit.image, generator=g).to(dev), widths=widths, nframe=3,
                 answer=torch.zeros(2, 1, dtype=torch.long, device=dev), text_answer=[""] * 2, question=q.to(dev), question_attention_mask=qm.to(dev))
    m.fast_decode = False
    ref = m.eval_forward(batch)
    assert getattr(m, "_decoder", None) is None and ref.shape == (2, 11)
    m.fast_decode = True
    _refuse_hf(lm, monkeypatch)
    ids = m.eval_forward(batch)
    assert m._decoder.lora is not None and ids.tolist() == ref.tolist()
