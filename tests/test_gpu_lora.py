"""-m gpu: LoRA adapters on the Llama graph decoder.  The kernel (vtgb_llm_lora through ops.lora_update) is held to the rule of
tests/lora_refs.py -- the fp64 reference, a derived fp32 accumulation bound, monotone roundings; the decoder with adapters is compared
with HF generate over the train.LoraLinear model: token for token at fp32, at bf16 within twice the error the adapter-free decoder (the
parent's code) shows against its own fp32 HF model in the same run."""
import copy
import functools

import pytest
import torch

import lora_refs as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return "cuda:0"


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _on(dev, x, y, segs):
    """The case on the device with the host's strides (column slices of wider buffers)."""
    xd = torch.zeros(x.shape[0], x.stride(0), dtype=x.dtype, device=dev)[:, : x.shape[1]]
    yd = torch.zeros(y.shape[0], y.stride(0), dtype=y.dtype, device=dev)[:, : y.shape[1]]
    xd.copy_(x)
    yd.copy_(y)
    return xd, yd, [(c, A.to(dev), B.to(dev), s) for c, A, B, s in segs]


# -------------------------------------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("r", [1, 8, 64])
@pytest.mark.parametrize("K", [32, 4096])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_kernel_obeys_the_rule(dev, dtype, K, r):
    """rows 1 / 17 / 130 (one partial row tile; two full tiles and one row; seventeen tiles), scaling 4.0 / 0.3, two segments (n = 32 at
    column 0, n = 40 at column 64) of a 112-column y whose row stride is 120; x's row stride is K + 8."""
    from videotgb_amd import ops
    for rows in (1, 17, 130):
        for scaling in (4.0, 0.3):
            x, y, segs = R.make_case(dtype, K, r, rows, scaling)
            assert x.stride(0) == K + 8 and y.stride(0) == R.N_COLS + 8 and y.shape[1] == 112
            xd, yd, sd = _on(dev, x, y, segs)
            pad_before = yd.as_strided((rows, 8), (yd.stride(0), 1), yd.storage_offset() + R.N_COLS).clone()
            got = ops.lora_update(xd, yd, sd)
            assert got is yd
            why = R.verdict(x, y, segs, yd.cpu())
            assert why is None, (rows, scaling, why)
            assert not torch.equal(yd.cpu(), y)
            # the padding between rows is not y's: untouched as well
            assert torch.equal(yd.as_strided((rows, 8), (yd.stride(0), 1), yd.storage_offset() + R.N_COLS), pad_before)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("K,r", [(32, 1), (4096, 8), (4096, 64)])
def test_a_row_does_not_depend_on_the_batch(dev, dtype, K, r):
    """Row 0 of a 130-row call equals the 1-row call, and row 129 (alone in the last tile) the call on that row alone, bit for bit."""
    from videotgb_amd import ops
    x, y, segs = R.make_case(dtype, K, r, 130, 4.0, seed=1)
    xd, yd, sd = _on(dev, x, y, segs)
    full = ops.lora_update(xd, yd.clone(), sd)
    for m in (0, 129, 77):
        one = ops.lora_update(xd[m: m + 1], yd[m: m + 1].clone(), sd)
        assert torch.equal(_bits(one), _bits(full[m: m + 1])), m


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_zero_adapters_leave_y_bit_identical(dev, dtype):
    from videotgb_amd import ops
    x, y, segs = R.make_case(dtype, 4096, 8, 17, 4.0, seed=2)
    y[3, 5] = -0.0      # (y + 0 keeps y's bits for every finite y but -0: rnd(-0 + 0) = +0 -- which IS LoraLinear.forward's result)
    xd, yd, sd = _on(dev, x, y, [(c, A, torch.zeros_like(B), s) for c, A, B, s in segs])
    ops.lora_update(xd, yd, sd)
    want = y.clone()
    want[3, 5] = 0.0
    assert torch.equal(_bits(yd.cpu()), _bits(want))


def test_many_rows_one_segment_and_the_wrapper_refuses_what_the_library_refuses(dev):
    """A prefill-sized call (8193 rows: 1025 row tiles, one column chunk per segment) against the rule; then five segments, which the
    library rejects on the host (ValueError through _lib.check)."""
    from videotgb_amd import ops
    x, y, segs = R.make_case(torch.bfloat16, 64, 8, 8193, 4.0, seed=3, segments=((16, 72),))
    xd, yd, sd = _on(dev, x, y, segs)
    ops.lora_update(xd, yd, sd)
    assert R.verdict(x, y, segs, yd.cpu()) is None
    five = [(8 * i, sd[0][1], sd[0][2][:8].contiguous(), 1.0) for i in range(5)]
    with pytest.raises(ValueError, match="n_seg=5"):
        ops.lora_update(xd, yd, five)


# ------------------------------------------------------------------------------------------------------------------------------- decoder
B_, P_, N_ = 3, 9, 12
PADDED = [[1] * 9, [0, 0, 0] + [1] * 6, [1, 1, 0, 1, 1, 1, 0, 1, 1]]
BIG = dict(hidden_size=2048, intermediate_size=2048, num_attention_heads=16, num_key_value_heads=16, num_hidden_layers=2, vocab_size=320)


@functools.lru_cache(maxsize=None)
def _lm(dev, dtype, big=False, lora=True, std=0.3):
    from videotgb_amd import llm, train
    kw = BIG if big else dict(num_hidden_layers=3, num_key_value_heads=1)
    lm = llm.build_llama("tiny", dtype, dev, seed=3, **kw)
    if lora:
        train.apply_lora(lm)
        R.nonzero_lora_(lm, seed=5, std=std)
        lm.eval()
    return lm


def _emb(dev, H, dtype, seed=0, B=B_):
    return (torch.randn(B, P_, H, generator=torch.Generator().manual_seed(seed)) * 0.5).to(dev, dtype)


def _hf(lm, emb, mask, n=N_):
    return lm.generate(inputs_embeds=emb, attention_mask=mask, do_sample=False, max_new_tokens=n, min_new_tokens=n, use_cache=True)


@pytest.mark.parametrize("padded", [False, True])
def test_fp32_fused_decoder_ids_equal_hf_generate_over_the_lora_model(dev, padded):
    from videotgb_amd.decode import GreedyDecoder
    lm, emb = _lm(dev, torch.float32), _emb(dev, 32, torch.float32)
    mask = torch.tensor(PADDED, device=dev) if padded else torch.ones(B_, P_, dtype=torch.long, device=dev)
    ref = _hf(lm, emb, mask)
    dec = GreedyDecoder(lm)
    kw = dict(attention_mask=mask) if padded else {}
    out = dec.generate(emb, N_, **kw)
    (st,) = dec.graphs.values()
    assert st["attn"] is not None and st["graph"] is not None      # the fused step, replayed
    assert out.tolist() == ref.tolist()
    assert torch.equal(GreedyDecoder(lm).generate(emb, N_, use_graph=False, **kw), out)
    base = _lm(dev, torch.float32, lora=False)
    assert not torch.equal(GreedyDecoder(base).generate(emb, N_, **kw), out)


def _logits(dec, emb, use_graph):
    """Two tokens: (ids, the first token's logits, the logits of the one step after it -- replayed from the graph, or eager)."""
    rec, pick = {}, dec._pick

    def spy(st, logits, step):
        if torch.cuda.is_current_stream_capturing():
            rec["step"] = logits                       # the graph's own buffer: holds the last replay's logits afterwards
        elif "first" not in rec:
            rec["first"] = logits.float().clone()
        elif not use_graph:
            rec["step"] = logits
        return pick(st, logits, step)
    dec._pick = spy
    try:
        ids = dec.generate(emb, 2, use_graph=use_graph)
    finally:
        del dec._pick
    torch.cuda.synchronize()
    return ids, rec["first"], rec["step"].float().clone()


def _hf_logits(lm, emb, ids):
    """The same two logit rows from HF's forward of the model upcast to fp32, fed the decoder's own first token."""
    lm32 = copy.deepcopy(lm).float()
    with torch.no_grad():
        first = lm32(inputs_embeds=emb.float()).logits[:, -1]
        e2 = torch.cat([emb.float(), lm32.get_input_embeddings()(ids[:, :1])], 1)
        step = lm32(inputs_embeds=e2).logits[:, -1]
    return first, step


# lora_B of the accuracy comparison: N(0, 0.02), the size of the projections' own weights -- an update of the size of the base output or
# below (a trained adapter is a perturbation of its projection), so that "one more rounding of the same size" is what the adapter adds;
# N(0, 0.3) doubles q and v at hidden_size 2048 and would measure a different model's conditioning, not the adapter arithmetic
ACC_STD = 0.02


@pytest.mark.parametrize("big", [False, True])
def test_bf16_decoder_logits_against_the_fp32_model_and_graph_replay(dev, big):
    from videotgb_amd.decode import GreedyDecoder
    H = 2048 if big else 32
    emb = _emb(dev, H, torch.bfloat16, seed=1, B=4)
    errs = {}
    for name, lora in (("adapter-free", False), ("lora", True)):
        lm = _lm(dev, torch.bfloat16, big, lora, ACC_STD)
        dec = GreedyDecoder(lm)
        ids, first, step = _logits(dec, emb, True)
        (st,) = dec.graphs.values()
        assert st["attn"] is not None and st["graph"] is not None and ("sk_ws" in st) == big      # big: the skinny GEMMs, o / down deferred
        hf_first, hf_step = _hf_logits(lm, emb, ids)
        errs[name] = ((first - hf_first).abs().max().item(), (step - hf_step).abs().max().item())
        if lora:      # graph replay equals the eager step, bit for bit
            ids_e, first_e, step_e = _logits(GreedyDecoder(lm), emb, False)
            assert torch.equal(ids, ids_e) and torch.equal(first, first_e) and torch.equal(step, step_e)
            assert torch.equal(dec.generate(emb, N_), GreedyDecoder(lm).generate(emb, N_, use_graph=False))
    print(f"bf16 decoder vs its fp32 HF model (hidden {H}), max |logit error| (first token, replayed step): adapter-free "
          f"{errs['adapter-free'][0]:.4e} {errs['adapter-free'][1]:.4e}; with adapters {errs['lora'][0]:.4e} {errs['lora'][1]:.4e}")
    for k in (0, 1):
        assert errs["lora"][k] <= 2 * errs["adapter-free"][k], errs


@pytest.mark.parametrize("mode", [dict(weights="fp8"), dict(kv_cache="fp8"), dict(weights="fp8", kv_cache="fp8")])
@pytest.mark.parametrize("big", [False, True])
def test_fp8_modes_combine_with_adapters(dev, big, mode):
    from videotgb_amd.decode import GreedyDecoder
    H = 2048 if big else 32
    emb = _emb(dev, H, torch.bfloat16, seed=2, B=4)
    lm = _lm(dev, torch.bfloat16, big)
    dec = GreedyDecoder(lm, **mode)
    ids = dec.generate(emb, 16)
    (st,) = dec.graphs.values()
    assert st["graph"] is not None
    if big and "kv_cache" in mode:
        assert st["attn"] == "split_fp8"
    assert torch.equal(ids, GreedyDecoder(lm, **mode).generate(emb, 16, use_graph=False))
    assert not torch.equal(ids, GreedyDecoder(_lm(dev, torch.bfloat16, big, False), **mode).generate(emb, 16))


def test_the_hip_prefill_applies_the_adapters_like_the_torch_prefill(dev):
    """hidden 2048 prefills on libvtgb.so (bf16, plain and into the fp8 code caches); PREFILL_MAX_TOKENS = 0 forces the torch statement
    of the model.  The first token's logits of both agree to bf16 accuracy (a few 2^-8 of the largest logit; 5 % is the bound) and are
    several times further from the adapter-free model's."""
    from videotgb_amd.decode import GreedyDecoder
    emb = _emb(dev, 2048, torch.bfloat16, seed=4, B=4)
    lm, base = _lm(dev, torch.bfloat16, True), _lm(dev, torch.bfloat16, True, False)
    for mode in ({}, dict(kv_cache="fp8")):
        hip, tor, plain = GreedyDecoder(lm, **mode), GreedyDecoder(lm, **mode), GreedyDecoder(base, **mode)
        tor.PREFILL_MAX_TOKENS = 0
        assert hip._use_hip_prefill(emb, P_)
        a, b, c = (_logits(d, emb, False)[1] for d in (hip, tor, plain))
        scale = a.abs().max().item()
        print(f"first-token logits {mode}: hip vs torch prefill {(a - b).abs().max().item():.3e}, vs adapter-free {(a - c).abs().max().item():.3e}, max |logit| {scale:.3e}")
        ab, ac = (a - b).abs().max().item(), (a - c).abs().max().item()
        assert ab <= 0.05 * scale and ac >= 4 * ab and ac > 0      # (a prefill that dropped the adapters would give ac = 0 and a large ab)


def test_no_launch_without_adapters(dev, monkeypatch):
    """An adapter-free decoder never reaches vtgb_llm_lora (prefill, eager steps, capture, replay); a decoder with adapters does, so the
    counter counts."""
    from videotgb_amd import _lib as L, ops
    from videotgb_amd.decode import GreedyDecoder
    calls = []
    entry, update = L.lib().vtgb_llm_lora, ops.lora_update
    monkeypatch.setattr(L.lib(), "vtgb_llm_lora", lambda *a: (calls.append("entry"), entry(*a))[1])
    monkeypatch.setattr(ops, "lora_update", lambda *a: (calls.append("ops"), update(*a))[1])
    for dtype, big in ((torch.float32, False), (torch.bfloat16, True)):
        H = 2048 if big else 32
        dec = GreedyDecoder(_lm(dev, dtype, big, False))
        assert dec.lora is None
        dec.generate(_emb(dev, H, dtype), 4)
        dec.generate(_emb(dev, H, dtype), 4, use_graph=False)
        assert calls == []
        dec = GreedyDecoder(_lm(dev, dtype, big))
        dec.generate(_emb(dev, H, dtype), 4)
        layers = len(dec.layers)
        # prefill + the warm-up step + the captured step, one launch per layer each (q and v of a layer share a launch)
        assert calls.count("entry") == calls.count("ops") == 3 * layers, calls
        calls.clear()


# ---------------------------------------------------------------------------------------------------------------------- through the top
def test_lstp_generate_and_clip_session_with_adapters(dev, tiny_sd):
    """models.LSTP(..., lora=True) at fp32 with nonzero lora_B: generate on the graph decoder (fast_decode=True) equals HF generate over
    the LoraLinear model (fast_decode=False), and a clip session equals both."""
    from test_gpu_session import clip, questions
    from videotgb_amd import llm, models
    from videotgb_amd.decode import lora_state
    from videotgb_amd.synth import synth_tensor
    cfg, sd = tiny_sd["instructblip"]
    lm = llm.build_llama("tiny", torch.float32, dev)
    lm.load_state_dict({k: synth_tensor("model.language_model." + k, tuple(v.shape)).to(dev) for k, v in lm.state_dict().items()}, strict=True)
    base_ids = None
    T, nframe = 12, 4
    frames, flow_frames = clip(cfg, dev, T)
    (te, se, noise), = questions("instructblip", cfg, dev, [(5, 7, 4)], T)
    kw = dict(do_sample=False, temperature=None, max_new_tokens=12, min_new_tokens=12, noise=noise)
    m = models.LSTP(cfg, dev, False, language_model=lm, compute_dtype="f32")
    m.load_state_dict(sd, strict=False)
    m.to(dev)
    base_ids, _ = m.generate(frames, flow_frames, nframe, te, se, fast_decode=True, **kw)
    m = models.LSTP(cfg, dev, True, language_model=lm, compute_dtype="f32")      # wraps q_proj / v_proj of the same lm
    m.load_state_dict(sd, strict=False)
    m.to(dev)
    R.nonzero_lora_(m.model.language_model, seed=9)
    assert lora_state(m.model.language_model) == "ok"
    ref, cand_ref = m.generate(frames, flow_frames, nframe, te, se, fast_decode=False, **kw)
    ids, cand = m.generate(frames, flow_frames, nframe, te, se, fast_decode=True, **kw)
    assert m._decoder.lora is not None
    assert torch.equal(ids, ref) and torch.equal(cand, cand_ref), (ids.tolist(), ref.tolist())
    ids_s, cand_s = m.clip_session(frames, flow_frames).generate(nframe, te, se, fast_decode=True, **kw)
    assert torch.equal(ids_s, ref) and torch.equal(cand_s, cand_ref)
    auto, _ = m.generate(frames, flow_frames, nframe, te, se, **kw)
    assert torch.equal(auto, ref)
    assert not torch.equal(ids, base_ids)
