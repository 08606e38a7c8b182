"""-m gpu: beam search over the fp8 K/V cache (opt-in: beam_search="graph+kv8" with kv_cache="fp8"; ``GreedyDecoder(fp8_beams=True)``).
Every assertion is an equality with something the project already trusts.  The kernel, ops.decode_attention_beam_fp8
(vtgb_llm_decode_attention_beam_fp8): bit equality with ops.decode_attention_beam on the dequantised caches and with
ops.decode_attention(split=True) on the gathered dequantised cache (tests/beam_refs.py::gather_cache), over caches whose rows differ in
magnitude by 2^12 -- so neighbouring keys, and prompt and generated rows, carry different scales --, with every slot the contract calls
unread poisoned (the e4m3 NaN code, NaN scales, table entries outside the caches).  The decoder: strict equality with a bf16-cache beam
decoder whose attention calls see dq(q(K)), dq(q(V)); replay = eager steps = a repeat.  And a LightningModule twin with the shipped SF
``generate_configs``."""
import functools

import pytest
import torch
from torch.profiler import ProfilerActivity, profile

import beam_refs as R

pytestmark = pytest.mark.gpu

B, TMAX_P, TMAX_G = 2, 320, 64
NAN_CODE = 0x7F
KERNEL = "llm_decode_attn_beam_fp8_kernel"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return "cuda:0"


# ------------------------------------------------------------------------------------------------------------------------------- kernel
@functools.lru_cache(maxsize=None)
def _draw(dev, K, nq, nkv, hd):
    """q, the fp8 caches (codes as uint8, scales), their dequantised bf16 twins and the ancestry table; never modified."""
    from videotgb_amd import ops
    g = torch.Generator(device=dev).manual_seed(23 + K + nq + 3 * nkv + hd)
    Rr = B * K

    def rows(n, slots):      # N(0, 1) rows, each times 2^e with e uniform in -6 .. 6: the row scales span 2^12
        x = torch.randn(n, nkv, slots, hd, generator=g, device=dev)
        e = torch.randint(-6, 7, (n, nkv, slots, 1), generator=g, device=dev)
        return (x * torch.exp2(e.float())).bfloat16()

    def cache(n, slots):
        q8, s = ops.quantize_fp8_kv(rows(n, slots))
        return q8.view(torch.uint8).contiguous(), s.contiguous(), ops.dequantize_fp8_kv(q8, s).contiguous()
    q = torch.randn(Rr, nq * hd, generator=g, device=dev).bfloat16()
    (kp8, kps, kpd), (vp8, vps, vpd) = cache(B, TMAX_P), cache(B, TMAX_P)
    (kg8, kgs, kgd), (vg8, vgs, vgd) = cache(Rr, TMAX_G), cache(Rr, TMAX_G)
    # the scales do differ: between neighbouring keys, and between the prompt and the generated rows at one slot
    assert (kps[:, :, 1:] != kps[:, :, :-1]).float().mean() > 0.5 and (kgs[:, :, 1:] != kgs[:, :, :-1]).float().mean() > 0.5
    assert (kps[:1, :, :TMAX_G] != kgs[:1]).float().mean() > 0.5 and kps.max() / kps.min() >= 2 ** 8 and (kps != vps).float().mean() > 0.5
    # rows permuted within an item, independently per slot
    perm = torch.stack([torch.stack([torch.randperm(K, generator=g, device=dev) for _ in range(TMAX_G)], 1) for _ in range(B)])      # [B, K, tmax_g]
    src = (perm + (torch.arange(B, device=dev) * K)[:, None, None]).reshape(Rr, TMAX_G).int().contiguous()
    return q, (kp8, vp8, kps, vps, kg8, vg8, kgs, vgs), (kpd, vpd, kgd, vgd), src


def _masks(dev, K, n_prompt):
    """Leading pads, another count per item: key_valid [B, tmax_p] and its twin over the gathered cache."""
    kv = torch.ones(B, TMAX_P, dtype=torch.uint8, device=dev)
    for b in range(B):
        kv[b, : min(3 + 4 * b, n_prompt - 1)] = 0
    kv_full = torch.ones(B * K, TMAX_P + TMAX_G, dtype=torch.uint8, device=dev)
    kv_full[:, :TMAX_P] = kv.repeat_interleave(K, 0)
    kv_full[:, n_prompt:] = 1
    return kv, kv_full.contiguous()


def _poison(fp8, src, n_prompt, step, kv):
    """Everything the contract calls unread: the NaN code and a NaN scale in prompt slots >= n_prompt, in masked slots and in generated
    slots > step; table entries behind the step far outside [0, R)."""
    kp8, vp8, kps, vps, kg8, vg8, kgs, vgs = (t.clone() for t in fp8)
    nan = float("nan")
    for c, s in ((kp8, kps), (vp8, vps)):
        c[:, :, n_prompt:] = NAN_CODE
        s[:, :, n_prompt:] = nan
        if kv is not None:
            c.masked_fill_((kv == 0)[:, None, :, None], NAN_CODE)
            s.masked_fill_((kv == 0)[:, None, :], nan)
    for c, s in ((kg8, kgs), (vg8, vgs)):
        c[:, :, step + 1:] = NAN_CODE
        s[:, :, step + 1:] = nan
    src2 = src.clone()
    src2[:, step + 1:] = 1 << 20
    return (kp8, vp8, kps, vps, kg8, vg8, kgs, vgs), src2


def _check(dev, K, nq, nkv, hd, n_prompt, step, masked, identity=False):
    from videotgb_amd import ops
    q, fp8, (kpd, vpd, kgd, vgd), src = _draw(dev, K, nq, nkv, hd)
    Rr = B * K
    if identity:
        src = torch.arange(Rr, device=dev, dtype=torch.int32)[:, None].expand(Rr, TMAX_G).contiguous()
    kv, kv_full = _masks(dev, K, n_prompt) if masked else (None, None)
    scale = float(hd) ** -0.5
    n, pos = torch.tensor([n_prompt], device=dev), torch.tensor([n_prompt + step], device=dev)
    # the two references, from clean dequantised caches
    want_beam = ops.decode_attention_beam(q, kpd, vpd, kgd, vgd, src, n, pos, scale, key_valid=kv)
    want_split = ops.decode_attention(q, R.gather_cache(kpd, kgd, src, n_prompt, K), R.gather_cache(vpd, vgd, src, n_prompt, K), pos, scale,
                                      key_valid=kv_full, split=True)
    clean = ops.decode_attention_beam_fp8(q, *fp8, src, n, pos, scale, key_valid=kv)
    bad, src2 = _poison(fp8, src, n_prompt, step, kv)
    got = ops.decode_attention_beam_fp8(q, *bad, src2, n, pos, scale, key_valid=kv)
    where = (nq, nkv, hd, n_prompt, step, masked)
    assert torch.isfinite(got).all() and got.float().abs().sum() > 0, where
    assert torch.equal(got, clean), where                                                          # the poison changes nothing
    assert torch.equal(got, want_beam), (where, (got.float() - want_beam.float()).abs().max().item())
    assert torch.equal(got, want_split), (where, (got.float() - want_split.float()).abs().max().item())


# steps that put pos = n_prompt + step on both sides of a 256-key boundary (and the first and last slots)
STEPS = {1: (0, 1, 63), 250: (0, 5, 6, 63), 256: (0, 1, 63), 257: (0, 30)}


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("nq,nkv", [(4, 4), (8, 2), (16, 1)])
def test_equals_the_beam_and_the_split_attention_on_the_dequantised_caches(dev, hd, nq, nkv):
    for n_prompt, steps in STEPS.items():
        for step in steps:
            _check(dev, 3, nq, nkv, hd, n_prompt, step, masked=False)


@pytest.mark.parametrize("hd", [64, 128])
def test_masked_prompts_with_leading_pads(dev, hd):
    for n_prompt, steps in STEPS.items():
        for step in steps[:2]:
            _check(dev, 3, 8, 2, hd, n_prompt, step, masked=True)


@pytest.mark.parametrize("hd", [64, 128])
def test_one_beam_with_the_identity_table(dev, hd):
    for n_prompt in (250, 257):
        _check(dev, 1, 8, 2, hd, n_prompt, 6, masked=False, identity=True)
        _check(dev, 1, 8, 2, hd, n_prompt, 6, masked=True, identity=True)


def test_a_mixed_up_scale_would_show(dev):
    """(The caches are such that the equalities above test the scales: the same codes under the prompt's scales shifted by one key, or with the
    generated rows' V scales taken from the neighbouring cache row, give other numbers.)"""
    from videotgb_amd import ops
    K, nq, nkv, hd, n_prompt, step = 3, 8, 2, 128, 250, 30
    q, fp8, _, src = _draw(dev, K, nq, nkv, hd)
    kp8, vp8, kps, vps, kg8, vg8, kgs, vgs = fp8
    n, pos = torch.tensor([n_prompt], device=dev), torch.tensor([n_prompt + step], device=dev)
    want = ops.decode_attention_beam_fp8(q, *fp8, src, n, pos, float(hd) ** -0.5)
    shifted = ops.decode_attention_beam_fp8(q, kp8, vp8, kps.roll(1, 2).contiguous(), vps, kg8, vg8, kgs, vgs, src, n, pos, float(hd) ** -0.5)
    own_row = ops.decode_attention_beam_fp8(q, kp8, vp8, kps, vps, kg8, vg8, kgs, vgs.roll(1, 0).contiguous(), src, n, pos, float(hd) ** -0.5)
    assert not torch.equal(shifted, want) and not torch.equal(own_row, want)


def test_a_wrong_table_reads_inside_the_caches(dev):
    """Entries outside [0, R) within the step are clamped: the numbers are those of the clamped table."""
    from videotgb_amd import ops
    K, nq, nkv, hd, n_prompt, step = 3, 8, 2, 128, 250, 9
    q, fp8, _, src = _draw(dev, K, nq, nkv, hd)
    bad = src.clone()
    bad[::2, : step + 1] = -5
    bad[1::2, : step + 1] = 1 << 30
    n, p = torch.tensor([n_prompt], device=dev), torch.tensor([n_prompt + step], device=dev)
    got = ops.decode_attention_beam_fp8(q, *fp8, bad, n, p, float(hd) ** -0.5)
    want = ops.decode_attention_beam_fp8(q, *fp8, bad.clamp(0, B * K - 1), n, p, float(hd) ** -0.5)
    assert torch.isfinite(got).all() and torch.equal(got, want)
    assert not torch.equal(got, ops.decode_attention_beam_fp8(q, *fp8, src, n, p, float(hd) ** -0.5))


# ------------------------------------------------------------------------------------------------------------------------------ decoder
LAYERS, H, N = 2, 512, 8


def _build_lm(dev, kv_heads=2):
    from videotgb_amd import llm
    lm = llm.build_llama("tiny", torch.bfloat16, dev, seed=7, hidden_size=H, intermediate_size=1024, num_attention_heads=4,
                         num_key_value_heads=kv_heads, num_hidden_layers=LAYERS, vocab_size=320, max_position_embeddings=4096).eval()
    with torch.no_grad():
        lm.lm_head.weight.mul_(40.0)      # (unscaled, random-init logits are nearly flat and every beam ties)
    return lm


@functools.lru_cache(maxsize=None)
def _lm(dev, lora=False):
    lm = _build_lm(dev)
    if lora:
        import lora_refs
        from videotgb_amd import train
        train.apply_lora(lm)
        lora_refs.nonzero_lora_(lm, seed=5, std=0.3)
        lm.eval()
    return lm


def _call(dev, Bn, P, K):
    """Embeddings and a padded mask (leading pads, another count per row), the shipped penalties."""
    emb = (torch.randn(Bn, P, H, generator=torch.Generator(device=dev).manual_seed(4 + Bn + P), device=dev) * 0.5).bfloat16()
    am = torch.ones(Bn, P, dtype=torch.long, device=dev)
    for b in range(Bn):
        am[b, : (3, 0, 5)[b]] = 0
    return emb, dict(attention_mask=am, num_beams=K, repetition_penalty=1.5, length_penalty=1.0, eos_token_id=2, pad_token_id=0)


def _steps(dec, emb, use_graph, **kw):
    """generate: ids and the logits of every eagerly emitted step (under graph replay: the prefill's alone)."""
    rec, emit = [], dec._beam_emit

    def spy(st, logits):
        if not torch.cuda.is_current_stream_capturing() and (not use_graph or not rec):
            rec.append(logits.float().clone())
        return emit(st, logits)
    dec._beam_emit = spy
    try:
        ids = dec.generate(emb, N, use_graph=use_graph, **kw)
    finally:
        del dec._beam_emit
    return ids, rec


def _rounding_attention(monkeypatch):
    """Every attention a bf16-cache beam decoder calls sees dq(q(K)), dq(q(V)): the model of kv_cache="fp8" stated with the kernels the
    project already trusts (the prefill's two and the bf16 beam attention)."""
    from videotgb_amd import ops
    att, att_cached, att_beam = ops.attention, ops.attention_cached, ops.decode_attention_beam

    def attention(q, k, v, heads, scale, **kws):
        hd = q.shape[2] // heads
        r = lambda t: ops.fp8_kv_round(t.reshape(t.shape[0], t.shape[1], -1, hd)).reshape(t.shape)      # noqa: E731
        return att(q, r(k), r(v), heads, scale, **kws)

    def attention_cached(q, kc, vc, *a, **kws):
        return att_cached(q, ops.fp8_kv_round(kc), ops.fp8_kv_round(vc), *a, **kws)

    def decode_attention_beam(q, kp, vp, kg, vg, *a, **kws):
        return att_beam(q, *(ops.fp8_kv_round(t) for t in (kp, vp, kg, vg)), *a, **kws)
    monkeypatch.setattr(ops, "attention", attention)
    monkeypatch.setattr(ops, "attention_cached", attention_cached)
    monkeypatch.setattr(ops, "decode_attention_beam", decode_attention_beam)


def _check_decoder(dev, monkeypatch, lm, Bn, P, K, **dec_kw):
    from videotgb_amd.decode import GreedyDecoder
    emb, kw = _call(dev, Bn, P, K)
    dec = GreedyDecoder(lm, kv_cache="fp8", fp8_beams=True, **dec_kw)
    ids, rec = _steps(dec, emb, True, **kw)
    (st,) = dec.graphs.values()
    Rr, nkv, pst = Bn * K, lm.config.num_key_value_heads, st["prompt"]
    assert st["attn"] == "beam_fp8" and st["beam"]["kernel"] and st["graph"] is not None and "kg" not in st and "vg" not in st
    assert len(st["kg8"]) == len(st["vgs"]) == LAYERS and st["kg8"][0].dtype == st["vg8"][0].dtype == torch.uint8
    assert st["kg8"][0].shape == st["vg8"][0].shape == (Rr, nkv, st["tmax_g"], 128)
    assert st["kgs"][0].dtype == st["vgs"][0].dtype == torch.float32 and st["kgs"][0].shape == st["vgs"][0].shape == (Rr, nkv, st["tmax_g"])
    assert pst["attn"] == "split_fp8" and "kc" not in pst and pst["kc8"][0].shape == (Bn, nkv, pst["tmax"], 128) and pst["ks"][0].shape == (Bn, nkv, pst["tmax"])
    assert st["key_valid"] is pst["key_valid"] and st["kg8"][0][:, :, : ids.shape[1] - 1].any()
    assert torch.equal(dec.generate(emb, N, **kw), ids)                                    # the replay, repeated
    ids_e, rec_e = _steps(dec, emb, False, **kw)                                           # eager stepping
    assert torch.equal(ids_e, ids) and torch.equal(rec_e[0], rec[0]) and len(rec_e) >= 2
    plain = GreedyDecoder(lm, **dec_kw)                                                    # the bf16-cache beam decoder, as it is
    _, rec_p = _steps(plain, emb, False, **kw)
    assert not torch.equal(rec_e[1], rec_p[1])                                             # the switch matters (ids may coincide)
    _rounding_attention(monkeypatch)
    ref = GreedyDecoder(lm, **dec_kw)
    ids_r, rec_r = _steps(ref, emb, False, **kw)
    (st_r,) = ref.graphs.values()
    assert st_r["attn"] == "beam" and "kg" in st_r
    assert torch.equal(rec[0], rec_r[0]), (rec[0] - rec_r[0]).abs().max().item()           # first logits: the prefill
    assert torch.equal(ids, ids_r), (ids.tolist(), ids_r.tolist())
    assert len(rec_e) == len(rec_r) and all(torch.equal(a, b) for a, b in zip(rec_e, rec_r))      # and every later step's
    assert ids.shape[0] == Bn and 1 <= ids.shape[1] <= N


@pytest.mark.parametrize("K", [2, 5])
@pytest.mark.parametrize("P", [9, 300])
@pytest.mark.parametrize("Bn", [1, 3])
def test_decoder_equals_the_bf16_cache_beam_decoder_over_rounded_kv(dev, monkeypatch, Bn, P, K):
    _check_decoder(dev, monkeypatch, _lm(dev), Bn, P, K)


def test_fp8_weights_and_fp8_cache_together(dev, monkeypatch):
    _check_decoder(dev, monkeypatch, _lm(dev), 3, 300, 5, weights="fp8")


def test_lora_adapters(dev, monkeypatch):
    from videotgb_amd.decode import GreedyDecoder
    emb, kw = _call(dev, 3, 9, 5)
    base = GreedyDecoder(_lm(dev), kv_cache="fp8", fp8_beams=True).generate(emb, N, **kw)
    lm = _lm(dev, True)
    _check_decoder(dev, monkeypatch, lm, 3, 9, 5)
    monkeypatch.undo()
    assert not torch.equal(GreedyDecoder(lm, kv_cache="fp8", fp8_beams=True).generate(emb, N, **kw), base)      # (the adapters matter)


def test_the_torch_prefill_fills_the_code_caches(dev):
    """PREFILL_MAX_TOKENS = 0 forces the torch prefill into the prompt state's code caches; the beam steps stay on the fp8 kernels."""
    from videotgb_amd.decode import GreedyDecoder
    emb, kw = _call(dev, 3, 70, 2)
    dec = GreedyDecoder(_lm(dev), kv_cache="fp8", fp8_beams=True)
    dec.PREFILL_MAX_TOKENS = 0
    ids = dec.generate(emb, N, **kw)
    (st,) = dec.graphs.values()
    assert ids.shape[0] == 3 and st["attn"] == "beam_fp8" and st["graph"] is not None
    assert st["prompt"]["kc8"][0][:, :, :70].any() and not st["prompt"]["kc8"][0][:, :, 70:].any()


def test_what_stays_refused(dev):
    from videotgb_amd import llm
    from videotgb_amd.decode import GreedyDecoder
    lm = _lm(dev)
    x = torch.zeros(1, 4, H, device=dev, dtype=torch.bfloat16)
    for dec in (GreedyDecoder(lm, kv_cache="fp8"), GreedyDecoder(lm, kv_cache="fp8", fp8_beams=False)):
        with pytest.raises(NotImplementedError, match="kv_cache='fp8'"):
            dec.generate(x, 4, num_beams=2)
    dec = GreedyDecoder(lm, kv_cache="fp8", fp8_beams=True)
    with pytest.raises(NotImplementedError):
        dec.generate(x, 4, num_beams=2, do_sample=True)
    with pytest.raises(NotImplementedError):
        dec.generate(x, 4, num_beams=2, stop_ids=[[5, 6]])
    with pytest.raises(NotImplementedError):
        dec.generate(x, 4, num_beams=2, eos_token_id=[4, 5])
    small = llm.build_llama("tiny", torch.bfloat16, dev, seed=3)      # head_dim 16: the bf16 beam path's refusal, in its words
    with pytest.raises(NotImplementedError, match="head_dim"):
        GreedyDecoder(small, kv_cache="fp8", fp8_beams=True).generate(torch.zeros(1, 4, 32, device=dev, dtype=torch.bfloat16), 4, num_beams=2)
    # with a bf16 cache the flag is inert: the state, the launches and the ids of the plain beam decoder
    emb, kw = _call(dev, 3, 9, 5)
    a, b = GreedyDecoder(lm, fp8_beams=True), GreedyDecoder(lm)
    assert torch.equal(a.generate(emb, N, **kw), b.generate(emb, N, **kw))
    (sa,), (sb,) = a.graphs.values(), b.graphs.values()
    assert sa["attn"] == sb["attn"] == "beam" and sorted(k for k in sa) == sorted(k for k in sb) and "kg8" not in sa


# ------------------------------------------------------------------------------------------------------------------- a module twin
def _kernel_names(fn):
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, {e.key for e in prof.key_averages()}


class BE(dict):
    __getattr__ = dict.get


def _sf_module(dev, tmp_path, **kw):
    """test_gpu_beam_decode.py's SF twin (tiny fixtures, head_dim 64, lm_head x 40) at bf16: the fused fp8 cache takes a bf16 language model."""
    from conftest import full_state_dict, load_golden, write_hf_config
    from test_gpu_beam_decode import SHIPPED_SF
    from videotgb_amd import models, modules
    from videotgb_amd.synth import tiny_cfg
    cfg = tiny_cfg("instructblip")
    cfg.llm_hidden = 128      # two heads: head_dim 64
    base = write_hf_config(str(tmp_path / "instructblip-tiny"), "instructblip", cfg, "llama")
    sd = full_state_dict(cfg, models.build_language_model(models.load_hf_config(base, "instructblip")))
    raft_pth = str(tmp_path / "raft-things.pth")
    torch.save({"module." + k[len("of_extractor."):]: v for k, v in sd.items() if k.startswith("of_extractor.")}, raft_pth)
    proc = BE(tokenizer=BE(pad_token_id=0), batch_decode=lambda ids, skip_special_tokens=True: [" ".join(map(str, r)) for r in ids.tolist()])
    m = modules.LSTPSFModule(model_name_or_path=base, sampler_name_or_path=str(tmp_path / "no-bert-weights"), of_extractor_name_or_path=raft_pth,
                             temperature=1.0, generate_configs=dict(SHIPPED_SF), compute_dtype="bf16", processor=proc, tgb_cfg=cfg.tgb, **kw)
    m.load_state_dict(sd, strict=True)
    m.to(dev)
    with torch.no_grad():
        m.model.language_model.lm_head.weight.mul_(40.0)
    g = load_golden("tiny_modules")
    up4 = lambda q: q.float().repeat_interleave(4, -2).repeat_interleave(4, -1)      # noqa: E731
    Bn = 2
    batch = dict(frames=(up4(g["frames_q8"]) / 48).to(dev), nframe=int(g["nframe"]), of_lengths=g["of_lengths"].tolist(),
                 answer=torch.zeros(Bn, 1, dtype=torch.long, device=dev), text_answer=[""] * Bn,
                 sampler_question=g["sf_sampler_ids"].to(dev), sampler_question_attention_mask=g["sf_sampler_mask"].to(dev),
                 qformer_text=g["sf_qformer_ids"].to(dev), qformer_text_attention_mask=g["sf_qformer_mask"].to(dev),
                 question=g["sf_question"].to(dev), question_attention_mask=g["sf_question_mask"].to(dev),
                 of=(up4(g["of_q8"]) / 127).to(dev), of_mask=g["of_mask"].to(dev))
    return m, batch, g["sf_noise"].to(dev)


def test_sf_module_eval_forward_with_the_shipped_generate_configs(dev, tmp_path):
    """An SF twin with the literal shipped ``generate_configs``, kv_cache="fp8" and beam_search="graph+kv8" at bf16: eval_forward runs on the
    graph decoder, over the fp8 beam attention and without a BLAS kernel."""
    from test_gpu_beam_decode import SHIPPED_SF
    m, batch, noise = _sf_module(dev, tmp_path, kv_cache="fp8", beam_search="graph+kv8")
    assert m.generate_configs == SHIPPED_SF and m.kv_cache == "fp8" and m.beam_search == "graph+kv8"
    assert m.model.language_model.lm_head.weight.dtype == torch.bfloat16
    ids, names = _kernel_names(lambda: m.eval_forward(batch, noise=noise))
    dec = getattr(m, "_decoder", None)
    assert dec is not None and dec.kv_cache == "fp8" and dec.fp8_beams is True
    st = next(reversed(dec.graphs.values()))
    assert st["attn"] == "beam_fp8" and st["beam"]["K"] == 5 and st["prompt"]["attn"] == "split_fp8" and st["graph"] is not None
    assert ids.shape[0] == 2 and ids.shape[1] > 1
    assert any(KERNEL in n for n in names) and any("beam_row_kernel" in n for n in names), sorted(names)[:60]
    assert not any("llm_decode_attn_beam_kernel" in n for n in names)      # (the bf16 beam attention is not launched)
    blas = sorted(n for n in names if "Cijk_" in n)
    assert not blas, blas
    ids2, _ = _kernel_names(lambda: m.eval_forward(batch, noise=noise))
    assert ids2.tolist() == ids.tolist() and m._decoder is dec
