"""-m gpu: padded prompt batches on the graph decoders -- the masked / per-row-position kernels against fp64 torch and HF's rotary
arithmetic, the decoders under hipGraph replay against HF generate with the same attention mask (fp32, 16 tokens), and the callers
that used to fall back to HF generate (LSTP.generate, clip sessions, the LightningModule twins, self-refinement)."""
import ctypes as C
import functools

import pytest
import torch
from torch.profiler import ProfilerActivity, profile

from conftest import deq, full_state_dict, load_golden, write_hf_config
from test_padded_decode import _masks, _tiny_t5

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tables(tmax, hd, dev, dtype):
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, device=dev, dtype=torch.float32) / hd))
    fr = torch.arange(tmax, device=dev, dtype=torch.float32)[:, None] * inv[None]
    emb = torch.cat((fr, fr), dim=-1)
    return emb.cos().to(dtype), emb.sin().to(dtype)


# ------------------------------------------------------------------------------------------------------------------------------ kernels
def _ref_decode_attn(q, kc, vc, kv, pos, nq, nkv, scale):
    B, hd = q.shape[0], kc.shape[-1]
    n = pos + 1
    ok = kv[:, :n] != 0                                                                  # [B, n]
    K = kc[:, :, :n].double().repeat_interleave(nq // nkv, 1)
    V = vc[:, :, :n].double().repeat_interleave(nq // nkv, 1)
    V = torch.where(ok[:, None, :, None], V, torch.zeros_like(V))
    s = torch.einsum("bhd,bhtd->bht", q.double().view(B, nq, hd), K) * scale
    s = s.masked_fill(~ok[:, None, :], float("-inf"))
    return torch.einsum("bht,bhtd->bhd", torch.softmax(s, -1), V).reshape(B, nq * hd)


@pytest.mark.parametrize("dtype,B,nq,nkv,hd,tmax,pos", [(torch.bfloat16, 128, 8, 2, 128, 2048, 1500), (torch.float32, 128, 8, 1, 128, 2048, 2047),
                                                        (torch.bfloat16, 5, 32, 32, 128, 64, 40), (torch.float32, 3, 4, 4, 64, 128, 100)])
def test_masked_decode_attention_vs_fp64_with_nan_pad_slots(dev, dtype, B, nq, nkv, hd, tmax, pos):
    from videotgb_amd import _lib as L
    g = torch.Generator(device=dev).manual_seed(B + tmax)
    code = L.BF16 if dtype == torch.bfloat16 else L.F32
    q = torch.randn(B, nq * hd, generator=g, device=dev).to(dtype)
    kc = torch.randn(B, nkv, tmax, hd, generator=g, device=dev).to(dtype)
    vc = torch.randn(B, nkv, tmax, hd, generator=g, device=dev).to(dtype)
    P = min(pos, 48)                                                                    # prompt part: left, right or middle pads per row
    kv = torch.ones(B, tmax, dtype=torch.uint8, device=dev)
    for b in range(B):
        npad = (b * 7) % (P - 1)
        start = (0, P - npad, (P - npad) // 2)[b % 3]
        kv[b, start:start + npad] = 0
    kc[kv[:, None, :, None].expand_as(kc) == 0] = float("nan")                        # pad slots hold garbage: must not leak
    vc[kv[:, None, :, None].expand_as(vc) == 0] = float("nan")
    kc[:, :, pos + 1:] = float("nan")                                                   # (and keys past *pos are never read)
    vc[:, :, pos + 1:] = float("nan")
    pos_t = torch.tensor([pos], device=dev)
    out = torch.empty(B, nq * hd, dtype=dtype, device=dev)
    scale = float(hd) ** -0.5
    L.check(L.lib().vtgb_llm_decode_attention_masked(code, q.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), pos_t.data_ptr(), kv.data_ptr(),
                                                      B, nq, nkv, hd, tmax, scale, _stream()))
    ref = _ref_decode_attn(q, kc, vc, kv, pos, nq, nkv, scale)
    assert torch.isfinite(out).all()
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    err = (out.double() - ref).abs().max().item()
    assert err <= tol * ref.abs().max().item(), err
    # every key valid: the masked entry is the unmasked one, bit for bit (same summation order)
    kc2, vc2 = torch.nan_to_num(kc), torch.nan_to_num(vc)
    ones = torch.ones_like(kv)
    a, b_ = torch.empty_like(out), torch.empty_like(out)
    L.check(L.lib().vtgb_llm_decode_attention_masked(code, q.data_ptr(), kc2.data_ptr(), vc2.data_ptr(), a.data_ptr(), pos_t.data_ptr(), ones.data_ptr(),
                                                      B, nq, nkv, hd, tmax, scale, _stream()))
    L.check(L.lib().vtgb_llm_decode_attention(code, q.data_ptr(), kc2.data_ptr(), vc2.data_ptr(), b_.data_ptr(), pos_t.data_ptr(), B, nq, nkv, hd, tmax,
                                              scale, _stream()))
    assert torch.equal(a, b_)
    # a row without any valid key stays finite (zeros)
    none = kv.clone()
    none[0].zero_()
    L.check(L.lib().vtgb_llm_decode_attention_masked(code, q.data_ptr(), kc.data_ptr(), vc.data_ptr(), a.data_ptr(), pos_t.data_ptr(), none.data_ptr(),
                                                      B, nq, nkv, hd, tmax, scale, _stream()))
    torch.cuda.synchronize()
    assert not a[0].any() and torch.isfinite(a).all()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_rope_cache_pos_is_hf_rotary_at_per_row_positions(dev, dtype):
    from videotgb_amd import _lib as L
    from videotgb_amd.decode import _rot_half
    B, nq, nkv, hd, tmax = 6, 8, 2, 128, 128
    g = torch.Generator(device=dev).manual_seed(1)
    code = L.BF16 if dtype == torch.bfloat16 else L.F32
    cos, sin = _tables(tmax, hd, dev, dtype)
    qkv = torch.randn(B, nq + 2 * nkv, hd, generator=g, device=dev).to(dtype)
    pos = torch.tensor([70], device=dev)
    off = torch.tensor([0, -3, -70, -12, -45, -1], device=dev)

    def run(fn_off):
        q = torch.zeros(B, nq * hd, dtype=dtype, device=dev)
        kc, vc = torch.zeros(B, nkv, tmax, hd, dtype=dtype, device=dev), torch.zeros(B, nkv, tmax, hd, dtype=dtype, device=dev)
        if fn_off is None:
            L.check(L.lib().vtgb_llm_rope_cache(code, qkv.data_ptr(), q.data_ptr(), kc.data_ptr(), vc.data_ptr(), cos.data_ptr(), sin.data_ptr(),
                                                pos.data_ptr(), B, nq, nkv, hd, tmax, _stream()))
        else:
            L.check(L.lib().vtgb_llm_rope_cache_pos(code, qkv.data_ptr(), q.data_ptr(), kc.data_ptr(), vc.data_ptr(), cos.data_ptr(), sin.data_ptr(),
                                                    pos.data_ptr(), fn_off.data_ptr(), B, nq, nkv, hd, tmax, _stream()))
        return q, kc, vc
    q, kc, vc = run(off)
    rp = pos + off
    c, s = cos[rp][:, None], sin[rp][:, None]
    qk = qkv[:, : nq + nkv]
    ref = qk * c + _rot_half(qk) * s                                                  # apply_rotary_pos_emb in the model's dtype
    assert torch.equal(q.view(B, nq, hd), ref[:, :nq])
    assert torch.equal(kc[:, :, 70], ref[:, nq:]) and torch.equal(vc[:, :, 70], qkv[:, nq + nkv:])
    assert not kc[:, :, :70].any() and not kc[:, :, 71:].any()
    for t0, t1 in zip(run(torch.zeros_like(off)), run(None)):                          # zero offsets: today's entry bit for bit
        assert torch.equal(t0, t1)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_rope_cache_prefill_pos_is_hf_rotary_and_leading_pads_stay_finite(dev, dtype):
    from videotgb_amd import _lib as L
    from videotgb_amd.decode import _rot_half
    B, S, nh, hd, tmax = 3, 21, 4, 128, 64
    g = torch.Generator(device=dev).manual_seed(2)
    code = L.BF16 if dtype == torch.bfloat16 else L.F32
    cos, sin = _tables(tmax, hd, dev, dtype)
    qkv = torch.randn(B, S, 3 * nh, hd, generator=g, device=dev).to(dtype)
    mask = _masks(B, S)["left"].to(dev)
    pid = (mask.cumsum(-1) - 1).masked_fill(mask == 0, 0)
    got = qkv.clone()
    kc, vc = torch.zeros(B, nh, tmax, hd, device=dev, dtype=dtype), torch.zeros(B, nh, tmax, hd, device=dev, dtype=dtype)
    L.check(L.lib().vtgb_llm_rope_cache_prefill_pos(code, got.data_ptr(), kc.data_ptr(), vc.data_ptr(), cos.data_ptr(), sin.data_ptr(), pid.data_ptr(),
                                                    B, S, nh, nh, hd, tmax, _stream()))
    qk = qkv[:, :, : 2 * nh]
    ref = qk * cos[pid][:, :, None] + _rot_half(qk) * sin[pid][:, :, None]
    assert torch.equal(got[:, :, : 2 * nh], ref) and torch.equal(kc[:, :, :S], ref[:, :, nh:].transpose(1, 2))
    # zero-based positions of an unpadded row: the existing entry, bit for bit
    ar = torch.arange(S, device=dev).expand(B, S).contiguous()
    a, b = qkv.clone(), qkv.clone()
    kc2 = torch.zeros_like(kc)
    L.check(L.lib().vtgb_llm_rope_cache_prefill_pos(code, a.data_ptr(), kc2.data_ptr(), vc.data_ptr(), cos.data_ptr(), sin.data_ptr(), ar.data_ptr(),
                                                    B, S, nh, nh, hd, tmax, _stream()))
    L.check(L.lib().vtgb_llm_rope_cache_prefill(code, b.data_ptr(), kc.data_ptr(), vc.data_ptr(), cos.data_ptr(), sin.data_ptr(), B, S, nh, nh, hd, tmax,
                                                _stream()))
    assert torch.equal(a, b) and torch.equal(kc, kc2)


@pytest.mark.parametrize("M", [1, 124])
def test_rope_cache_parts_pos_equals_its_two_launch_form(dev, M):
    from videotgb_amd import _lib as L, ops
    lib = L.lib()
    g = torch.Generator(device=dev).manual_seed(M)
    H, nq, hd, tmax = 4096, 32, 128, 128
    a = torch.randn(M, H, generator=g, device=dev).bfloat16()
    w = ops.SkinnyWeight((torch.randn(3 * H, H, generator=g, device=dev) * H ** -0.5).bfloat16())
    cos, sin = _tables(tmax, hd, dev, torch.bfloat16)
    pos = torch.tensor([90], device=dev)
    off = -torch.randint(0, 91, (M,), generator=g, device=dev)
    res = []
    for deferred in (False, True):
        q = torch.zeros(M, nq * hd, dtype=torch.bfloat16, device=dev)
        kc = torch.zeros(M, nq, tmax, hd, dtype=torch.bfloat16, device=dev)
        vc = torch.zeros_like(kc)
        if deferred:
            _, S, ws = ops.gemm_skinny(a, w, defer_reduce=True)
            assert S > 1
            L.check(lib.vtgb_llm_rope_cache_parts_pos(L.BF16, ws.data_ptr(), S, q.data_ptr(), kc.data_ptr(), vc.data_ptr(), cos.data_ptr(), sin.data_ptr(),
                                                      pos.data_ptr(), off.data_ptr(), M, nq, nq, hd, tmax, _stream()))
        else:
            qkv = ops.gemm_skinny(a, w)
            L.check(lib.vtgb_llm_rope_cache_pos(L.BF16, qkv.data_ptr(), q.data_ptr(), kc.data_ptr(), vc.data_ptr(), cos.data_ptr(), sin.data_ptr(),
                                                pos.data_ptr(), off.data_ptr(), M, nq, nq, hd, tmax, _stream()))
        res.append((q, kc, vc))
    for t0, t1 in zip(*res):
        assert torch.equal(t0, t1) and t0.abs().sum() > 0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_attention_rows_masked_vs_fp64(dev, dtype):
    """The T5 encoder's form (rows = B x P straight out of q|k|v, relative bias) with pad keys holding NaN."""
    from videotgb_amd import _lib as L
    B, P, H, dk = 4, 37, 4, 64
    HD = H * dk
    g = torch.Generator(device=dev).manual_seed(3)
    qkv = torch.randn(B * P, 3 * HD, generator=g, device=dev).to(dtype)
    bias = torch.randn(H, P, P, generator=g, device=dev).to(dtype)
    mask = _masks(B, P)["right"].to(dev)
    kv = mask.to(torch.uint8).contiguous()
    pad_rows = (mask.reshape(-1) == 0)
    qkv[pad_rows, HD:] = float("nan")
    out = torch.empty(B * P, HD, dtype=dtype, device=dev)
    a = L.LlmAttnRowsArgs(L.BF16 if dtype == torch.bfloat16 else L.F32, B * P, H, dk, P, P, P, 1.0, qkv.data_ptr(), 3 * HD, qkv[:, HD:].data_ptr(),
                          qkv[:, 2 * HD:].data_ptr(), P * 3 * HD, dk, 3 * HD, bias.data_ptr(), P, P * P, None, out.data_ptr(), HD)
    L.check(L.lib().vtgb_llm_attention_rows_masked(C.byref(a), kv.data_ptr(), P, _stream()))
    x = qkv.double().view(B, P, 3, H, dk)
    q, k, v = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)     # [B, H, P, dk]
    ok = mask[:, None, None, :] != 0
    rnd = (lambda t: t.to(dtype).double()) if dtype == torch.bfloat16 else (lambda t: t)    # HF's bf16 roundings: scores, + bias, weights
    s = rnd(rnd(q @ torch.nan_to_num(k).transpose(-1, -2)) + bias.double()[None])
    s = s.masked_fill(~ok, float("-inf"))
    ref = (rnd(torch.softmax(s, -1)) @ torch.nan_to_num(v)).transpose(1, 2).reshape(B * P, HD)
    assert torch.isfinite(out).all()
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    assert (out.double() - ref).abs().max().item() <= tol * ref.abs().max().item()


# ----------------------------------------------------------------------------------------------------------------------------- decoders
def _llama(dev, dtype=torch.float32, **kw):
    from videotgb_amd import llm
    return llm.build_llama("tiny", dtype, dev, seed=3, **kw)


@pytest.mark.parametrize("kv_heads", [1, 2])
@pytest.mark.parametrize("kind", ["left", "right", "mid"])
def test_llama_padded_graph_decode_equals_hf_generate(dev, kv_heads, kind):
    from videotgb_amd.decode import GreedyDecoder
    lm = _llama(dev, num_hidden_layers=3, num_key_value_heads=kv_heads)
    B, P, N = 5, 9, 16
    g = torch.Generator(device=dev).manual_seed(7)
    emb = torch.randn(B, P, 32, generator=g, device=dev) * 0.5
    am = _masks(B, P)[kind].to(dev)
    dec = GreedyDecoder(lm)
    ref = lm.generate(inputs_embeds=emb, attention_mask=am, do_sample=False, max_new_tokens=N, min_new_tokens=N)
    assert dec.generate(emb, N, attention_mask=am).tolist() == ref.tolist()
    am2 = am.flip(0)                                                                    # another ragged batch: the same graph, replayed
    ref2 = lm.generate(inputs_embeds=emb * 0.9, attention_mask=am2, do_sample=False, max_new_tokens=N, min_new_tokens=N)
    assert dec.generate(emb * 0.9, N, attention_mask=am2).tolist() == ref2.tolist()
    assert sum(1 for k in dec.graphs if k[-1]) == 1
    eos = int(ref[1, 3])
    ref3 = lm.generate(inputs_embeds=emb, attention_mask=am, do_sample=False, max_new_tokens=N, eos_token_id=eos, pad_token_id=0)
    assert dec.generate(emb, N, eos_token_id=eos, pad_token_id=0, attention_mask=am).tolist() == ref3.tolist()


def test_t5_padded_graph_decode_equals_hf_generate(dev):
    from videotgb_amd.decode import T5GreedyDecoder
    lm = _tiny_t5().to(dev)
    B, P, N = 4, 9, 16
    g = torch.Generator(device=dev).manual_seed(8)
    emb = torch.randn(B, P, 32, generator=g, device=dev) * 0.5
    dec = T5GreedyDecoder(lm)
    for kind, am in _masks(B, P).items():
        am = am.to(dev)
        ref = lm.generate(inputs_embeds=emb, attention_mask=am, do_sample=False, max_new_tokens=N, min_new_tokens=N)
        out = dec.generate(emb, N, attention_mask=am)
        assert out.tolist() == ref.tolist(), kind
    assert sum(1 for k in dec.graphs if k[-1]) == 1 and dec.graphs[next(k for k in dec.graphs if k[-1])]["hip"]


def _kernel_names(fn):
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.key for e in prof.key_averages()}


PADDED_KERNELS = ("llm_decode_attn_masked", "llm_rope_cache_pos", "llm_rope_cache_prefill_pos", "llm_attn_rows_masked")


@pytest.mark.parametrize("dtype,kv_heads", [(torch.bfloat16, 4), (torch.float32, 2)])
def test_padded_generate_runs_on_own_kernels_and_unpadded_on_the_old_ones(dev, dtype, kv_heads):
    from videotgb_amd.decode import GreedyDecoder
    lm = _llama(dev, dtype, hidden_size=512, intermediate_size=1024, num_attention_heads=4, num_key_value_heads=kv_heads, num_hidden_layers=2,
                vocab_size=256)
    B, P = 6, 12
    emb = (torch.randn(B, P, 512, device=dev, generator=torch.Generator(device=dev).manual_seed(9)) * 0.5).to(dtype)
    am = _masks(B, P)["right"].to(dev)
    dec = GreedyDecoder(lm)
    for use_graph in (False, True):
        names = _kernel_names(lambda: dec.generate(emb, 8, use_graph=use_graph, attention_mask=am))
        blas = sorted(n for n in names if "Cijk_" in n or "rocblas" in n.lower() or "hipblaslt" in n.lower())
        assert not blas, blas
        if not use_graph:
            assert all(any(k in n for n in names) for k in PADDED_KERNELS[:3]), sorted(names)[:60]
        names = _kernel_names(lambda: dec.generate(emb, 8, use_graph=use_graph))
        assert not any(k in n for n in names for k in PADDED_KERNELS), sorted(n for n in names if any(k in n for k in PADDED_KERNELS))


@pytest.mark.parametrize("kv_heads", [16, 4])
def test_bf16_padded_decode_ignores_what_the_pads_hold(dev, kv_heads):
    """Vicuna-width rows (hidden 2048: the skinny GEMM with deferred split-K reduction, HIP or eager-GQA prefill) at bf16: under left
    padding a row's ids do not depend on the pad positions' embeddings -- the pad keys get exactly no weight anywhere."""
    from videotgb_amd.decode import GreedyDecoder
    lm = _llama(dev, torch.bfloat16, hidden_size=2048, intermediate_size=5504, num_attention_heads=16, num_key_value_heads=kv_heads,
                num_hidden_layers=2, vocab_size=512)
    B, P, N = 8, 12, 12
    g = torch.Generator(device=dev).manual_seed(10)
    emb = torch.randn(B, P, 2048, generator=g, device=dev).bfloat16()
    am = _masks(B, P)["left"].to(dev)
    pads = (am == 0)[..., None]
    other = torch.where(pads, torch.randn(B, P, 2048, generator=g, device=dev).bfloat16() * 3 + 1, emb)
    dec = GreedyDecoder(lm)
    assert "sk_ws" in dec._state(B, P, N, dev, torch.bfloat16, padded=True)
    a = dec.generate(emb, N, attention_mask=am)
    b = dec.generate(other, N, attention_mask=am)
    assert torch.equal(a, b)
    st = dec.graphs[next(k for k in dec.graphs if k[-1])]
    # leading pads have no valid key: their attention rows stay finite, so layer 1's cache (built from layer 0's attention) is finite too
    assert len(st["kc"]) == 2 and all(torch.isfinite(c[:, :, :P]).all() for c in st["kc"] + st["vc"])


# ------------------------------------------------------------------------------------------------------------------------ end to end
def _padded_questions(arch, cfg, dev, T, lens=(7, 4, 5)):
    from test_gpu_session import BE, questions
    qs = questions(arch, cfg, dev, [(6, n, 4) for n in lens], T, seed=35)
    Pm = max(lens)
    ids = torch.zeros(len(lens), Pm, dtype=torch.long, device=dev)                      # the tokenizer's padding="longest", on the right
    mask = torch.zeros_like(ids)
    for i, (te, _, _) in enumerate(qs):
        ids[i, : lens[i]], mask[i, : lens[i]] = te["input_ids"][0], 1
    te = BE(input_ids=ids, attention_mask=mask)
    for k in ("qformer_input_ids", "qformer_attention_mask"):
        if k in qs[0][0]:
            te[k] = torch.cat([q[0][k] for q in qs])
    se = BE({k: torch.cat([q[1][k] for q in qs]) for k in qs[0][1]})
    noise = torch.cat([torch.stack([q[2][:, 0] for q in qs], 1), torch.stack([q[2][:, 1] for q in qs], 1)], 1)
    return te, se, noise


@pytest.mark.parametrize("arch", ["instructblip", "blip2"])
def test_generate_and_session_on_right_padded_questions(dev, tiny_sd, arch):
    from test_gpu_session import build, clip
    m, cfg, _ = build(arch, tiny_sd, dev, "f32")
    T, nframe, B = 12, 4, 3
    frames, flow_frames = clip(cfg, dev, T)
    te, se, noise = _padded_questions(arch, cfg, dev, T)
    kw = dict(do_sample=False, temperature=None, max_new_tokens=16, noise=noise)
    framesB, flowB = frames.repeat(B, 1, 1, 1), flow_frames.repeat(B, 1, 1, 1, 1)
    ref_ids, ref_cand = m.generate(framesB, flowB, nframe, te, se, fast_decode=False, **kw)
    ids, cand = m.generate(framesB, flowB, nframe, te, se, fast_decode=True, **kw)
    assert torch.equal(ids, ref_ids) and torch.equal(cand, ref_cand), (ids.tolist(), ref_ids.tolist())
    sess = m.clip_session(frames, flow_frames)
    ids2, cand2 = sess.generate(nframe, te, se, fast_decode=True, **kw)
    assert torch.equal(ids2, ref_ids) and torch.equal(cand2, ref_cand), (ids2.tolist(), ref_ids.tolist())


@pytest.mark.parametrize("tag", ["ib", "b2"])
def test_twin_eval_forward_on_right_padded_questions(dev, tmp_path, tag):
    from test_gpu_modules import CASES, up4
    from test_gpu_session import BE
    from videotgb_amd import models, modules
    from videotgb_amd.synth import tiny_cfg
    cls_name, arch, llm, uses_of = CASES[tag]
    cfg = tiny_cfg(arch)
    base = write_hf_config(str(tmp_path / f"{arch}-tiny"), arch, cfg, llm)
    sd = full_state_dict(cfg, models.build_language_model(models.load_hf_config(base, arch)))
    raft_pth = str(tmp_path / "raft-things.pth")
    torch.save({"module." + k[len("of_extractor."):]: v for k, v in sd.items() if k.startswith("of_extractor.")}, raft_pth)
    proc = BE(tokenizer=BE(pad_token_id=0), batch_decode=lambda ids, skip_special_tokens=True: [" ".join(map(str, r)) for r in ids.tolist()])
    m = getattr(modules, cls_name)(model_name_or_path=base, sampler_name_or_path=str(tmp_path / "no-bert-weights"),
                                   of_extractor_name_or_path=raft_pth, temperature=1.0,
                                   optimizer=functools.partial(torch.optim.AdamW, lr=1e-4), scheduler="cosine",
                                   scheduler_params={"warmup_steps": 0.1}, generate_configs=dict(do_sample=False, max_new_tokens=16),
                                   compute_dtype="f32", processor=proc, tgb_cfg=cfg.tgb)
    m.load_state_dict(sd, strict=True)
    m.to(dev)
    g = load_golden("tiny_modules")
    B = 2
    question, qmask = g[f"{tag}_question"].clone(), g[f"{tag}_question_mask"].clone()
    question[0, -2:], qmask[0, -2:] = 0, 0                                              # row 0 two tokens shorter, padded on the right
    batch = dict(frames=(up4(g["frames_q8"]) / 48).to(dev), nframe=int(g["nframe"]), of_lengths=g["of_lengths"].tolist(),
                 answer=torch.zeros(B, 1, dtype=torch.long, device=dev), text_answer=[""] * B,
                 sampler_question=g[f"{tag}_sampler_ids"].to(dev), sampler_question_attention_mask=g[f"{tag}_sampler_mask"].to(dev),
                 qformer_text=g[f"{tag}_qformer_ids"].to(dev), qformer_text_attention_mask=g[f"{tag}_qformer_mask"].to(dev),
                 question=question.to(dev), question_attention_mask=qmask.to(dev))
    noise = g[f"{tag}_noise"].to(dev) if f"{tag}_noise" in g else None
    m.fast_decode = False
    ref = m.eval_forward(batch, noise=noise)
    m.fast_decode = True
    calls = []
    from videotgb_amd import decode
    orig = decode.GreedyDecoder.generate if llm == "llama" else decode.T5GreedyDecoder.generate
    cls = decode.GreedyDecoder if llm == "llama" else decode.T5GreedyDecoder
    cls.generate = lambda self, *a, **k: calls.append(k.get("attention_mask")) or orig(self, *a, **k)
    try:
        got = m.eval_forward(batch, noise=noise)
    finally:
        cls.generate = orig
    assert len(calls) == 1 and calls[0] is not None                                       # the graph decoder ran, with the mask
    assert got.tolist() == ref.tolist()


def test_frame_answers_on_right_padded_questions_equal_hf(dev, tiny_sd):
    from test_gpu_e2e import build
    from videotgb_amd import refine
    m, cfg = build("instructblip", tiny_sd, dev, "f32")
    g = load_golden("tiny_instructblip_e2e")
    frames1 = deq(g, "frames_q8").to(dev)
    N, B = frames1.shape[0], 2
    frames = frames1.repeat(B, 1, 1, 1)
    q1, qt = g["prompt_ids"].to(dev), g["qformer_ids"].to(dev)
    L = q1.shape[1]
    q = torch.cat([q1, torch.cat([q1[:, : L - 2], torch.zeros(1, 2, dtype=q1.dtype, device=dev)], 1)])
    qm = torch.ones_like(q)
    qm[1, L - 2:] = 0
    qt2, qtm2 = qt.repeat(B, 1), g["qformer_mask"].to(dev).repeat(B, 1)
    max_length = 40
    got = refine.frame_answers(m, frames, B, qt2, qtm2, q, qm, max_length=max_length)
    enc = {"qformer_input_ids": torch.repeat_interleave(qt2, N, 0), "qformer_attention_mask": torch.repeat_interleave(qtm2, N, 0)}
    lm = m.model.language_model
    pre = m.prefix(frames, B * N, 1, enc, "mean")
    emb = torch.cat([pre, m.model.get_input_embeddings()(torch.repeat_interleave(q, N, 0))], 1)
    mask = torch.cat([torch.ones(B * N, pre.shape[1], dtype=torch.long, device=dev), torch.repeat_interleave(qm, N, 0)], 1)
    ref = lm.generate(inputs_embeds=emb, attention_mask=mask, do_sample=False, max_length=max_length)
    ref[ref == 0] = 2
    eos = lm.generation_config.eos_token_id
    for i in range(B * N):
        a, b = got[i].tolist(), ref[i].tolist()
        a = a[: a.index(eos) + 1] if eos in a else a
        b = b[: b.index(eos) + 1] if eos in b else b
        assert a == b, (i, a[:12], b[:12])
