"""-m gpu: the decode step's split-KV attention (vtgb_llm_decode_attention_split behind ops.decode_attention) -- the kernel against fp64
torch and against the one-wave-per-head kernel on the same draw, its masked-key contract, its independence of batch, cache length and
head grouping (strict equality), and the Llama graph decoder on caches past 2048 slots, which the decode step refused before.

Tolerances are the project's for this operation (test_gpu_padded_decode.py): max |out - ref| <= 1e-5 (fp32) / 1e-2 (bf16) of max |ref|
against fp64 on N(0, 1) inputs; 3e-2 * max(1, |logits|max) between the fused and the torch arithmetic of a decoder
(test_decode.py::test_bf16_prefill_runs_on_libvtgb_and_matches_the_blas_path)."""
import copy
import functools
import math

import pytest
import torch
from torch.profiler import ProfilerActivity, profile

pytestmark = pytest.mark.gpu

LAYERS = 3
SPLIT_KERNEL, SINGLE_KERNEL = "llm_decode_attn_split_kernel", "llm_decode_attn_kernel"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return "cuda:0"


# ------------------------------------------------------------------------------------------------------------------------------ kernel
def _ref_decode_attn(q, kc, vc, kv, pos, nq, nkv, scale):
    """fp64 (test_gpu_padded_decode.py's reference): keys [0, pos] with kv != 0; a row without a valid key is 0"""
    B, hd = q.shape[0], kc.shape[-1]
    n = pos + 1
    ok = kv[:, :n] != 0                                                                  # [B, n]
    K = torch.nan_to_num(kc[:, :, :n].double()).repeat_interleave(nq // nkv, 1)
    V = torch.nan_to_num(vc[:, :, :n].double()).repeat_interleave(nq // nkv, 1)
    V = torch.where(ok[:, None, :, None], V, torch.zeros_like(V))
    s = torch.einsum("bhd,bhtd->bht", q.double().view(B, nq, hd), K) * scale
    s = s.masked_fill(~ok[:, None, :], float("-inf"))
    return torch.nan_to_num(torch.einsum("bht,bhtd->bhd", torch.softmax(s, -1), V)).reshape(B, nq * hd)


@functools.lru_cache(maxsize=None)
def _draw(dev, dtype, B, nq, nkv, hd, tmax, seed=0):
    g = torch.Generator(device=dev).manual_seed(1000 * seed + B + tmax + nq + 3 * nkv + hd)
    q = torch.randn(B, nq * hd, generator=g, device=dev).to(dtype)
    kc = torch.randn(B, nkv, tmax, hd, generator=g, device=dev).to(dtype)
    vc = torch.randn(B, nkv, tmax, hd, generator=g, device=dev).to(dtype)
    return q, kc, vc


def _past_pos_nan(kc, vc, pos):
    kc, vc = kc.clone(), vc.clone()
    kc[:, :, pos + 1:] = float("nan")
    vc[:, :, pos + 1:] = float("nan")
    return kc, vc


def _run(q, kc, vc, pos, key_valid=None, split=True):
    from videotgb_amd import ops
    return ops.decode_attention(q, kc, vc, torch.tensor([pos], device=q.device), float(kc.shape[-1]) ** -0.5, key_valid=key_valid, split=split)


def _err(out, ref):
    return ((out.double() - ref).abs().max() / ref.abs().max()).item()


def _err_rows(out, ref, nq):
    """worst (row, head): max |out - ref| over its channels, relative to its own max |ref|"""
    o, r = out.double().view(out.shape[0], nq, -1), ref.view(out.shape[0], nq, -1)
    return ((o - r).abs().amax(-1) / r.abs().amax(-1)).max().item()


TOL = {torch.float32: 1e-5, torch.bfloat16: 1e-2}
GEOMETRIES = [(4, 4), (4, 2), (4, 1), (16, 1)]      # heads per K/V head: 1, 2, 4 and 16 (two blocks of 8 query heads)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("nq,nkv", GEOMETRIES)
def test_split_kernel_vs_fp64_at_wave_chunk_and_old_limit_boundaries(dev, dtype, hd, nq, nkv):
    """tmax = 2112; 1 .. 2112 keys; the cache past *pos holds NaN.  2049 keys and more: refused before this kernel."""
    B, tmax = 2, 2112
    q, kc0, vc0 = _draw(dev, dtype, B, nq, nkv, hd, tmax)
    ones = torch.ones(B, tmax, dtype=torch.uint8, device=dev)
    for n_keys in (1, 63, 64, 65, 255, 256, 257, 2049, 2112):
        pos = n_keys - 1
        kc, vc = _past_pos_nan(kc0, vc0, pos)
        out = _run(q, kc, vc, pos)
        ref = _ref_decode_attn(q, kc, vc, ones, pos, nq, nkv, float(hd) ** -0.5)
        err = _err(out, ref)
        print(f"split {dtype} hd={hd} nq={nq} nkv={nkv} keys={n_keys}: err {err:.3e}")
        assert torch.isfinite(out).all(), n_keys
        assert err <= TOL[dtype], (n_keys, err)


@pytest.mark.parametrize("dtype,nq,nkv,hd", [(torch.bfloat16, 4, 2, 128), (torch.float32, 4, 1, 64)])
def test_split_kernel_vs_fp64_at_4096_keys(dev, dtype, nq, nkv, hd):
    B, tmax, pos = 2, 4096, 4095
    q, kc, vc = _draw(dev, dtype, B, nq, nkv, hd, tmax)
    out = _run(q, kc, vc, pos)
    ref = _ref_decode_attn(q, kc, vc, torch.ones(B, tmax, dtype=torch.uint8, device=dev), pos, nq, nkv, float(hd) ** -0.5)
    err = _err(out, ref)
    print(f"split {dtype} hd={hd} nq={nq} nkv={nkv} keys=4096: err {err:.3e}")
    assert err <= TOL[dtype], err
    with pytest.raises(NotImplementedError):      # the one-wave kernel ends at 2048 slots
        _run(q, kc, vc, pos, split=False)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("nq,nkv,hd", [(4, 2, 128), (4, 4, 64)])
@pytest.mark.parametrize("n_keys", [300, 2048])
def test_split_kernel_is_as_accurate_as_the_one_wave_kernel_on_the_same_draw(dev, dtype, nq, nkv, hd, n_keys):
    """Both kernels against fp64 on the same tensors (tmax = 2048, what both take): the split kernel's error may be at most 1.5 x the
    one-wave kernel's, as the global maximum and as the worst (row, head) relative to its own largest value -- the bound and the method
    of test_gpu_prefill_attention.py; the yardstick is measured on the draw the case uses because both metrics are extreme values that
    the roundings of a few outputs decide.  Both kernels keep scores, weights and sums in fp32 and round the output once; the split
    kernel adds one fp32 rescale per chunk."""
    B, tmax, pos = 2, 2048, n_keys - 1
    q, kc0, vc0 = _draw(dev, dtype, B, nq, nkv, hd, tmax, seed=1)
    kc, vc = _past_pos_nan(kc0, vc0, pos)
    ref = _ref_decode_attn(q, kc, vc, torch.ones(B, tmax, dtype=torch.uint8, device=dev), pos, nq, nkv, float(hd) ** -0.5)
    new, old = _run(q, kc, vc, pos, split=True), _run(q, kc, vc, pos, split=False)
    (err, base), (err_r, base_r) = (_err(new, ref), _err(old, ref)), (_err_rows(new, ref, nq), _err_rows(old, ref, nq))
    print(f"{dtype} hd={hd} nq={nq} nkv={nkv} keys={n_keys}: split err {err:.3e}, one-wave {base:.3e}, ratio {err / base:.3f}; "
          f"worst row {err_r:.3e}, one-wave {base_r:.3e}, ratio {err_r / base_r:.3f}")
    assert 0 < base <= TOL[dtype] and 0 < base_r
    assert err <= 1.5 * base, (err, base)
    assert err_r <= 1.5 * base_r, (err_r, base_r)


@pytest.mark.parametrize("dtype,nq,nkv,hd", [(torch.bfloat16, 4, 2, 128), (torch.float32, 4, 4, 64), (torch.bfloat16, 16, 1, 64)])
def test_masked_keys_get_no_weight_and_nan_pad_slots_do_not_leak(dev, dtype, nq, nkv, hd):
    B, tmax, pos = 4, 2112, 2100
    q, kc, vc = _draw(dev, dtype, B, nq, nkv, hd, tmax, seed=2)
    kc, vc = _past_pos_nan(kc, vc, pos)
    kv = torch.ones(B, tmax, dtype=torch.uint8, device=dev)
    kv[0, :37] = 0                       # left pads
    kv[1, 1900:2050] = 0                 # right pads of a prompt that ends at slot 2049
    kv[2, 100:130] = 0                   # a hole
    kv[2, 700] = 0
    kv[3, 256:512] = 0                   # a whole chunk in the middle
    scale = float(hd) ** -0.5
    ones = torch.ones_like(kv)
    plain = _run(q, torch.nan_to_num(kc), torch.nan_to_num(vc), pos)
    assert torch.equal(_run(q, torch.nan_to_num(kc), torch.nan_to_num(vc), pos, key_valid=ones), plain)      # all ones == NULL, bit for bit
    bad = kv[:, None, :, None] == 0
    kc[bad.expand_as(kc)] = float("nan")
    vc[bad.expand_as(vc)] = float("nan")
    out = _run(q, kc, vc, pos, key_valid=kv)
    ref = _ref_decode_attn(q, kc, vc, kv, pos, nq, nkv, scale)
    assert torch.isfinite(out).all()
    for b in range(B):
        err = _err(out[b:b + 1], ref[b:b + 1])
        print(f"masked {dtype} hd={hd} nq={nq} nkv={nkv} row {b}: err {err:.3e}")
        assert err <= TOL[dtype], (b, err)
    assert not torch.equal(out[3], plain[3])
    none = kv.clone()
    none[1].zero_()                      # a row without any valid key: zeros
    out = _run(q, kc, vc, pos, key_valid=none)
    assert torch.isfinite(out).all() and not out[1].any() and out[0].any()


@pytest.mark.parametrize("dtype,hd", [(torch.bfloat16, 128), (torch.float32, 64)])
def test_a_row_does_not_depend_on_batch_cache_length_or_head_grouping(dev, dtype, hd):
    nq, nkv, pos = 4, 2, 2070
    q, kc, vc = _draw(dev, dtype, 5, nq, nkv, hd, 2112, seed=3)
    kv = torch.ones(5, 2112, dtype=torch.uint8, device=dev)
    kv[1, 5:40] = 0
    out = _run(q, kc, vc, pos, key_valid=kv)
    assert torch.equal(_run(q, kc, vc, pos, key_valid=kv), out)                                                    # two runs
    alone = _run(q[1:2].contiguous(), kc[1:2].contiguous(), vc[1:2].contiguous(), pos, key_valid=kv[1:2].contiguous())
    assert torch.equal(alone[0], out[1])                                                                            # B = 5 vs B = 1
    kc2, vc2 = torch.zeros(5, nkv, 4096, hd, dtype=dtype, device=dev), torch.zeros(5, nkv, 4096, hd, dtype=dtype, device=dev)
    kc2[:, :, :2112], vc2[:, :, :2112] = kc, vc
    kv2 = torch.ones(5, 4096, dtype=torch.uint8, device=dev)
    kv2[:, :2112] = kv
    assert torch.equal(_run(q, kc2, vc2, pos, key_valid=kv2), out)                                                  # tmax = 2112 vs 4096
    rep = _run(q, kc.repeat_interleave(2, 1).contiguous(), vc.repeat_interleave(2, 1).contiguous(), pos, key_valid=kv)
    assert torch.equal(rep, out)                                                                                    # nkv = 2 vs replicated to 4
    assert out.float().abs().sum() > 0


# ----------------------------------------------------------------------------------------------------------------------------- decoder
@functools.lru_cache(maxsize=None)
def _lm(dev, kv_heads, dtype=torch.bfloat16):
    from videotgb_amd import llm
    return llm.build_llama("tiny", dtype, dev, seed=7, hidden_size=512, intermediate_size=1024, num_attention_heads=4,
                           num_key_value_heads=kv_heads, num_hidden_layers=LAYERS, vocab_size=320, max_position_embeddings=4096)


def _emb(dev, B, P, seed=4, dtype=torch.bfloat16):
    return (torch.randn(B, P, 512, generator=torch.Generator(device=dev).manual_seed(seed), device=dev) * 0.5).to(dtype)


def _kernel_names(fn):
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.key for e in prof.key_averages()}


def _steps(dec, emb, n, **kw):
    """eager generate: ids and the logits every token was picked from"""
    rec, pick = [], dec._pick
    dec._pick = lambda st, logits, step: rec.append(logits.float().clone()) or pick(st, logits, step)
    try:
        ids = dec.generate(emb, n, use_graph=False, **kw)
    finally:
        del dec._pick
    return ids, rec


def _gap_ulps(logits):
    """distance of the best two logits of row 0 in bf16 ulps at the best one's magnitude"""
    top = logits[0].topk(2).values.double()
    ulp = 2.0 ** (math.floor(math.log2(max(top[0].abs().item(), 2.0 ** -100))) - 7)
    return ((top[0] - top[1]) / ulp).item()


@functools.lru_cache(maxsize=None)
def _seed_without_a_tie(dev, kv_heads, P):
    """The first embedding seed from 4 (test_gpu_long_prefill.py's default draw) upward at which the token picked from the prefill is
    decided by no rounding, in the fused and in the torch decoder: best two logits at least 5 bf16 ulps apart, the rule of
    test_gpu_long_prefill.py::test_left_padded_long_batch.  -> (seed, the torch decoder's ids and per-step logits of two steps)"""
    from videotgb_amd.decode import GreedyDecoder
    lm = _lm(dev, kv_heads)
    for seed in range(4, 20):
        emb = _emb(dev, 1, P, seed=seed)
        (_, rec), (ids_t, rec_t) = _steps(GreedyDecoder(lm), emb, 2), _steps(GreedyDecoder(lm, fused=False), emb, 2)
        gaps = [_gap_ulps(r) for r in (rec[0], rec_t[0], rec[1], rec_t[1])]
        print(f"kv_heads={kv_heads} P={P} seed={seed}: best two logits apart, bf16 ulps: step 0 fused {gaps[0]:.1f} torch {gaps[1]:.1f}, "
              f"step 1 fused {gaps[2]:.1f} torch {gaps[3]:.1f}")
        if min(gaps[:2]) >= 5:
            return seed, ids_t, rec_t
    raise AssertionError("no seed in 4 .. 19 keeps the first token's best two logits 5 bf16 ulps apart")


def _expect_route(dec, st, P, N):
    """P + N = 2048 rounds to a cache of exactly 2048 slots, the last the one-wave kernel takes: DECODE_SPLIT_MIN_KEYS decides, and the
    state holds a workspace exactly when the split kernel runs.  From 2049 on only the split kernel is left."""
    tmax = -(-(P + N) // 64) * 64
    route = dec._attn_route(tmax)
    assert st["tmax"] == tmax and route in ("split", "single") and (tmax <= 2048 or route == "split")
    assert st["attn"] == route and ("attn_ws" in st) == (route == "split")      # the kernel the state's captured graph holds
    return route


@pytest.mark.parametrize("P", [2040, 2048])
@pytest.mark.parametrize("kv_heads", [4, 2])
def test_long_cache_decodes_under_graph_replay_on_the_split_kernel(dev, kv_heads, P):
    """bf16, B = 1, N = 8.  P = 2048: tmax = 2112, a cache the decode step refused before (NotImplementedError from the first replay).
    P = 2040: P + N = 2048 fills a 2048-slot cache to its last slot, the longest cache both kernels take; the kernel is the one
    DECODE_SPLIT_MIN_KEYS routes 2048 slots to, and everything else is asserted alike.

    The torch decoder (fused=False: F.linear + SDPA) is a second arithmetic; its step-1 logits -- the first step that runs decode
    attention -- are compared under the bound of that pair of arithmetics, given an equal first token.  The first token is the only one
    compared across arithmetics, so the embedding seed is the first one at which no rounding decides it (_seed_without_a_tie, which
    prints every seed's gaps); ids under graph replay and from eager steps come from the same kernels and are equal at any seed."""
    from videotgb_amd.decode import GreedyDecoder
    lm = _lm(dev, kv_heads)
    N = 8
    seed, ids_t, rec_t = _seed_without_a_tie(dev, kv_heads, P)
    emb = _emb(dev, 1, P, seed=seed)
    dec = GreedyDecoder(lm)
    ids = dec.generate(emb, N)
    (st,) = dec.graphs.values()
    assert ids.shape == (1, N) and st["graph"] is not None                                # replayed: the state's captured graph
    ran, other = (SPLIT_KERNEL, SINGLE_KERNEL) if _expect_route(dec, st, P, N) == "split" else (SINGLE_KERNEL, SPLIT_KERNEL)
    ids_e, rec = _steps(GreedyDecoder(lm), emb, N)
    assert torch.equal(ids_e, ids)                                                       # graph replay and eager steps: the same kernels
    for use_graph in (False, True):
        names = _kernel_names(lambda: dec.generate(emb, N, use_graph=use_graph))
        blas = sorted(n for n in names if "Cijk_" in n or "rocblas" in n.lower() or "hipblaslt" in n.lower())
        assert not blas, blas
        if not use_graph:
            assert any(ran in n for n in names) and not any(other in n for n in names), sorted(names)[:40]
            assert any("llm_decode_attn_combine" in n for n in names) == (ran == SPLIT_KERNEL)
    for s in range(2):
        print(f"kv_heads={kv_heads} P={P} seed={seed} step {s}: best two logits {_gap_ulps(rec[s]):.1f} bf16 ulps apart, |logits|max {rec[s].abs().max().item():.3f}, "
              f"fused vs torch differ by {(rec[s] - rec_t[s]).abs().max().item():.4f}")
    assert ids_t[0, 0].item() == ids[0, 0].item()
    assert (rec[1] - rec_t[1]).abs().max().item() <= 3e-2 * max(1.0, rec_t[1].abs().max().item())


@pytest.mark.parametrize("kind", ["unpadded", "left"])
def test_fp32_long_cache_ids_equal_hf_generate(dev, kind):
    """The fp32 exactness mode past 2048 slots: ids token for token those of HF generate under the same attention_mask."""
    from videotgb_amd.decode import GreedyDecoder
    lm = _lm(dev, 2, torch.float32)
    B, P, N = (1, 2050, 8) if kind == "unpadded" else (2, 2050, 8)
    emb = _emb(dev, B, P, seed=5, dtype=torch.float32)
    am = torch.ones(B, P, dtype=torch.long, device=dev)
    if kind == "left":
        am[0, :7] = 0
        am[1, :300] = 0
    dec = GreedyDecoder(lm)
    ref = lm.generate(inputs_embeds=emb, attention_mask=am, do_sample=False, max_new_tokens=N, min_new_tokens=N)
    out = dec.generate(emb, N, attention_mask=am if kind == "left" else None)
    (st,) = dec.graphs.values()
    assert st["tmax"] == 2112 and "attn_ws" in st and st["graph"] is not None and ("key_valid" in st) == (kind == "left")
    assert out.tolist() == ref.tolist()


def test_short_caches_stay_on_the_one_wave_kernel(dev):
    """P = 131, N = 8 (tmax = 192): the kernel of before and not the split one; a second decoder with DECODE_SPLIT_MIN_KEYS forced to 64
    runs the split kernel, and its step-1 logits are within the bound of two arithmetics of the first decoder's."""
    from videotgb_amd.decode import GreedyDecoder
    lm = _lm(dev, 4)
    emb = _emb(dev, 2, 131)
    dec = GreedyDecoder(lm)
    assert 384 <= dec.DECODE_SPLIT_MIN_KEYS <= 2112
    names = _kernel_names(lambda: dec.generate(emb, 8, use_graph=False))
    assert any(SINGLE_KERNEL in n for n in names) and not any(SPLIT_KERNEL in n for n in names)
    assert "attn_ws" not in next(iter(dec.graphs.values()))
    forced = GreedyDecoder(lm)
    forced.DECODE_SPLIT_MIN_KEYS = 64
    names = _kernel_names(lambda: forced.generate(emb, 8, use_graph=False))
    assert any(SPLIT_KERNEL in n for n in names) and not any(SINGLE_KERNEL in n for n in names)
    (ids_a, rec_a), (ids_b, rec_b) = _steps(dec, emb, 2), _steps(forced, emb, 2)
    assert torch.equal(rec_a[0], rec_b[0]) and torch.equal(ids_a[:, 0], ids_b[:, 0])      # the prefill is the same
    diff = (rec_a[1] - rec_b[1]).abs().max().item()
    print(f"step-1 logits, one-wave vs split kernel: differ by {diff:.5f}, |logits|max {rec_a[1].abs().max().item():.3f}")
    assert diff <= 3e-2 * max(1.0, rec_a[1].abs().max().item())


@pytest.mark.parametrize("P", [2040, 2048])
def test_fp8_weights_decode_long_caches_on_the_split_path(dev, P):
    """decode_weights="fp8", N = 4; P = 2048: tmax = 2112, the split path; P = 2040: a 2048-slot cache, on the kernel
    DECODE_SPLIT_MIN_KEYS routes it to.  The ids of the bf16 decoder on a model carrying the dequantised weights (the equality of
    test_gpu_fp8_decode.py: both stream the same numbers through the same kernels)."""
    from videotgb_amd import ops
    from videotgb_amd.decode import GreedyDecoder
    lm = _lm(dev, 2)
    ref = copy.deepcopy(lm)
    with torch.no_grad():
        for l in ref.model.layers:
            for part, names in ((l.self_attn, ("q_proj", "k_proj", "v_proj", "o_proj")), (l.mlp, ("gate_proj", "up_proj", "down_proj"))):
                for n in names:
                    w = getattr(part, n).weight
                    w.copy_(ops.dequantize_fp8_rows(*ops.quantize_fp8_rows(w)))
        ref.lm_head.weight.copy_(ops.dequantize_fp8_rows(*ops.quantize_fp8_rows(ref.lm_head.weight)))
    emb = _emb(dev, 1, P, seed=6)
    dec8, dec16 = GreedyDecoder(lm, weights="fp8"), GreedyDecoder(ref)
    out8, out16 = dec8.generate(emb, 4), dec16.generate(emb, 4)
    (st,) = dec8.graphs.values()
    assert "sk_ws" in st and st["graph"] is not None
    _expect_route(dec8, st, P, 4)
    assert out8.shape == (1, 4) and torch.equal(out8, out16), (out8.tolist(), out16.tolist())
