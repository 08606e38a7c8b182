"""-m gpu: chunked prefill of the Llama graph decoder -- bf16 prompts past PREFILL_MAX_TOKENS go through the layer stack in chunks of at
most PREFILL_CHUNK_TOKENS rows, every chunk attending over the KV cache (ops.attention_cached) -- on the tiny Llama of
test_gpu_long_prefill.py (hidden 512, 4 heads of 128, 3 layers, vocab 320).

Small chunks: a decoder with the instance attributes PREFILL_MAX_TOKENS = 100 and PREFILL_CHUNK_TOKENS = 128 prefills P = 300 in three
chunks (128, 128, 44 rows).  It is compared with the default decoder (one launch sequence, vtgb_attention_tiled) or with the torch route
(PREFILL_MAX_TOKENS = 0) under the bounds of test_gpu_long_prefill.py::_compare: KV caches within 3e-2 * max(1, |cache|max), first-token
logits within 3e-2 * max(1, |logits|max), the same first token.  The attention of the two bf16 sequences is bit-equal
(test_gpu_attention_cached.py); whether a vtgb_gemm row's bits depend on M is not established, so cache equality is printed, not asserted.

Where two arithmetics are compared on a token (chunked vs torch), the project's tie rule applies (test_gpu_decode_split.py::
_seed_without_a_tie, restated): a token counts where its best two logits are at least 5 bf16 ulps apart in both decoders."""
import functools
import math

import pytest
import torch
from torch.profiler import ProfilerActivity, profile

pytestmark = pytest.mark.gpu

LAYERS = 3
SMALL = dict(PREFILL_MAX_TOKENS=100, PREFILL_CHUNK_TOKENS=128)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return "cuda:0"


@functools.lru_cache(maxsize=None)
def _lm(dev, kv_heads, dtype=torch.bfloat16, lora=False):
    from videotgb_amd import llm
    lm = llm.build_llama("tiny", dtype, dev, seed=7, hidden_size=512, intermediate_size=1024, num_attention_heads=4,
                         num_key_value_heads=kv_heads, num_hidden_layers=LAYERS, vocab_size=320, max_position_embeddings=4096)
    if lora:      # q_proj / v_proj adapters with non-zero B (tests/lora_refs.py)
        import lora_refs as R
        from videotgb_amd import train
        train.apply_lora(lm)
        R.nonzero_lora_(lm, seed=5, std=0.3)
        lm.eval()
    return lm


def _emb(dev, B, P, seed=4, dtype=torch.bfloat16):
    return (torch.randn(B, P, 512, generator=torch.Generator(device=dev).manual_seed(seed), device=dev) * 0.5).to(dtype)


def _decoder(lm, attrs=None, **kw):
    from videotgb_amd.decode import GreedyDecoder
    dec = GreedyDecoder(lm, **kw)
    for k, v in (attrs or {}).items():
        setattr(dec, k, v)
    return dec


def _generate(dec, emb, n, **kw):
    """ids, the state used, the first token's logits, and which prefill ran ("hip" one-shot, "chunked", or "torch": ``_layer`` calls)"""
    seen, route = [], []
    head, hip, chunked, layer = dec._head, dec._prefill_hip, dec._prefill_chunked, dec._layer
    dec._head = lambda x: seen.append(head(x)) or seen[-1]
    dec._prefill_hip = lambda *a, **k: route.append("hip") or hip(*a, **k)
    dec._prefill_chunked = lambda *a, **k: route.append("chunked") or chunked(*a, **k)
    dec._layer = lambda x, *a, **k: (route.append("torch") if x.shape[1] > 1 else None) or layer(x, *a, **k)
    try:
        ids = dec.generate(emb, n, **kw)
    finally:
        del dec._head, dec._prefill_hip, dec._prefill_chunked, dec._layer
    (st,) = dec.graphs.values()      # a fresh decoder: the one state of this call
    assert len(set(route)) == 1, route
    return ids, st, seen[0].float(), route[0]


def _gap_ulps(row):
    """distance of the best two logits of one row in bf16 ulps at the best one's magnitude"""
    top = row.topk(2).values.double()
    ulp = 2.0 ** (math.floor(math.log2(max(top[0].abs().item(), 2.0 ** -100))) - 7)
    return ((top[0] - top[1]) / ulp).item()


def _compare(tag, a, b, P, valid=None, tokens="all"):
    """a, b = _generate(...) results of the decoder under test and of the reference: the bounds of test_gpu_long_prefill.py::_compare.
    ``tokens``: "all" -- the same first token in every row; "untied" -- in the rows the tie rule counts (5 bf16 ulps in both)."""
    (ia, sa, la, _), (ib, sb, lb, _) = a, b
    worst, equal = 0.0, True
    for li in range(LAYERS):
        for c in ("kc", "vc"):
            x, y = sa[c][li][:, :, :P].float(), sb[c][li][:, :, :P].float()           # [B, kv_heads, P, hd]
            if valid is not None:      # pad slots are never read; past layer 0 they hold each path's own finite filler
                assert torch.isfinite(x).all(), (c, li)
                x, y = x * valid[:, None, :, None], y * valid[:, None, :, None]
            d, scale = (x - y).abs().max().item(), max(1.0, y.abs().max().item())
            worst, equal = max(worst, d / scale), equal and torch.equal(x, y)
            assert d <= 3e-2 * scale, (c, li, d, scale)
    dl, sl = (la - lb).abs().max().item(), max(1.0, lb.abs().max().item())
    print(f"{tag}: caches differ by at most {worst:.3e} of their scale (bit-equal: {equal}); first-token logits differ by {dl:.4f}, "
          f"|logits|max {lb.abs().max().item():.3f} (bit-equal: {torch.equal(la, lb)})")
    assert dl <= 3e-2 * sl, (dl, sl)
    for r in range(la.shape[0]):
        ga, gb = _gap_ulps(la[r]), _gap_ulps(lb[r])
        if tokens == "untied":
            print(f"{tag}: row {r} best two logits apart, bf16 ulps: {ga:.1f} / {gb:.1f}")
        if tokens == "all" or min(ga, gb) >= 5:
            assert ia[r, 0].item() == ib[r, 0].item() == lb[r].argmax().item(), (r, ga, gb)


# ------------------------------------------------------------------------------------------------------------- chunked vs one-shot
@pytest.mark.parametrize("kv_heads", [4, 2])
def test_three_chunks_match_the_one_shot_prefill(dev, kv_heads):
    lm = _lm(dev, kv_heads)
    emb = _emb(dev, 2, 300)
    a, b = _generate(_decoder(lm, SMALL), emb, 4), _generate(_decoder(lm), emb, 4)
    assert a[3] == "chunked" and b[3] == "hip"
    _compare(f"chunked vs one-shot kv_heads={kv_heads}", a, b, 300)
    print(f"ids chunked {a[0].tolist()} one-shot {b[0].tolist()}")


def test_lora_adapters_on_the_chunked_route(dev):
    lm = _lm(dev, 2, lora=True)
    emb = _emb(dev, 2, 300)
    a, b = _generate(_decoder(lm, SMALL), emb, 4), _generate(_decoder(lm), emb, 4)
    assert a[3] == "chunked" and b[3] == "hip" and _decoder(lm).lora is not None
    _compare("lora, chunked vs one-shot", a, b, 300)
    plain = _generate(_decoder(_lm(dev, 2), SMALL), emb, 4)
    assert not torch.equal(plain[2], a[2])                                               # (the adapters act)


def test_fp8_weights_on_the_chunked_route(dev):
    lm = _lm(dev, 2)
    emb = _emb(dev, 2, 300)
    a, b = _generate(_decoder(lm, SMALL, weights="fp8"), emb, 4), _generate(_decoder(lm, weights="fp8"), emb, 4)
    assert a[3] == "chunked" and b[3] == "hip"
    _compare("decode_weights=fp8, chunked vs one-shot", a, b, 300)
    assert not torch.equal(_generate(_decoder(lm, SMALL), emb, 4)[2], a[2])              # (another model than the bf16 weights')


# --------------------------------------------------------------------------------------------------------------------- padded batch
@pytest.mark.parametrize("kv_heads", [4, 2])
def test_padded_batch_against_the_torch_route(dev, kv_heads):
    """B = 3, P = 300, left pads (0, 4, 9); the row without left pads is right-padded (its last 3 slots)."""
    lm = _lm(dev, kv_heads)
    B, P = 3, 300
    emb = _emb(dev, B, P, seed=14)
    am = torch.stack([torch.arange(P, device=dev) >= n for n in (0, 4, 9)]).long()
    am[0, -3:] = 0
    a = _generate(_decoder(lm, SMALL), emb, 4, attention_mask=am)
    b = _generate(_decoder(lm, dict(PREFILL_MAX_TOKENS=0)), emb, 4, attention_mask=am)
    assert a[3] == "chunked" and b[3] == "torch" and "key_valid" in a[1]
    _compare(f"padded, chunked vs torch kv_heads={kv_heads}", a, b, P, valid=am.float(), tokens="untied")
    for li in range(LAYERS):      # pad slots hold finite values
        assert torch.isfinite(a[1]["kc"][li]).all() and torch.isfinite(a[1]["vc"][li]).all()


# ------------------------------------------------------------------------------------------------------------------- the real threshold
def _kernel_names(fn):
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.key for e in prof.key_averages()}


def test_a_2100_token_prompt_prefills_on_libvtgb(dev):
    """Default attributes, B = 1, P = 2100 (chunks of 2048 and 52 rows), N = 4: no BLAS kernel, an attn_cached kernel ran, the decode
    state is the split kernel's, graph replay and eager steps give the same ids; against the torch route at the first embedding seed from
    4 upward whose first token no rounding decides (best two logits 5 bf16 ulps apart in both decoders): the same first token, first-token
    logits within 3e-2 * max(1, |logits|max)."""
    lm = _lm(dev, 2)
    P, N = 2100, 4
    for seed in range(4, 20):
        emb = _emb(dev, 1, P, seed=seed)
        a = _generate(_decoder(lm), emb, N)
        b = _generate(_decoder(lm, dict(PREFILL_MAX_TOKENS=0)), emb, N)
        gaps = (_gap_ulps(a[2][0]), _gap_ulps(b[2][0]))
        print(f"P={P} seed={seed}: best two logits apart, bf16 ulps: chunked {gaps[0]:.1f} torch {gaps[1]:.1f}")
        if min(gaps) >= 5:
            break
    else:
        raise AssertionError("no seed in 4 .. 19 keeps the first token's best two logits 5 bf16 ulps apart")
    assert a[3] == "chunked" and b[3] == "torch"
    assert a[1]["attn"] == "split" and a[1]["tmax"] == 2112 and a[1]["graph"] is not None
    diff = (a[2] - b[2]).abs().max().item()
    print(f"first-token logits, chunked vs torch: differ by {diff:.4f}, |logits|max {b[2].abs().max().item():.3f}")
    assert a[0][0, 0].item() == b[0][0, 0].item()
    assert diff <= 3e-2 * max(1.0, b[2].abs().max().item())
    dec = _decoder(lm)
    ids = dec.generate(emb, N)
    assert torch.equal(ids, a[0])
    assert torch.equal(dec.generate(emb, N, use_graph=False), ids)                        # graph replay and eager steps: the same kernels
    for use_graph in (False, True):
        names = _kernel_names(lambda: dec.generate(emb, N, use_graph=use_graph))
        blas = sorted(n for n in names if "Cijk_" in n or "rocblas" in n.lower() or "hipblaslt" in n.lower())
        assert not blas, blas
        assert any("attn_cached" in n for n in names), sorted(names)[:40]
        assert not any("attn_tiled" in n for n in names)


def test_a_16000_token_prompt_allocates_no_mask(dev):
    """The additive [1, 1, P, Tmax] mask of the torch route is 0.5 GB in bf16 at P = 16000 (and more while it is built): the chunked route
    never builds it.  Peak memory over the call stays under 400 MB (caches: 3 layers x 2 x 16064 x 512 bf16 = 99 MB, one chunk's
    activations and the embeddings a few tens of MB)."""
    lm = _lm(dev, 4)
    P = 16000
    emb = _emb(dev, 1, P)
    dec = _decoder(lm)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    ids, st, logits, route = _generate(dec, emb, 4)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print(f"P={P}: peak memory over generate {peak / 2**20:.0f} MiB, tmax {st['tmax']}")
    assert route == "chunked" and st["tmax"] == 16064 and st["attn"] == "split"
    assert ids.shape == (1, 4) and torch.isfinite(logits).all()
    assert peak < 400 * 2**20


# --------------------------------------------------------------------------------------------------------------------------- fp8 cache
def _reference_decoder(monkeypatch, lm, attrs):
    """test_gpu_kv_fp8.py::_reference_decoder with the chunked route's kernel added: a bf16-cache decoder on the split kernel from 64 slots
    whose attention calls -- ops.attention, ops.attention_cached, ops.decode_attention -- see dq(q(K)) and dq(q(V))."""
    from videotgb_amd import ops
    att, cached, dec_att = ops.attention, ops.attention_cached, ops.decode_attention

    def attention(q, k, v, heads, scale, **kws):
        hd = q.shape[2] // heads
        r = lambda t: ops.fp8_kv_round(t.reshape(t.shape[0], t.shape[1], -1, hd)).reshape(t.shape)
        return att(q, r(k), r(v), heads, scale, **kws)

    def attention_cached(q, kc, vc, q0, heads, scale, **kws):
        assert kws.get("scales") is None
        return cached(q, ops.fp8_kv_round(kc), ops.fp8_kv_round(vc), q0, heads, scale, **kws)

    def decode_attention(q, kc, vc, pos, scale, **kws):
        return dec_att(q, ops.fp8_kv_round(kc), ops.fp8_kv_round(vc), pos, scale, **kws)
    monkeypatch.setattr(ops, "attention", attention)
    monkeypatch.setattr(ops, "attention_cached", attention_cached)
    monkeypatch.setattr(ops, "decode_attention", decode_attention)
    ref = _decoder(lm, attrs)
    monkeypatch.setattr(ref, "DECODE_SPLIT_MIN_KEYS", 64, raising=False)
    return ref


@pytest.mark.parametrize("padded", [False, True])
def test_fp8_cache_equals_the_bf16_cache_decoder_over_rounded_kv(dev, monkeypatch, padded):
    from videotgb_amd import ops
    lm = _lm(dev, 2)
    B, P, N = 2, 300, 6
    emb = _emb(dev, B, P)
    kw = {}
    if padded:      # left pads in the first row, right pads in the last
        am = torch.ones(B, P, dtype=torch.long, device=dev)
        am[0, :3] = 0
        am[B - 1, -2:] = 0
        kw = dict(attention_mask=am)
    ids, st, logits, route = _generate(_decoder(lm, SMALL, kv_cache="fp8"), emb, N, **kw)
    assert route == "chunked" and st["attn"] == "split_fp8" and "kc" not in st and st["graph"] is not None
    ids_r, st_r, logits_r, route_r = _generate(_reference_decoder(monkeypatch, lm, SMALL), emb, N, use_graph=False, **kw)
    assert route_r == "chunked" and st_r["attn"] == "split" and "kc" in st_r
    assert torch.equal(logits, logits_r), (logits - logits_r).abs().max().item()
    assert torch.equal(ids, ids_r), (ids.tolist(), ids_r.tolist())
    for c8, sc in zip(st["kc8"] + st["vc8"], st["ks"] + st["vs"]):      # the written rows are fixed points of quantise o dequantise
        dq = ops.dequantize_fp8_kv(c8[:, :, :P].view(torch.float8_e4m3fn), sc[:, :, :P])
        q2, s2 = ops.quantize_fp8_kv(dq)
        assert dq.float().abs().sum() > 0 and torch.equal(ops.dequantize_fp8_kv(q2, s2), dq) and not c8[:, :, P + N:].any()


# ----------------------------------------------------------------------------------------------------------------------------- routing
def test_routing(dev):
    lm = _lm(dev, 2)
    x = _emb(dev, 1, 20)
    dec = _decoder(lm)
    assert dec.PREFILL_CHUNK_TOKENS == 2048
    assert dec._use_hip_prefill(x, 2048) and not dec._use_hip_prefill(x, 2049)            # the one-shot bound stays
    st = dict(tmax=4096, attn="split", kc=[None])                                          # (what the predicate reads of a state)
    assert dec._use_chunked_prefill(st, x, 2049) and not dec._use_chunked_prefill(st, x, 2048)
    assert dec._use_chunked_prefill(dict(st, tmax=16384), x, 16000)
    assert not dec._use_chunked_prefill(dict(st, tmax=16448, attn=None), x, 16400)       # a cache past 16384 slots
    assert not dec._use_chunked_prefill(st, x.float(), 2049) and not dec._use_chunked_prefill(st, x.cpu(), 2049)
    assert dec._use_chunked_prefill(dict(tmax=4096, attn="split_fp8", kc8=[None]), x, 2049)
    fp8 = _decoder(lm, kv_cache="fp8")
    assert fp8._use_chunked_prefill(dict(tmax=4096, attn="split_fp8", kc8=[None]), x, 2049)
    assert not fp8._use_chunked_prefill(dict(tmax=4096, attn=None, kc=[None]), x, 2049)  # the fallback state: bf16 caches of dequantised values
    assert not _decoder(lm, fused=False)._use_chunked_prefill(st, x, 2049)
    off = _decoder(lm, dict(PREFILL_MAX_TOKENS=0))
    assert not any(off._use_chunked_prefill(st, x, P) for P in (1, 300, 2049, 16000)) and not off._use_hip_prefill(x, 20)
    # ... and the calls themselves: PREFILL_MAX_TOKENS = 0 at a short and at a chunk-sized prompt, an fp32 model past its one-shot bound
    assert _generate(_decoder(lm, dict(PREFILL_MAX_TOKENS=0)), _emb(dev, 1, 60), 2)[3] == "torch"
    assert _generate(_decoder(lm, dict(PREFILL_MAX_TOKENS=0, PREFILL_CHUNK_TOKENS=128)), _emb(dev, 1, 300), 2)[3] == "torch"
    lm32 = _lm(dev, 2, torch.float32)
    assert _generate(_decoder(lm32), _emb(dev, 1, 1000, dtype=torch.float32), 2)[3] == "hip"
    assert _generate(_decoder(lm32), _emb(dev, 1, 1100, dtype=torch.float32), 2)[3] == "torch"
