"""-m gpu: the bf16 Llama prefill stays on libvtgb.so for prompts past 288 tokens and for grouped-query models (vtgb_attention_tiled
behind ops.attention).  A decoder forced to the torch path (PREFILL_MAX_TOKENS = 0: F.linear + SDPA, the arithmetic HF generate
runs) is the reference, with the bounds of test_decode.py::test_bf16_prefill_runs_on_libvtgb_and_matches_the_blas_path, which pins
the same pair of arithmetics: KV caches within 3e-2 of the cache's scale, first-token logits within 3e-2 of theirs and the same
first token."""
import functools

import pytest
import torch
from torch.profiler import ProfilerActivity, profile

pytestmark = pytest.mark.gpu

LAYERS = 3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return "cuda:0"


@functools.lru_cache(maxsize=None)
def _lm(dev, kv_heads):
    from videotgb_amd import llm
    return llm.build_llama("tiny", torch.bfloat16, dev, seed=7, hidden_size=512, intermediate_size=1024, num_attention_heads=4,
                           num_key_value_heads=kv_heads, num_hidden_layers=LAYERS, vocab_size=320)


def _emb(dev, B, P, seed=4):
    return (torch.randn(B, P, 512, generator=torch.Generator(device=dev).manual_seed(seed), device=dev) * 0.5).bfloat16()


def _pair(lm):
    from videotgb_amd.decode import GreedyDecoder
    own, blas = GreedyDecoder(lm), GreedyDecoder(lm)
    blas.PREFILL_MAX_TOKENS = 0
    return own, blas


def _generate(dec, emb, n, **kw):
    """ids, the state used and the first token's logits (what the prefill hands to the sampler)"""
    seen, head = [], dec._head
    dec._head = lambda x: seen.append(head(x)) or seen[-1]
    try:
        ids = dec.generate(emb, n, **kw)
    finally:
        del dec._head
    (st,) = dec.graphs.values()      # a fresh decoder: the one state of this call
    return ids, st, seen[0].float()


def _compare(own, blas, emb, P, valid=None, **kw):
    a, sa, la = _generate(own, emb, 4, **kw)
    b, sb, lb = _generate(blas, emb, 4, **kw)
    for li in range(LAYERS):
        for c in ("kc", "vc"):
            x, y = sa[c][li][:, :, :P].float(), sb[c][li][:, :, :P].float()           # [B, kv_heads, P, hd]
            if valid is not None:      # pad slots are never read (their keys carry no weight in either path); past layer 0 they hold each path's own finite filler
                assert torch.isfinite(x).all()
                x, y = x * valid[:, None, :, None], y * valid[:, None, :, None]
            assert (x - y).abs().max().item() <= 3e-2 * max(1.0, y.abs().max().item()), (c, li)
    assert (la - lb).abs().max().item() <= 3e-2 * max(1.0, lb.abs().max().item())
    assert a[:, 0].tolist() == b[:, 0].tolist() == lb.argmax(-1).tolist()
    return a


@pytest.mark.parametrize("B,P", [(2, 300), (1, 520)])
@pytest.mark.parametrize("kv_heads", [4, 2])
def test_long_and_grouped_prefill_runs_on_libvtgb_and_matches_the_torch_path(dev, kv_heads, B, P):
    own, blas = _pair(_lm(dev, kv_heads))
    emb = _emb(dev, B, P)
    assert own._use_hip_prefill(emb, P) and not blas._use_hip_prefill(emb, P)
    assert own._use_hip_prefill(emb[:, :20], 20) and own._use_hip_prefill(emb[:, :20], 2048) and not own._use_hip_prefill(emb[:, :20], 2049)
    _compare(own, blas, emb, P)


def _steps(dec, emb, n, **kw):
    """eager generate: ids and the logits every token was picked from"""
    rec, pick = [], dec._pick
    dec._pick = lambda st, logits, step: rec.append(logits.float().clone()) or pick(st, logits, step)
    try:
        ids = dec.generate(emb, n, use_graph=False, **kw)
    finally:
        del dec._pick
    return ids, rec


@pytest.mark.parametrize("kv_heads", [4, 2])
def test_left_padded_long_batch(dev, kv_heads):
    """B = 3, P = 300, ragged left padding (0, 4 and 9 pads): caches (valid slots) and first-token logits against the torch path under
    the same attention_mask; a padded row decodes the ids it decodes alone, unpadded -- strict equality, every row, every token.

    Alone, a row's keys fall into other 64-key tiles and its GEMM rows into other tiles: two bf16 roundings of the same logits, which
    here differ by up to 0.012 (1.5 bf16 ulps at the logits' scale of 1.3).  This tiny random-weight model's two best logits are often
    closer than that, and an exact bf16 tie decides differently in the two runs (the torch path has the same ties).  So the embedding
    seed and the token count are chosen where no step is near a tie: of seeds 1 .. 20 at 4 tokens, 15 give equal ids for both
    kv_heads, and the ids part only at steps whose best two logits are EQUAL in bf16 (seeds 3, 5, 12, 17 at kv_heads = 4, 19 at 2);
    seed 14 with 3 tokens keeps the best two at least 0.039 (5 ulps) apart at every step, in both runs, for both kv_heads.  The
    per-step logits of the two runs are bounded as well, with the bound of the torch-path comparison."""
    from videotgb_amd.decode import GreedyDecoder
    lm = _lm(dev, kv_heads)
    own, blas = _pair(lm)
    B, P, N = 3, 300, 3
    pads = (0, 4, 9)
    emb = _emb(dev, B, P, seed=14)
    am = torch.stack([torch.arange(P, device=dev) >= n for n in pads]).long()
    assert own._use_hip_prefill(emb, P)
    ids = _compare(own, blas, emb, P, valid=am.float(), attention_mask=am)[:, :N]
    ids_e, rec = _steps(GreedyDecoder(lm), emb, N, attention_mask=am)
    assert torch.equal(ids_e, ids)                                                      # graph replay and eager steps: the same kernels
    for b, n in enumerate(pads):
        alone, rec1 = _steps(GreedyDecoder(lm), emb[b: b + 1, n:].contiguous(), N)
        assert alone[0].tolist() == ids[b].tolist(), (b, alone.tolist(), ids[b].tolist())
        for s in range(N):
            la, lb = rec1[s][0], rec[s][b]
            diff, gap = (la - lb).abs().max().item(), (la.topk(2).values[0] - la.topk(2).values[1]).item()
            print(f"kv_heads={kv_heads} row {b} step {s}: logits differ by {diff:.4f}, best two alone {gap:.4f} apart")
            assert diff <= 3e-2 * max(1.0, la.abs().max().item()), (b, s, diff)


def _kernel_names(fn):
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.key for e in prof.key_averages()}


@pytest.mark.parametrize("kv_heads,B,P", [(2, 12, 20), (4, 2, 300)])
def test_generate_issues_no_blas_kernel_with_grouped_heads_or_a_long_prompt(dev, kv_heads, B, P):
    from videotgb_amd.decode import GreedyDecoder
    dec = GreedyDecoder(_lm(dev, kv_heads))
    emb = _emb(dev, B, P)
    dec.generate(emb, 4)                                   # capture outside the profile
    for use_graph in (False, True):
        names = _kernel_names(lambda: dec.generate(emb, 4, use_graph=use_graph))
        blas = sorted(n for n in names if "Cijk_" in n or "rocblas" in n.lower() or "hipblaslt" in n.lower())
        assert not blas, blas
        if not use_graph:                                  # (graph replays show up as one launch; the eager run names the kernels)
            assert any("attn_tiled" in n for n in names) and any("gemm_bf16" in n for n in names) and any("gemm_skinny" in n for n in names), sorted(names)[:40]
            assert not any("attn_bf16" in n for n in names)


def test_short_prompts_with_equal_heads_stay_on_the_single_pass_kernel(dev, monkeypatch):
    """P = 131, kv_heads = heads: the kernel of before (attn_bf16, not attn_tiled), and ids and caches bit-identical to a decoder whose
    ops.attention is called without kv_heads, i.e. the way it was called before the keyword existed."""
    from videotgb_amd import decode
    from videotgb_amd.decode import GreedyDecoder
    lm = _lm(dev, 4)
    emb = _emb(dev, 2, 131)
    dec = GreedyDecoder(lm)
    a = dec.generate(emb, 8)
    names = _kernel_names(lambda: dec.generate(emb, 8, use_graph=False))
    assert any("attn_bf16" in n for n in names) and not any("attn_tiled" in n for n in names)
    sa = next(iter(dec.graphs.values()))
    real = decode.ops.attention
    calls = []

    def before(q, k, v, heads, scale, key_mask=None, causal=False, kv_heads=None):
        calls.append(kv_heads)
        return real(q, k, v, heads, scale, key_mask=key_mask, causal=causal)

    monkeypatch.setattr(decode.ops, "attention", before)
    old = GreedyDecoder(lm)
    b = old.generate(emb, 8)
    sb = next(iter(old.graphs.values()))
    assert calls == [4] * LAYERS
    assert torch.equal(a, b)
    for li in range(LAYERS):
        assert torch.equal(sa["kc"][li][:, :, :131], sb["kc"][li][:, :, :131]) and torch.equal(sa["vc"][li][:, :, :131], sb["vc"][li][:, :, :131])
