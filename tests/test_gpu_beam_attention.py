"""-m gpu: ops.decode_attention_beam (vtgb_llm_decode_attention_beam) -- bit equality with ops.decode_attention(split=True) on the cache that
the gather of (prompt cache, generated cache, ancestry table) materialises (tests/beam_refs.py::gather_cache), with every slot the contract
calls unread filled with NaN: the prompt cache from *n_prompt on, the generated cache behind the step, masked prompt keys, and the
generated-cache rows of another batch item are never a beam's ancestors."""
import functools

import pytest
import torch

import beam_refs as R

pytestmark = pytest.mark.gpu

B, TMAX_P, TMAX_G = 2, 320, 64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return "cuda:0"


@functools.lru_cache(maxsize=None)
def _draw(dev, dtype, K, nq, nkv, hd):
    g = torch.Generator(device=dev).manual_seed(11 + K + nq + 3 * nkv + hd)
    Rr = B * K

    def rnd(*shape):
        return torch.randn(*shape, generator=g, device=dev).to(dtype)
    q = rnd(Rr, nq * hd)
    kp, vp = rnd(B, nkv, TMAX_P, hd), rnd(B, nkv, TMAX_P, hd)
    kg, vg = rnd(Rr, nkv, TMAX_G, hd), rnd(Rr, nkv, TMAX_G, hd)
    # rows permuted within an item, independently per slot
    perm = torch.stack([torch.stack([torch.randperm(K, generator=g, device=dev) for _ in range(TMAX_G)], 1) for _ in range(B)])      # [B, K, tmax_g]
    src = (perm + (torch.arange(B, device=dev) * K)[:, None, None]).reshape(Rr, TMAX_G).int().contiguous()
    return q, kp, vp, kg, vg, src


def _check(dev, dtype, K, nq, nkv, hd, n_prompt, step, masked, identity=False):
    from videotgb_amd import ops
    q, kp, vp, kg, vg, src = _draw(dev, dtype, K, nq, nkv, hd)
    Rr = B * K
    if identity:
        src = torch.arange(Rr, device=dev, dtype=torch.int32)[:, None].expand(Rr, TMAX_G).contiguous()
    pos = n_prompt + step
    kv = None
    if masked:      # leading pads, another count per item
        kv = torch.ones(B, TMAX_P, dtype=torch.uint8, device=dev)
        for b in range(B):
            kv[b, : min(3 + 4 * b, n_prompt - 1)] = 0
    # the materialised cache, from clean inputs
    kk, vv = R.gather_cache(kp, kg, src, n_prompt, K), R.gather_cache(vp, vg, src, n_prompt, K)
    kv_full = None
    if masked:
        kv_full = torch.ones(Rr, TMAX_P + TMAX_G, dtype=torch.uint8, device=dev)
        kv_full[:, :TMAX_P] = kv.repeat_interleave(K, 0)
        kv_full[:, n_prompt:] = 1
        kv_full = kv_full.contiguous()
    post = torch.tensor([pos], device=dev)
    want = ops.decode_attention(q, kk, vv, post, float(hd) ** -0.5, key_valid=kv_full, split=True)
    # NaN in everything the contract calls unread
    kp2, vp2, kg2, vg2 = kp.clone(), vp.clone(), kg.clone(), vg.clone()
    for t in (kp2, vp2):
        t[:, :, n_prompt:] = float("nan")
        if masked:
            t.masked_fill_((kv == 0)[:, None, :, None], float("nan"))
    for t in (kg2, vg2):
        t[:, :, step + 1:] = float("nan")
    src2 = src.clone()
    src2[:, step + 1:] = 1 << 20      # (a table entry behind the step is not read; one that were would be clamped)
    got = ops.decode_attention_beam(q, kp2, vp2, kg2, vg2, src2, torch.tensor([n_prompt], device=dev), post, float(hd) ** -0.5, key_valid=kv)
    assert torch.isfinite(got).all(), (n_prompt, step)
    assert torch.equal(got, want), (n_prompt, step, (got.float() - want.float()).abs().max().item())


# steps that put pos = n_prompt + step on both sides of a 256-key boundary (and the first and last slots)
STEPS = {1: (0, 1, 63), 250: (0, 5, 6, 63), 256: (0, 1, 63), 257: (0, 30)}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("nq,nkv", [(4, 4), (8, 2), (16, 1)])
def test_beam_attention_equals_split_attention_on_the_gathered_cache(dev, dtype, hd, nq, nkv):
    for n_prompt, steps in STEPS.items():
        for step in steps:
            _check(dev, dtype, 3, nq, nkv, hd, n_prompt, step, masked=False)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("hd", [64, 128])
def test_masked_prompts_with_leading_pads(dev, dtype, hd):
    for n_prompt, steps in STEPS.items():
        for step in steps[:2]:
            _check(dev, dtype, 3, 8, 2, hd, n_prompt, step, masked=True)


@pytest.mark.parametrize("dtype,hd", [(torch.bfloat16, 128), (torch.float32, 64)])
def test_one_beam_with_the_identity_table(dev, dtype, hd):
    for n_prompt in (250, 257):
        _check(dev, dtype, 1, 8, 2, hd, n_prompt, 6, masked=False, identity=True)
        _check(dev, dtype, 1, 8, 2, hd, n_prompt, 6, masked=True, identity=True)


def test_a_wrong_table_reads_inside_the_caches(dev):
    """Entries outside [0, R) are clamped: the numbers are those of the clamped table."""
    from videotgb_amd import ops
    dtype, K, nq, nkv, hd, n_prompt, step = torch.bfloat16, 3, 8, 2, 128, 250, 9
    q, kp, vp, kg, vg, src = _draw(dev, dtype, K, nq, nkv, hd)
    bad = src.clone()
    bad[::2, : step + 1] = -5
    bad[1::2, : step + 1] = 1 << 30
    n, p = torch.tensor([n_prompt], device=dev), torch.tensor([n_prompt + step], device=dev)
    got = ops.decode_attention_beam(q, kp, vp, kg, vg, bad, n, p, float(hd) ** -0.5)
    want = ops.decode_attention_beam(q, kp, vp, kg, vg, bad.clamp(0, B * K - 1), n, p, float(hd) ** -0.5)
    assert torch.equal(got, want)
