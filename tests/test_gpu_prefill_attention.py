"""-m gpu: vtgb_attention_tiled, the prefill's tiled causal attention (online softmax over 64-key tiles, grouped-query heads read in
place), against an fp64 torch softmax-attention on the same bf16 inputs.

Inputs.  One draw per (head_dim, kv_heads) from a fixed seed: Q, K, V ~ N(0, 1), [3, 1000, ...] bf16; every case takes its leading
batch rows and tokens.  Causal attention with Sq = Skv makes row q of every such case the same problem (keys 0 .. q), so one fp64
reference (1000 tokens) serves all sizes.

Error bound.  The metric is max |out - ref| / max |ref|.  The bound is not a constant: the single-pass kernel (vtgb_attention, called
with kv_heads = heads -- grouped K / V replicated for it --, Sq = Skv = 288, the leading 288 tokens of the same draw) is measured
against the same fp64 reference, and the tiled kernel may be at most 1.5 x that error at any size.  Both kernels round P to bf16 once
and the output once; the margin covers the extra fp32 rescale of the accumulator per key tile.  The yardstick runs on the same draw
because the metric is an extreme value that the bf16 rounding of the few largest outputs decides (half an ulp is 2^-7 for an output
in [2, 4) and 2^-6 in [4, 8), against max |ref| near 4): those sit in the first rows, where a query sees a handful of keys, and they
are the same numbers for both kernels only if both get the same rows.

Long key walks.  That metric is decided by the first rows and says little about a query that walks many key tiles (its outputs are
averages, an order of magnitude below max |ref|).  So every case is also measured PER ROW: max over the row's channels of
|out - ref|, relative to the row's own max |ref|, and the worst row counts.  The yardstick is the single-pass kernel's worst row over
its 288 rows, the bound again 1.5 x: a row's relative error comes from the same two roundings at any length (the output's, at most
2^-8 of the row's largest value, and P's, whose relative error per weight does not depend on how many weights there are), so a
kernel that loses or misweights a tile in a long walk (a missing 64-key tile of 1000 moves a row by several percent of its
scale) fails it by an order of magnitude."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

KT = 64                                   # the kernel's key tile (attn_tiled.hip)
SIZES = (289, 320, 3 * KT - 1, 3 * KT, 3 * KT + 1, 1000)
FMIN = torch.finfo(torch.float32).min


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


_DRAW = {}


def _qkv(dev, B, heads, kv_heads, hd, Sq, Skv):
    """the leading B rows / Sq, Skv tokens of the one fixed-seed draw of (hd, kv_heads): strided views, as the decoder passes them"""
    assert heads == 4 and B <= 3
    if (hd, kv_heads) not in _DRAW:
        g = torch.Generator(device=dev).manual_seed(0)
        _DRAW[hd, kv_heads] = tuple(torch.randn(3, max(SIZES), n * hd, generator=g, device=dev).bfloat16() for n in (4, kv_heads, kv_heads))
    q, k, v = _DRAW[hd, kv_heads]
    return q[:B, :Sq], k[:B, :Skv], v[:B, :Skv]


def _ref(q, k, v, heads, kv_heads, scale, valid=None):
    """fp64 causal softmax attention; ``valid`` [B, Skv] bool: the other keys are removed (their K / V rows may hold anything).
    Rows without any visible key come back as NaN."""
    B, Sq, D = q.shape
    Skv, hd = k.shape[1], D // heads
    Q = q.double().view(B, Sq, heads, hd).transpose(1, 2)
    K = torch.nan_to_num(k.double()).view(B, Skv, kv_heads, hd).transpose(1, 2).repeat_interleave(heads // kv_heads, 1)
    V = torch.nan_to_num(v.double()).view(B, Skv, kv_heads, hd).transpose(1, 2).repeat_interleave(heads // kv_heads, 1)
    s = Q @ K.transpose(-1, -2) * scale
    ar_q, ar_k = torch.arange(Sq, device=q.device)[:, None], torch.arange(Skv, device=q.device)[None, :]
    see = (ar_k <= ar_q + (Skv - Sq))[None, None]
    if valid is not None:
        see = see & valid[:, None, None, :]
    s = s.masked_fill(~see, float("-inf"))
    return (torch.softmax(s, -1) @ V).transpose(1, 2).reshape(B, Sq, D)


def _err(out, ref):
    return ((out.double() - ref).abs().max() / ref.abs().max()).item()


def _err_rows(out, ref):
    """worst row: max |out - ref| over a (batch, query) row's channels, relative to that row's max |ref|"""
    return ((out.double() - ref).abs().amax(-1) / ref.abs().amax(-1)).max().item()


_BASE, _REF = {}, {}


def _baseline(dev, hd, kv_heads):
    """error of the single-pass kernel at its largest size on the draw's leading 288 tokens, measured once and left unchanged"""
    if (hd, kv_heads) not in _BASE:
        from videotgb_amd import ops
        q, k, v = _qkv(dev, 2, 4, kv_heads, hd, 288, 288)
        rep = lambda t: t.reshape(2, 288, kv_heads, 1, hd).expand(2, 288, kv_heads, 4 // kv_heads, hd).reshape(2, 288, 4 * hd)
        out = ops.attention(q, rep(k), rep(v), 4, hd ** -0.5, causal=True)
        ref = _ref(q, k, v, 4, kv_heads, hd ** -0.5)
        _BASE[hd, kv_heads] = (_err(out, ref), _err_rows(out, ref))
    return _BASE[hd, kv_heads]


def _ref_rows(dev, hd, kv_heads, S):
    """rows 0 .. S-1 of the causal fp64 reference over the whole draw (row q sees keys 0 .. q whatever the size)"""
    if (hd, kv_heads) not in _REF:
        _REF[hd, kv_heads] = _ref(*_qkv(dev, 2, 4, kv_heads, hd, max(SIZES), max(SIZES)), 4, kv_heads, hd ** -0.5)
    return _REF[hd, kv_heads][:, :S]


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("kv_heads", [4, 2, 1])
@pytest.mark.parametrize("hd", [128, 64])
def test_tiled_attention_vs_fp64(dev, hd, kv_heads, S):
    from videotgb_amd import ops
    base, base_rows = _baseline(dev, hd, kv_heads)
    q, k, v = _qkv(dev, 2, 4, kv_heads, hd, S, S)
    out = ops.attention_tiled(q, k, v, 4, hd ** -0.5, kv_heads=kv_heads, causal=True)
    ref = _ref_rows(dev, hd, kv_heads, S)
    err, err_rows = _err(out, ref), _err_rows(out, ref)
    print(f"tiled hd={hd} kv_heads={kv_heads} S={S}: err {err:.3e}, single-pass (288 keys) {base:.3e}, ratio {err / base:.3f}; "
          f"worst row {err_rows:.3e}, single-pass {base_rows:.3e}, ratio {err_rows / base_rows:.3f}")
    assert torch.isfinite(out).all()
    assert 0 < base < 1e-2 and 0 < base_rows < 1e-2      # (the yardsticks themselves are bf16-rounding-sized errors)
    assert err <= 1.5 * base, (err, base)
    assert err_rows <= 1.5 * base_rows, (err_rows, base_rows)


@pytest.mark.parametrize("hd,kv_heads", [(128, 2), (64, 1)])
def test_fewer_queries_than_keys(dev, hd, kv_heads):
    """Sq < Skv: query q sees keys <= q + (Skv - Sq), as vtgb_attention's causal does"""
    from videotgb_amd import ops
    q, k, v = _qkv(dev, 2, 4, kv_heads, hd, 70, 330)
    out = ops.attention_tiled(q, k, v, 4, hd ** -0.5, kv_heads=kv_heads, causal=True)
    ref = _ref(q, k, v, 4, kv_heads, hd ** -0.5)
    (err, err_rows), (base, base_rows) = (_err(out, ref), _err_rows(out, ref)), _baseline(dev, hd, kv_heads)
    print(f"tiled hd={hd} kv_heads={kv_heads} Sq=70 Skv=330: err {err:.3e}, single-pass {base:.3e}; worst row {err_rows:.3e}, single-pass {base_rows:.3e}")
    assert err <= 1.5 * base, (err, base)
    assert err_rows <= 1.5 * base_rows, (err_rows, base_rows)


@pytest.mark.parametrize("S", [3 * KT + 1, 320])
@pytest.mark.parametrize("hd", [128, 64])
def test_grouped_heads_equal_replicated_heads_bit_for_bit(dev, hd, S):
    from videotgb_amd import ops
    q, k, v = _qkv(dev, 2, 4, 2, hd, S, S)
    rep = lambda t: t.reshape(2, S, 2, 1, hd).expand(2, S, 2, 2, hd).reshape(2, S, 4 * hd)
    a = ops.attention_tiled(q, k, v, 4, hd ** -0.5, kv_heads=2)
    b = ops.attention_tiled(q, rep(k), rep(v), 4, hd ** -0.5, kv_heads=4)
    assert torch.equal(a, b)
    k1, v1 = k[:, :, :hd].contiguous(), v[:, :, :hd].contiguous()                       # one K/V head for all four query heads
    rep4 = lambda t: t.repeat(1, 1, 4)
    assert torch.equal(ops.attention_tiled(q, k1, v1, 4, hd ** -0.5, kv_heads=1), ops.attention_tiled(q, rep4(k1), rep4(v1), 4, hd ** -0.5, kv_heads=4))


def _pad_masks(dev, S):
    """[3, S] bool: left pads over more than a key tile, right pads, a hole that swallows a whole key tile"""
    ar = torch.arange(S, device=dev)
    return torch.stack([ar >= KT + 6, ar < S - 50, (ar < KT + 26) | (ar >= 3 * KT + 8)])


@pytest.mark.parametrize("hd,kv_heads", [(128, 2), (64, 4)])
def test_row_does_not_depend_on_the_batch_or_the_run(dev, hd, kv_heads):
    from videotgb_amd import ops
    S = 300
    q, k, v = _qkv(dev, 3, 4, kv_heads, hd, S, S)
    for mask in (None, torch.where(_pad_masks(dev, S).roll(1, 0), 0.0, FMIN).float().contiguous()):
        run = lambda sl: ops.attention_tiled(q[sl], k[sl], v[sl], 4, hd ** -0.5, kv_heads=kv_heads, key_mask=None if mask is None else mask[sl].contiguous())
        a = run(slice(0, 3))
        assert torch.equal(a, run(slice(0, 3)))
        assert torch.equal(a[:1], run(slice(0, 1)))
        assert torch.equal(a[2:], run(slice(2, 3)))


@pytest.mark.parametrize("hd,kv_heads", [(128, 4), (128, 2), (64, 1)])
def test_key_mask_with_nan_in_the_pad_slots(dev, hd, kv_heads):
    """Left pads, right pads and a hole in the middle; the masked keys' K and V rows hold NaN.  The output is finite everywhere --
    also for the leading pads' queries, which see no valid key -- and equals the reference computed without the masked keys."""
    from videotgb_amd import ops
    S = 300
    q, k, v = _qkv(dev, 3, 4, kv_heads, hd, S, S)
    valid = _pad_masks(dev, S)
    k = torch.where(valid[..., None], k, torch.full_like(k, float("nan")))
    v = torch.where(valid[..., None], v, torch.full_like(v, float("nan")))
    mask = torch.where(valid, 0.0, FMIN).float().contiguous()
    out = ops.attention_tiled(q, k, v, 4, hd ** -0.5, kv_heads=kv_heads, key_mask=mask)
    assert torch.isfinite(out).all()
    ref = _ref(q, k, v, 4, kv_heads, hd ** -0.5, valid)
    has_key = torch.isfinite(ref).all(-1)                                               # [3, S]
    assert not has_key[0, : KT + 6].any() and has_key[0, KT + 6:].all() and has_key[1:].all()
    err = ((out.double() - ref)[has_key].abs().max() / ref[has_key].abs().max()).item()
    base = _baseline(dev, hd, kv_heads)[0]
    print(f"tiled masked hd={hd} kv_heads={kv_heads}: err {err:.3e}, single-pass {base:.3e}")
    assert err <= 1.5 * base, (err, base)


def test_ops_attention_routes_long_and_grouped_calls_to_the_tiled_kernel(dev):
    """head_dim 128, 320 keys, causal: past the single-pass kernel's LDS (this call raises without the tiled kernel); grouped heads at
    any length.  Calls the single-pass kernel takes stay on it."""
    from videotgb_amd import _lib, ops
    assert hasattr(_lib.lib(), "vtgb_attention_tiled")
    q, k, v = _qkv(dev, 2, 4, 4, 128, 320, 320)
    out = ops.attention(q, k, v, 4, 128 ** -0.5, causal=True)
    assert torch.equal(out, ops.attention_tiled(q, k, v, 4, 128 ** -0.5))
    assert _err(out, _ref(q, k, v, 4, 4, 128 ** -0.5)) <= 1.5 * _baseline(dev, 128, 4)[0]
    assert torch.equal(ops.attention(q, k, v, 4, 128 ** -0.5, causal=True, kv_heads=4), out)
    q, k, v = _qkv(dev, 2, 4, 2, 128, 20, 20)
    assert torch.equal(ops.attention(q, k, v, 4, 128 ** -0.5, causal=True, kv_heads=2), ops.attention_tiled(q, k, v, 4, 128 ** -0.5, kv_heads=2))
    with pytest.raises(NotImplementedError):                                            # not causal: the single-pass kernel's call, which has no grouped form
        ops.attention(q, k, v, 4, 128 ** -0.5, kv_heads=2)
    with pytest.raises(NotImplementedError):                                            # not causal, 320 keys: still beyond the single-pass kernel
        ops.attention(*_qkv(dev, 1, 4, 4, 128, 320, 320), 4, 128 ** -0.5)


def test_host_side_rejections(dev):
    from videotgb_amd import _lib as L, ops
    q, k, v = _qkv(dev, 1, 4, 2, 128, 320, 320)
    out = torch.empty_like(q)

    def call(**kw):
        d = dict(batch=1, heads=4, kv_heads=2, head_dim=128, s_q=320, s_kv=320, q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), q_tok_stride=512,
                 kv_tok_stride=256, q_batch_stride=320 * 512, kv_batch_stride=320 * 256, key_mask=None, scale=0.088, causal=1, out=out.data_ptr(),
                 out_tok_stride=512, out_batch_stride=320 * 512)
        d.update(kw)
        return L.lib().vtgb_attention_tiled(C.byref(L.AttentionTiledArgs(**d)), None)

    assert call(q=None) == -1 and call(out=None) == -1 and call(heads=4, kv_heads=3) == -1
    assert call(head_dim=96) == -4 and call(s_kv=4097) == -4
    with pytest.raises(NotImplementedError, match="head_dim"):
        ops.attention_tiled(*_qkv(dev, 1, 4, 4, 96, 320, 320), 4, 0.1)
    with pytest.raises(ValueError, match="kv_heads"):
        ops.attention_tiled(q, torch.cat([k, k[:, :, :128]], -1), torch.cat([v, v[:, :, :128]], -1), 4, 0.1, kv_heads=3)
    with pytest.raises(NotImplementedError, match="4096"):
        ops.attention_tiled(torch.zeros(1, 8, 64, device=dev).bfloat16(), *(torch.zeros(1, 4097, 64, device=dev).bfloat16() for _ in range(2)), 1, 0.1)
