"""-m gpu: vtgb_attention_cached, the chunked prefill's attention -- a chunk of queries at cache row q0 over the decoder's KV cache
[B, kv_heads, tmax, hd], bf16 or fp8 codes + scales -- alone.

Main statement, no tolerance: the kernel has vtgb_attention_tiled's tile partition and per-tile arithmetic, so its output is
``torch.equal`` to ``ops.attention_tiled`` with s_kv = q0 + s_q on the same K / V values laid out token-major, wherever that kernel takes
the call (up to 4096 keys); key_valid 0 corresponds to the hard fp32 key_mask (finfo(float32).min); an fp8 cache gives the bits of the
bf16 cache holding its dequantised values.  Unused cache rows -- from q0 + s_q on, and masked ones -- hold NaN (fp8: the e4m3 NaN code
and NaN scales): they are never read.

Past 4096 keys the tiled kernel refuses the call, and two checks take over.
 - Against an fp64 softmax attention on the same bf16 inputs, with the per-row metric and the rule of tests/test_gpu_prefill_attention.py,
   restated: a row's error is max over its channels of |out - ref| relative to the row's own max |ref|, the worst row counts, and it may be
   at most 1.5 x the single-pass kernel's (vtgb_attention, 288 keys, the leading 288 tokens of the same draw) worst row measured in the same
   run.  Both kernels round P to bf16 once and the output once; a row's relative error comes from those two roundings at any length (the
   output's, at most 2^-8 of the row's largest value, and P's, whose relative error per weight does not depend on the number of weights);
   the margin covers the extra fp32 rescale of the accumulator per key tile.  A lost or misweighted 64-key tile moves a row by percents.
 - An exact one from the online update: a fully masked tile leaves m = -inf, l = 0, O = 0 -- bit for bit the initial state.  With
   key_valid zero for keys 0 .. 12287, the (q0, s_q) = (16320, 64) output equals ops.attention_tiled over keys 12288 .. (4096 keys,
   s_q 64): the kept keys start on a tile boundary, so the partitions coincide."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

KT = 64
HEADS = 4
FMIN = torch.finfo(torch.float32).min
NAN8 = 0x7F                               # the e4m3fn NaN code
CASES = [(0, 300), (128, 128), (70, 45), (63, 2), (64, 1), (65, 130), (1000, 24)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _draw(dev, hd, kv_heads, S=1024, B=3):
    """one fixed-seed N(0, 1) bf16 draw per (hd, kv_heads): q [B, S, 4 hd], k / v [B, S, kv_heads hd], token-major"""
    g = torch.Generator(device=dev).manual_seed(0)
    return tuple(torch.randn(B, S, n * hd, generator=g, device=dev).bfloat16() for n in (HEADS, kv_heads, kv_heads))


def _cache(x, kv_heads, tmax, n):
    """token-major [B, >= n, kv_heads hd] -> cache [B, kv_heads, tmax, hd] holding rows 0 .. n-1; every other row is NaN"""
    B, hd = x.shape[0], x.shape[2] // kv_heads
    c = torch.full((B, kv_heads, tmax, hd), float("nan"), dtype=x.dtype, device=x.device)
    c[:, :, :n] = x[:, :n].view(B, n, kv_heads, hd).transpose(1, 2)
    return c


def _up64(n):
    return -(-n // KT) * KT


def _call(dev, hd, kv_heads, q0, sq, B=2, tmax=None, valid=None):
    """(cached, tiled) on the draw's leading B rows: queries q0 .. q0+sq-1, keys 0 .. q0+sq-1; valid [B, q0+sq] bool or None"""
    from videotgb_amd import ops
    q, k, v = (t[:B] for t in _draw(dev, hd, kv_heads))
    n = q0 + sq
    tmax = _up64(n) if tmax is None else tmax
    qs = q[:, q0:n]
    key_valid = key_mask = None
    kk, vv = k[:, :n], v[:, :n]
    if valid is not None:
        key_valid = torch.ones(B, tmax, dtype=torch.uint8, device=dev)
        key_valid[:, :n] = valid
        key_mask = torch.where(valid, 0.0, FMIN).float().contiguous()
        nan = lambda t: torch.where(valid[..., None], t, torch.full_like(t, float("nan")))
        kk, vv = nan(kk), nan(vv)
    out = ops.attention_cached(qs, _cache(kk, kv_heads, tmax, n), _cache(vv, kv_heads, tmax, n), q0, HEADS, hd ** -0.5, key_valid=key_valid)
    ref = ops.attention_tiled(qs, kk, vv, HEADS, hd ** -0.5, kv_heads=kv_heads, key_mask=key_mask, causal=True)
    return out, ref


@pytest.mark.parametrize("q0,sq", CASES)
@pytest.mark.parametrize("kv_heads", [4, 2, 1])
@pytest.mark.parametrize("hd", [128, 64])
def test_bit_equal_to_the_tiled_kernel(dev, hd, kv_heads, q0, sq):
    out, ref = _call(dev, hd, kv_heads, q0, sq)
    assert out.shape == ref.shape == (2, sq, HEADS * hd) and torch.isfinite(out).all()
    assert torch.equal(out, ref)


@pytest.mark.parametrize("q0,sq", [(70, 45), (128, 128)])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("hd", [128, 64])
def test_fp8_cache_equals_the_bf16_cache_of_its_values(dev, hd, q0, sq, masked):
    from videotgb_amd import ops
    kv_heads, B = 2, 2
    q, k, v = (t[:B] for t in _draw(dev, hd, kv_heads))
    n = q0 + sq
    tmax = _up64(n) + KT
    heads_of = lambda t: t[:, :n].view(B, n, kv_heads, hd).transpose(1, 2).contiguous()      # [B, kv_heads, n, hd]
    (k8, ks), (v8, vs) = ops.quantize_fp8_kv(heads_of(k)), ops.quantize_fp8_kv(heads_of(v))
    kd, vd = ops.dequantize_fp8_kv(k8, ks), ops.dequantize_fp8_kv(v8, vs)
    assert not torch.equal(kd, heads_of(k))                                                    # (the rounding is there)
    key_valid = None
    if masked:      # a hole over a tile seam and the chunk's own first keys
        ar = torch.arange(tmax, device=dev)
        key_valid = torch.stack([(ar < 50) | (ar >= 70), ar >= q0 + 3]).to(torch.uint8).contiguous()
    dead = torch.zeros(B, tmax, dtype=torch.bool, device=dev)
    dead[:, n:] = True
    if masked:
        dead |= key_valid == 0

    def codes(c8, sc):
        cc = torch.full((B, kv_heads, tmax, hd), NAN8, dtype=torch.uint8, device=dev)
        ss = torch.full((B, kv_heads, tmax), float("nan"), device=dev)
        cc[:, :, :n], ss[:, :, :n] = c8.view(torch.uint8), sc
        cc[dead[:, None, :].expand(B, kv_heads, tmax)] = NAN8
        ss[dead[:, None, :].expand(B, kv_heads, tmax)] = float("nan")
        return cc, ss

    def values(d):
        c = torch.full((B, kv_heads, tmax, hd), float("nan"), dtype=torch.bfloat16, device=dev)
        c[:, :, :n] = d
        c[dead[:, None, :].expand(B, kv_heads, tmax)] = float("nan")
        return c
    (kc8, kss), (vc8, vss) = codes(k8, ks), codes(v8, vs)
    qs = q[:, q0:n]
    a = ops.attention_cached(qs, kc8, vc8, q0, HEADS, hd ** -0.5, key_valid=key_valid, scales=(kss, vss))
    b = ops.attention_cached(qs, values(kd), values(vd), q0, HEADS, hd ** -0.5, key_valid=key_valid)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    c = ops.attention_cached(qs, kc8.view(torch.float8_e4m3fn), vc8.view(torch.float8_e4m3fn), q0, HEADS, hd ** -0.5, key_valid=key_valid,
                             scales=(kss, vss))
    assert torch.equal(a, c)


def _pad_masks(dev, n):
    """[3, n] bool: left pads over more than a key tile, right pads, a hole that swallows a whole key tile"""
    ar = torch.arange(n, device=dev)
    return torch.stack([ar >= KT + 6, ar < n - 50, (ar < KT + 26) | (ar >= 3 * KT + 8)])


@pytest.mark.parametrize("q0,sq", [(0, 300), (40, 260), (230, 70)])
@pytest.mark.parametrize("hd,kv_heads", [(128, 4), (128, 2), (64, 1)])
def test_key_valid_with_nan_in_the_masked_rows(dev, hd, kv_heads, q0, sq):
    n = q0 + sq
    valid = _pad_masks(dev, n)
    out, ref = _call(dev, hd, kv_heads, q0, sq, B=3, valid=valid)
    assert torch.isfinite(out).all()
    assert torch.equal(out, ref)
    # queries that see no valid key: row 0's queries up to position KT + 5 (its left pads) -- all-zero rows; every other query has one
    qpos = torch.arange(q0, n, device=dev)
    sees = (valid[:, None, :] & (torch.arange(n, device=dev)[None, None, :] <= qpos[None, :, None])).any(-1)      # [3, sq]
    assert sees[1:].all() and (~sees[0]).sum().item() == max(0, KT + 6 - q0)
    assert (out[~sees] == 0).all()
    assert (out[sees].abs().amax(-1) > 0).all()


def _ref64(q, k, v, kv_heads, scale, q0, valid=None):
    """fp64 softmax attention of queries at positions q0 .. over keys 0 .. q0 + s_q - 1 (token-major bf16 inputs); valid [B, keys] bool"""
    B, Sq, D = q.shape
    Skv, hd = k.shape[1], D // HEADS
    Q = q.double().view(B, Sq, HEADS, hd).transpose(1, 2)
    K = k.double().view(B, Skv, kv_heads, hd).transpose(1, 2).repeat_interleave(HEADS // kv_heads, 1)
    V = v.double().view(B, Skv, kv_heads, hd).transpose(1, 2).repeat_interleave(HEADS // kv_heads, 1)
    s = Q @ K.transpose(-1, -2) * scale
    see = (torch.arange(Skv, device=q.device)[None, :] <= torch.arange(Sq, device=q.device)[:, None] + q0)[None, None]
    if valid is not None:
        see = see & valid[:, None, None, :]
    return (torch.softmax(s.masked_fill(~see, float("-inf")), -1) @ V).transpose(1, 2).reshape(B, Sq, D)


def _err_rows(out, ref):
    """worst row: max |out - ref| over a (batch, query) row's channels, relative to that row's max |ref|"""
    return ((out.double() - ref).abs().amax(-1) / ref.abs().amax(-1)).max().item()


@functools.lru_cache(maxsize=None)
def _long_draw(dev, hd, kv_heads):
    """B = 1, 16384 tokens, the fixed seed"""
    g = torch.Generator(device=dev).manual_seed(0)
    return tuple(torch.randn(1, 16384, n * hd, generator=g, device=dev).bfloat16() for n in (HEADS, kv_heads, kv_heads))


@functools.lru_cache(maxsize=None)
def _baseline_rows(dev, hd, kv_heads):
    """the single-pass kernel's worst row on the leading 288 tokens of the long draw, measured once"""
    from videotgb_amd import ops
    q, k, v = (t[:, :288] for t in _long_draw(dev, hd, kv_heads))
    rep = lambda t: t.reshape(1, 288, kv_heads, 1, hd).expand(1, 288, kv_heads, HEADS // kv_heads, hd).reshape(1, 288, HEADS * hd)
    out = ops.attention(q, rep(k), rep(v), HEADS, hd ** -0.5, causal=True)
    return _err_rows(out, _ref64(q, k, v, kv_heads, hd ** -0.5, 0))


@pytest.mark.parametrize("q0,sq,tmax", [(4100, 40, 4160), (16320, 64, 16384)])
@pytest.mark.parametrize("hd,kv_heads", [(128, 2), (64, 4), (128, 1)])
def test_past_4096_keys_vs_fp64(dev, hd, kv_heads, q0, sq, tmax):
    from videotgb_amd import ops
    q, k, v = _long_draw(dev, hd, kv_heads)
    n = q0 + sq
    qs = q[:, q0:n]
    with pytest.raises(NotImplementedError, match="4096"):      # the tiled kernel refuses these keys
        ops.attention_tiled(qs, k[:, :n], v[:, :n], HEADS, hd ** -0.5, kv_heads=kv_heads)
    out = ops.attention_cached(qs, _cache(k, kv_heads, tmax, n), _cache(v, kv_heads, tmax, n), q0, HEADS, hd ** -0.5)
    assert torch.isfinite(out).all()
    err, base = _err_rows(out, _ref64(qs, k[:, :n], v[:, :n], kv_heads, hd ** -0.5, q0)), _baseline_rows(dev, hd, kv_heads)
    print(f"cached hd={hd} kv_heads={kv_heads} q0={q0} s_q={sq} tmax={tmax}: worst row {err:.3e}, single-pass (288 keys) {base:.3e}, "
          f"ratio {err / base:.3f}")
    assert 0 < base < 1e-2      # (the yardstick itself is a bf16-rounding-sized error)
    assert err <= 1.5 * base, (err, base)


@pytest.mark.parametrize("hd,kv_heads", [(128, 2), (64, 4), (128, 1)])
def test_masked_leading_tiles_leave_the_initial_state_bit_for_bit(dev, hd, kv_heads):
    from videotgb_amd import ops
    q, k, v = _long_draw(dev, hd, kv_heads)
    q0, sq, tmax, cut = 16320, 64, 16384, 12288
    qs = q[:, q0:]
    key_valid = (torch.arange(tmax, device=dev) >= cut).to(torch.uint8)[None].contiguous()
    nan_head = lambda t: torch.cat([torch.full_like(t[:, :cut], float("nan")), t[:, cut:]], 1)
    out = ops.attention_cached(qs, _cache(nan_head(k), kv_heads, tmax, tmax), _cache(nan_head(v), kv_heads, tmax, tmax), q0, HEADS, hd ** -0.5,
                               key_valid=key_valid)
    ref = ops.attention_tiled(qs, k[:, cut:], v[:, cut:], HEADS, hd ** -0.5, kv_heads=kv_heads, causal=True)      # 4096 keys, s_q 64
    assert torch.isfinite(out).all() and torch.equal(out, ref)


@pytest.mark.parametrize("q0,sq", [(70, 45), (0, 300)])
@pytest.mark.parametrize("hd", [128, 64])
def test_a_row_depends_on_that_row_alone(dev, hd, q0, sq):
    from videotgb_amd import ops
    n = q0 + sq
    a3, _ = _call(dev, hd, 2, q0, sq, B=3)
    a1, _ = _call(dev, hd, 2, q0, sq, B=1)
    assert torch.equal(a3[:1], a1)                                                        # batch 1 and 3
    again, _ = _call(dev, hd, 2, q0, sq, B=3)
    assert torch.equal(a3, again)                                                         # run to run
    big, _ = _call(dev, hd, 2, q0, sq, B=3, tmax=_up64(n) + 5 * KT)
    assert torch.equal(a3, big)                                                           # the cache's length
    odd, _ = _call(dev, hd, 2, q0, sq, B=3, tmax=n)                                       # (tmax need not be a multiple of 64)
    assert torch.equal(a3, odd)
    q, k, v = _draw(dev, hd, 2)                                                           # kv_heads 2 against the heads replicated to 4
    rep = lambda t: t[:, :n].reshape(3, n, 2, 1, hd).expand(3, n, 2, 2, hd).reshape(3, n, 4 * hd)
    tmax = _up64(n)
    r = ops.attention_cached(q[:, q0:n], _cache(rep(k), 4, tmax, n), _cache(rep(v), 4, tmax, n), q0, HEADS, hd ** -0.5)
    assert torch.equal(a3, r)


def test_wrapper_asserts_and_library_rejections(dev):
    from videotgb_amd import ops
    q, k, v = (t[:1] for t in _draw(dev, 128, 2))
    kc, vc = _cache(k, 2, 320, 300), _cache(v, 2, 320, 300)
    with pytest.raises(NotImplementedError, match="exceed the cache"):
        ops.attention_cached(q[:, :100], kc, vc, 221, HEADS, 0.1)
    with pytest.raises(ValueError, match="q0"):
        ops.attention_cached(q[:, :100], kc, vc, -1, HEADS, 0.1)
    with pytest.raises(AssertionError):
        ops.attention_cached(q[:, :100].float(), kc, vc, 0, HEADS, 0.1)
    with pytest.raises(AssertionError):
        ops.attention_cached(q[:, :100], kc.transpose(1, 2), vc.transpose(1, 2), 0, HEADS, 0.1)
    with pytest.raises(AssertionError):      # codes without scales
        ops.attention_cached(q[:, :100], kc.view(torch.uint8)[..., :128].contiguous(), vc.view(torch.uint8)[..., :128].contiguous(), 0, HEADS, 0.1)
