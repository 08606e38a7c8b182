"""-m gpu: vtgb_gemm_skinny_bias (ops.gemm_skinny(..., bias=)) against the unbiased entries, bit for bit, on both weight streams.

The contract (include/vtgb.h): the fp32 bias is added to the accumulators of K split 0 alone, after the fp8 row scale, before the fragment is
written or -- without a split -- before the single rounding.  So with a split the biased call's fragments are the unbiased call's except
fragment 0 = fragment 0 + bias, and its ``out`` is round((frag0 + bias) + frag1 + ...) in split order; without one it is
round(acc + bias), acc = the unbiased call's fp32 output.  Nothing here needs a tolerance: every expected value is formed from the unbiased
kernel's own fp32 numbers with the one fp32 addition the contract names.  The bias holds zeros and +-large entries and sits in front of
NaN-filled memory, so a read of entry n >= N shows in the fragments' pad columns."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

MS = (1, 16, 17, 33, 65, 124)      # every x-row-block count of the fp8 stream (XB = 1, 1, 2, 4, 8, 8)
NS = (8, 128, 200, 384)            # less than a tile's 4-wide store, one tile, a ragged last tile, three tiles
SPLIT = ((512, 2), (512, 3), (512, 8))      # (K, n_splits): S > 1
UNSPLIT = ((128, 0), (512, 1))              # (K, n_splits): S == 1 -- the library's own choice at two k-tiles, and forced
STREAMS = ("rowmajor", "tiled", "fp8")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _weight(stream, N, K):
    from videotgb_amd import ops
    g = torch.Generator().manual_seed(1000 * N + K)
    w = (torch.randn(N, K, generator=g) * 0.05).bfloat16().cuda()
    return {"rowmajor": lambda: w, "tiled": lambda: ops.SkinnyWeight(w), "fp8": lambda: ops.SkinnyWeightFp8(w)}[stream]()


@functools.lru_cache(maxsize=None)
def _x(M, K):
    g = torch.Generator().manual_seed(7 * M + K)
    return torch.randn(M, K, generator=g).bfloat16().cuda()


@functools.lru_cache(maxsize=None)
def _bias(N):
    """fp32 [N] with zeros and +-large entries, the last N elements in front of NaN-filled memory (and behind some)."""
    g = torch.Generator().manual_seed(N)
    b = torch.randn(N, generator=g)
    b[::5] = 0.0
    b[1::7] = 3.0e4
    b[2::7] = -3.0e4
    buf = torch.full((64 + N + 1024,), float("nan"), device="cuda")
    buf[64: 64 + N] = b.cuda()
    return buf[64: 64 + N]


def _frags(ws, N, S, M):
    nt = (N + 127) // 128
    return ws.view(torch.float32)[: nt * S * M * 128].view(nt, S, M, 128).clone()


def _bias_tiles(N):
    nt = (N + 127) // 128
    b = torch.zeros(nt * 128, device="cuda")
    b[:N] = _bias(N)
    return b.view(nt, 1, 128)


def _check_split(stream, M, N, K, S):
    from videotgb_amd import ops
    x, w, bias = _x(M, K), _weight(stream, N, K), _bias(N)
    ws0, ws1 = (torch.zeros(ops.gemm_skinny_workspace_bytes(M, N, K, S), dtype=torch.uint8, device="cuda") for _ in range(2))
    _, S0, _ = ops.gemm_skinny(x, w, n_splits=S, workspace=ws0, defer_reduce=True)
    _, S1, _ = ops.gemm_skinny(x, w, n_splits=S, workspace=ws1, defer_reduce=True, bias=bias)
    assert S0 == S1 == S > 1
    f0, f1 = _frags(ws0, N, S, M), _frags(ws1, N, S, M)
    assert bool(torch.isfinite(f1).all()), "a bias entry n >= N was read"
    assert torch.equal(f1[:, 1:], f0[:, 1:])                                   # the other splits: untouched
    assert torch.equal(f1[:, 0], f0[:, 0] + _bias_tiles(N))                    # split 0: + bias, one fp32 addition
    acc = f0[:, 0] + _bias_tiles(N)
    for sp in range(1, S):
        acc = acc + f0[:, sp]                                                  # split order
    want = acc.permute(1, 0, 2).reshape(M, -1)[:, :N]
    for dt in (torch.bfloat16, torch.float32):
        out = ops.gemm_skinny(x, w, n_splits=S, out_dtype=dt, bias=bias)
        assert torch.equal(out, want.to(dt)), (stream, M, N, K, S, dt)


def _check_unsplit(stream, M, N, K, S):
    from videotgb_amd import ops
    x, w, bias = _x(M, K), _weight(stream, N, K), _bias(N)
    assert ops.gemm_skinny_workspace_bytes(M, N, K, S) == 0                    # no K split
    acc = ops.gemm_skinny(x, w, n_splits=S, out_dtype=torch.float32)
    for dt in (torch.bfloat16, torch.float32):
        out = ops.gemm_skinny(x, w, n_splits=S, out_dtype=dt, bias=bias)
        assert bool(torch.isfinite(out.float()).all())
        assert torch.equal(out, (acc + bias).to(dt)), (stream, M, N, K, S, dt)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("stream", STREAMS)
def test_split_calls_add_the_bias_to_split_0(dev, stream, M):
    for N in NS:
        for K, S in SPLIT:
            _check_split(stream, M, N, K, S)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("stream", STREAMS)
def test_unsplit_calls_round_acc_plus_bias_once(dev, stream, M):
    for N in NS:
        for K, S in UNSPLIT:
            _check_unsplit(stream, M, N, K, S)


def test_the_padded_out_keeps_its_pad_columns(dev):
    """An ``out`` with a row pitch above N: the scalar tail store of the unsplit epilogue and the reduce launch leave the pad alone."""
    from videotgb_amd import ops
    for S in (1, 3):
        x, w, bias = _x(17, 512), _weight("tiled", 200, 512), _bias(200)
        buf = torch.full((17, 208), 7.0, dtype=torch.bfloat16, device="cuda")
        ops.gemm_skinny(x, w, out=buf[:, :200], n_splits=S, bias=bias)
        assert bool((buf[:, 200:] == 7.0).all())
        assert torch.equal(buf[:, :200], ops.gemm_skinny(x, w, n_splits=S, bias=bias))


@pytest.mark.parametrize("stream", ["tiled", "fp8"])
def test_deferred_consumers_read_the_biased_fragments(dev, stream):
    """H = 2048: vtgb_llm_rmsnorm_parts / vtgb_llm_rope_cache_parts_pos over the biased call's fragments == vtgb_llm_rmsnorm /
    vtgb_llm_rope_cache_pos over its reduced ``out``, bit for bit -- the consumers add the fragments as before and see acc + bias."""
    from videotgb_amd import _lib as L, ops
    from videotgb_amd.ops import _ptr, _stream
    lib, code, eps = L.lib(), L.BF16, 1e-5
    M, H = 5, 2048
    g = torch.Generator().manual_seed(9)
    x, w, bias = _x(M, H), _weight(stream, H, H), _bias(H)
    ws = torch.zeros(ops.gemm_skinny_workspace_bytes(M, H, H), dtype=torch.uint8, device="cuda")
    _, S, _ = ops.gemm_skinny(x, w, workspace=ws, defer_reduce=True, bias=bias)
    assert S > 1
    out = ops.gemm_skinny(x, w, bias=bias)
    assert not torch.equal(out, ops.gemm_skinny(x, w))
    # residual + RMSNorm
    res = torch.randn(M, H, generator=g).bfloat16().cuda()
    nw = (1.0 + 0.1 * torch.randn(H, generator=g)).bfloat16().cuda()
    xa, xb, ha, hb = res.clone(), res.clone(), torch.empty_like(res), torch.empty_like(res)
    L.check(lib.vtgb_llm_rmsnorm_parts(code, _ptr(xa), _ptr(ws), S, _ptr(nw), _ptr(ha), M, H, eps, _stream()))
    L.check(lib.vtgb_llm_rmsnorm(code, _ptr(xb), _ptr(out), _ptr(nw), _ptr(hb), M, H, eps, _stream()))
    assert torch.equal(xa, xb) and torch.equal(ha, hb)
    # rotary + cache append, per-row rotary offsets: q | k | v = 8 + 4 + 4 heads of 128
    nq, nkv, hd, tmax = 8, 4, 128, 64
    fr = torch.arange(tmax, dtype=torch.float32)[:, None] * (1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd)))[None]
    emb = torch.cat((fr, fr), dim=-1)
    cos, sin = emb.cos().bfloat16().cuda(), emb.sin().bfloat16().cuda()
    pos = torch.tensor([7], dtype=torch.long, device="cuda")
    off = torch.tensor([0, 3, -2, 11, 5], dtype=torch.long, device="cuda")
    got = []
    for parts in (True, False):
        q = torch.zeros(M, nq * hd, dtype=torch.bfloat16, device="cuda")
        kc, vc = (torch.zeros(M, nkv, tmax, hd, dtype=torch.bfloat16, device="cuda") for _ in range(2))
        if parts:
            L.check(lib.vtgb_llm_rope_cache_parts_pos(code, _ptr(ws), S, _ptr(q), _ptr(kc), _ptr(vc), _ptr(cos), _ptr(sin), _ptr(pos), _ptr(off), M, nq, nkv,
                                                      hd, tmax, _stream()))
        else:
            L.check(lib.vtgb_llm_rope_cache_pos(code, _ptr(out), _ptr(q), _ptr(kc), _ptr(vc), _ptr(cos), _ptr(sin), _ptr(pos), _ptr(off), M, nq, nkv, hd,
                                                tmax, _stream()))
        got.append((q, kc, vc))
    for a, b in zip(*got):
        assert torch.equal(a, b)
    assert bool(got[0][1][:, :, 7].abs().sum() > 0)
