"""-m gpu: the language-model step kernels of csrc/llm.hip, entry by entry and dispatch branch by dispatch branch, against the fp64
references and acceptance rules of tests/llm_refs.py (tests/test_llm_refs.py shows on the CPU that those rules pass fp32 arithmetic and
reject mutants).  Calls go through ctypes on the current stream; every output and every in-place operand sits between 64 sentinel
elements that must be unchanged afterwards; inputs sit between NaNs, so a read past an end reaches the result."""
import ctypes as C
import gc

import pytest
import torch

import llm_refs as R
from llm_refs import BF16, F32

pytestmark = pytest.mark.gpu
PAD, SENT, NAN = 64, -1984.0, float("nan")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    # The graph decoders of earlier test modules are cyclic garbage that still holds captured hipGraphs.  torch.cuda.graph destroys such
    # graphs on an idle device (synchronize, gc.collect) when the next capture begins; the objects these 212 cases churn through would
    # instead let the collector run wherever it next falls due -- in the middle of a later module's decode step, with kernels in flight on a
    # side stream, where the destruction aborted the process.  So collect here and on leaving, with the device idle.
    torch.cuda.synchronize()
    gc.collect()
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    gc.collect()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _code(dtype):
    from videotgb_amd import _lib as L
    return L.BF16 if dtype == BF16 else L.F32


def _name(dtype):
    return "bf16" if dtype == BF16 else "f32"


class Guard:
    """a copy of `t` between PAD elements of `fill` on both sides, `off` elements further into the buffer (off = 1: not 16-byte aligned)"""

    def __init__(self, t, fill=SENT, off=0):
        n = t.numel()
        self.fill, self.lo, self.hi = fill, PAD + off, PAD + off + n
        self.buf = torch.full((self.hi + PAD,), fill, dtype=t.dtype, device=t.device)
        self.t = self.buf[self.lo:self.hi].view(t.shape)
        self.t.copy_(t)
        assert (self.t.data_ptr() % 16 == 0) == (off == 0)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return bool((self.buf[:self.lo] == self.fill).all()) and bool((self.buf[self.hi:] == self.fill).all())


def _out(shape, dtype, dev, off=0):
    """an output: NaN inside (an element the kernel leaves out fails its rule), sentinels around"""
    return Guard(torch.full(shape, NAN, dtype=dtype, device=dev), off=off)


def _tables(tmax, hd, dev, dtype):
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, device=dev, dtype=torch.float32) / hd))
    fr = torch.arange(tmax, device=dev, dtype=torch.float32)[:, None] * inv[None]
    emb = torch.cat((fr, fr), dim=-1)
    return emb.cos().to(dtype), emb.sin().to(dtype)


def _randn(shape, seed, dev, dtype=F32):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype).to(dev)


# ----------------------------------------------------------------------------------------------------------------------------- RMSNorm
# (dtype, rows, H, misaligned operand): bf16 vector NV = 2 / 1 at H = 4096 / 2048, fp32 vector NV = 4 / 2 at H = 4096 / 2048; every other H
# and every misaligned operand takes the scalar kernel of its dtype
RMS_CASES = ([(dt, r, H, None) for dt in (BF16, F32) for r, H in R.RMS_SHAPES[dt]] + [(BF16, 3, 4096, "x"), (F32, 3, 2048, "w")])


@pytest.mark.parametrize("eps", R.RMS_EPS)
@pytest.mark.parametrize("with_delta", [True, False], ids=["delta", "nodelta"])
@pytest.mark.parametrize("dtype,rows,H,mis", RMS_CASES, ids=[f"{_name(c[0])}-{c[1]}x{c[2]}" + (f"-mis_{c[3]}" if c[3] else "") for c in RMS_CASES])
def test_rmsnorm_vs_fp64(dev, dtype, rows, H, mis, with_delta, eps):
    from videotgb_amd import _lib as L
    x, delta, w = R.rmsnorm_inputs(rows, H, dtype, seed=rows * 10007 + H, device=dev)
    xg, wg, hg = Guard(x, off=int(mis == "x")), Guard(w, fill=NAN, off=int(mis == "w")), _out((rows, H), dtype, dev)
    dg = Guard(delta, fill=NAN) if with_delta else None
    L.check(L.lib().vtgb_llm_rmsnorm(_code(dtype), xg.ptr, dg.ptr if dg else None, wg.ptr, hg.ptr, rows, H, eps, _stream()))
    torch.cuda.synchronize()
    assert xg.intact() and hg.intact()
    share = R.check_rmsnorm(hg.t, xg.t, x, delta if with_delta else None, w, eps, dtype)
    print(f"off-centre share {share:.3e}")
    if rows > 1:                                                                       # the all-zero row: exactly 0 (and finite: the rule)
        assert not hg.t[-1].any()


@pytest.mark.parametrize("H", [4096, 2048])
@pytest.mark.parametrize("M", [1, 5, 128])
@pytest.mark.parametrize("S", [2, 3, 7])
def test_rmsnorm_parts_on_built_fragments(dev, S, M, H):
    """The fragments come from llm_refs.make_fragments (the layout as gemm_skinny.hip states it), not from a GEMM."""
    from videotgb_amd import _lib as L
    x, _, w = R.rmsnorm_inputs(M, H, BF16, seed=S * 1000 + M, device=dev)
    part, delta = R.make_fragments(H, S, M, seed=S * 77 + M + H, device=dev)
    xg, hg = Guard(x), _out((M, H), BF16, dev)
    pg = Guard(part, fill=NAN)
    L.check(L.lib().vtgb_llm_rmsnorm_parts(L.BF16, xg.ptr, pg.ptr, S, w.data_ptr(), hg.ptr, M, H, 1e-6, _stream()))
    torch.cuda.synchronize()
    assert xg.intact() and hg.intact()
    assert R.same_bits(xg.t, x + delta)
    R.check_rmsnorm(hg.t, xg.t, x, delta, w, 1e-6, BF16)


# ------------------------------------------------------------------------------------------------------------------------------ rotary
@pytest.mark.parametrize("per_row", [False, True], ids=["parts", "parts_pos"])
@pytest.mark.parametrize("nq,nkv,hd", [(8, 2, 128), (8, 2, 64), (8, 2, 96)])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S", [2, 5])
def test_rope_cache_parts_on_built_fragments(dev, S, B, nq, nkv, hd, per_row):
    """q, the cache rows at pos and the untouched rest of the cache are bit for bit HF's _rot_half arithmetic in bf16 on the rounded sums
    of the fragments (hd 64 and 96: heads straddle the 128-column fragment tiles)."""
    from videotgb_amd import _lib as L
    from videotgb_amd.decode import _rot_half
    tmax, pos, nh = 64, 40, nq + 2 * nkv
    part, sums = R.make_fragments(nh * hd, S, B, seed=S * 100 + B * 10 + hd, device=dev)
    qkv = sums.view(B, nh, hd)
    cos, sin = _tables(tmax, hd, dev, BF16)
    pos_t = torch.tensor([pos], device=dev)
    off = torch.tensor([-7, -40, 0][:B], device=dev)
    kc0, vc0 = _randn((B, nkv, tmax, hd), 1, dev, BF16), _randn((B, nkv, tmax, hd), 2, dev, BF16)
    qg, kg, vg, pg = _out((B, nq * hd), BF16, dev), Guard(kc0), Guard(vc0), Guard(part, fill=NAN)
    if per_row:
        L.check(L.lib().vtgb_llm_rope_cache_parts_pos(L.BF16, pg.ptr, S, qg.ptr, kg.ptr, vg.ptr, cos.data_ptr(), sin.data_ptr(), pos_t.data_ptr(),
                                                      off.data_ptr(), B, nq, nkv, hd, tmax, _stream()))
    else:
        L.check(L.lib().vtgb_llm_rope_cache_parts(L.BF16, pg.ptr, S, qg.ptr, kg.ptr, vg.ptr, cos.data_ptr(), sin.data_ptr(), pos_t.data_ptr(), B, nq, nkv,
                                                  hd, tmax, _stream()))
    torch.cuda.synchronize()
    assert qg.intact() and kg.intact() and vg.intact()
    rp = pos + off if per_row else torch.full((B,), pos, device=dev)
    c, s = cos[rp][:, None], sin[rp][:, None]
    qk = qkv[:, : nq + nkv]
    ref = qk * c + _rot_half(qk) * s                                                  # apply_rotary_pos_emb in the model's dtype
    kc_ref, vc_ref = kc0.clone(), vc0.clone()
    kc_ref[:, :, pos], vc_ref[:, :, pos] = ref[:, nq:], qkv[:, nq + nkv:]
    assert R.same_bits(qg.t.view(B, nq, hd), ref[:, :nq].contiguous())
    assert R.same_bits(kg.t, kc_ref) and R.same_bits(vg.t, vc_ref)


@pytest.mark.parametrize("hd", [16, 64])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=_name)
def test_rope_cache_without_tables_passes_q_through_and_appends(dev, dtype, hd):
    """cos = sin = NULL (T5's decoder)"""
    from videotgb_amd import _lib as L
    B, nq, nkv, tmax, pos = 3, 4, 2, 64, 40
    qkv = _randn((B, nq + 2 * nkv, hd), hd, dev, dtype)
    kc0, vc0 = _randn((B, nkv, tmax, hd), 3, dev, dtype), _randn((B, nkv, tmax, hd), 4, dev, dtype)
    pos_t = torch.tensor([pos], device=dev)
    qg, kg, vg, ig = _out((B, nq, hd), dtype, dev), Guard(kc0), Guard(vc0), Guard(qkv, fill=NAN)
    L.check(L.lib().vtgb_llm_rope_cache(_code(dtype), ig.ptr, qg.ptr, kg.ptr, vg.ptr, None, None, pos_t.data_ptr(), B, nq, nkv, hd, tmax, _stream()))
    torch.cuda.synchronize()
    assert qg.intact() and kg.intact() and vg.intact()
    kc_ref, vc_ref = kc0.clone(), vc0.clone()
    kc_ref[:, :, pos], vc_ref[:, :, pos] = qkv[:, nq:nq + nkv], qkv[:, nq + nkv:]
    assert R.same_bits(qg.t, qkv[:, :nq].contiguous()) and R.same_bits(kg.t, kc_ref) and R.same_bits(vg.t, vc_ref)


# -------------------------------------------------------------------------------------------------------------------------- activations
def _silu(dev, dtype, gu, rows, I, off=0):
    from videotgb_amd import _lib as L
    ig, og = Guard(gu, fill=NAN, off=off), _out((rows, I), dtype, dev, off=off)
    L.check(L.lib().vtgb_llm_silu_mul(_code(dtype), ig.ptr, og.ptr, rows, I, _stream()))
    torch.cuda.synchronize()
    assert og.intact()
    return og.t


def _gated_act(dev, dtype, gu, rows, I, kind, gated):
    from videotgb_amd import _lib as L
    ig, og = Guard(gu, fill=NAN), _out((rows, I), dtype, dev)
    L.check(L.lib().vtgb_llm_gated_act(_code(dtype), ig.ptr, og.ptr, rows, I, kind, gated, _stream()))
    torch.cuda.synchronize()
    assert og.intact()
    return og.t


# vtgb_llm_silu_mul's dispatch: the vector kernel when I % V == 0 (V = 8 bf16, 4 fp32), rows <= 65535 and both pointers are 16-byte aligned;
# else the scalar kernel -- I % V != 0: (3, 100) bf16 only, (5, 7), (2, 11), (300, 3501: also its grid-stride loop past 4096 blocks);
# rows > 65535: (65536, 8); misaligned gu: (3, 2056)
SILU_CASES = [(dt, r, I, 0) for dt in (BF16, F32) for r, I in R.SILU_SHAPES] + [(BF16, 3, 2056, 1), (F32, 3, 2056, 1)]


@pytest.mark.parametrize("dtype,rows,I,off", SILU_CASES, ids=[f"{_name(c[0])}-{c[1]}x{c[2]}" + ("-mis" if c[3] else "") for c in SILU_CASES])
def test_silu_mul_vs_fp64(dev, dtype, rows, I, off):
    g, u = R.act_inputs(rows, I, dtype, seed=rows * 31 + I, device=dev)
    gu = torch.cat([g, u], -1)
    got = _silu(dev, dtype, gu, rows, I, off)
    share = R.check_act(got, 0, g, u, dtype)
    print(f"off-centre share {share:.3e}")
    # the vector path, the scalar path (the same values at a misaligned address) and vtgb_llm_gated_act(kind 0, gated) state the same arithmetic
    assert R.same_bits(got, _silu(dev, dtype, gu, rows, I, 1 - off))
    assert R.same_bits(got, _gated_act(dev, dtype, gu, rows, I, 0, 1))


@pytest.mark.parametrize("rows,I", R.ACT_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("gated", [0, 1], ids=["ungated", "gated"])
@pytest.mark.parametrize("kind", [0, 1, 2, 3], ids=[R.KINDS[k] for k in range(4)])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=_name)
def test_gated_act_vs_fp64(dev, dtype, kind, gated, rows, I):
    """Ungated: gu has leading dimension I, and the NaNs after it prove that nothing past rows x I is read into the result."""
    g, u = R.act_inputs(rows, I, dtype, seed=rows * 31 + I, device=dev)
    gu = torch.cat([g, u], -1) if gated else g
    got = _gated_act(dev, dtype, gu, rows, I, kind, gated)
    share = R.check_act(got, kind, g, u if gated else None, dtype)
    print(f"off-centre share {share:.3e}")


# ---------------------------------------------------------------------------------------------------------------------- attention_rows
def _rounder(dtype):
    """HF's bf16 roundings (scores, + bias, weights), as test_attention_rows_masked_vs_fp64 takes them"""
    return (lambda t: t.to(dtype).double()) if dtype == BF16 else (lambda t: t)


def _attn_tol(dtype):
    return 1e-5 if dtype == F32 else 2e-2


@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("dk", [16, 64])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=_name)
def test_attention_rows_decode_form_vs_fp64(dev, dtype, dk, scale):
    """The T5 decoder's self-attention: keys [0, *pos] of a static cache, bias row *pos.  rows x heads = 9: the last workgroup has idle
    waves.  Cache slots past *pos and every other bias row hold NaN."""
    from videotgb_amd import _lib as L
    B, H, T = 3, 3, 256
    q = _randn((B, H * dk), 11 + dk, dev, dtype)
    kc, vc = _randn((B, H, T, dk), 12, dev, dtype), _randn((B, H, T, dk), 13, dev, dtype)
    bias = _randn((H, T, T), 14, dev, dtype)
    rnd = _rounder(dtype)
    for pos in (0, 63, 64, 200):
        n = pos + 1
        k_p, v_p, b_p = kc.clone(), vc.clone(), torch.full_like(bias, NAN)
        k_p[:, :, n:], v_p[:, :, n:] = NAN, NAN
        b_p[:, pos, :n] = bias[:, pos, :n]
        pos_t = torch.tensor([pos], device=dev)
        og = _out((B, H * dk), dtype, dev)
        a = L.LlmAttnRowsArgs(_code(dtype), B, H, dk, 1, 0, T, scale, q.data_ptr(), H * dk, k_p.data_ptr(), v_p.data_ptr(), H * T * dk, T * dk, dk,
                              b_p.data_ptr(), T, T * T, pos_t.data_ptr(), og.ptr, H * dk)
        L.check(L.lib().vtgb_llm_attention_rows(C.byref(a), _stream()))
        torch.cuda.synchronize()
        assert og.intact() and torch.isfinite(og.t).all()
        qd = q.double().view(B, H, dk)
        s = rnd(torch.einsum("bhd,bhtd->bht", qd, kc[:, :, :n].double()) * scale)
        s = rnd(s + bias[:, pos, :n].double()[None])
        ref = torch.einsum("bht,bhtd->bhd", rnd(torch.softmax(s, -1)), vc[:, :, :n].double()).reshape(B, H * dk)
        err = (og.t.double() - ref).abs().max().item()
        print(f"pos {pos}: max err {err:.3e} of max |ref| {ref.abs().max().item():.3e}")
        assert err <= _attn_tol(dtype) * ref.abs().max().item(), (pos, err)


@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("dk", [16, 64])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=_name)
def test_attention_rows_cross_form_vs_fp64(dev, dtype, dk, scale):
    """The T5 decoder's cross-attention: a fixed n_keys, no bias, one row per K/V batch.  Keys past n_keys hold NaN."""
    from videotgb_amd import _lib as L
    B, H, T = 3, 3, 80
    q = _randn((B, H * dk), 21 + dk, dev, dtype)
    kc, vc = _randn((B, H, T, dk), 22, dev, dtype), _randn((B, H, T, dk), 23, dev, dtype)
    rnd = _rounder(dtype)
    for n in (1, 37, 65):
        k_p, v_p = kc.clone(), vc.clone()
        k_p[:, :, n:], v_p[:, :, n:] = NAN, NAN
        og = _out((B, H * dk), dtype, dev)
        a = L.LlmAttnRowsArgs(_code(dtype), B, H, dk, 1, n, T, scale, q.data_ptr(), H * dk, k_p.data_ptr(), v_p.data_ptr(), H * T * dk, T * dk, dk,
                              None, 0, 0, None, og.ptr, H * dk)
        L.check(L.lib().vtgb_llm_attention_rows(C.byref(a), _stream()))
        torch.cuda.synchronize()
        assert og.intact() and torch.isfinite(og.t).all()
        s = rnd(torch.einsum("bhd,bhtd->bht", q.double().view(B, H, dk), kc[:, :, :n].double()) * scale)
        ref = torch.einsum("bht,bhtd->bhd", rnd(torch.softmax(s, -1)), vc[:, :, :n].double()).reshape(B, H * dk)
        err = (og.t.double() - ref).abs().max().item()
        print(f"n_keys {n}: max err {err:.3e} of max |ref| {ref.abs().max().item():.3e}")
        assert err <= _attn_tol(dtype) * ref.abs().max().item(), (n, err)


@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("dk", [16, 64])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=_name)
def test_attention_rows_encoder_form_equals_the_masked_entry_with_every_key_valid(dev, dtype, dk, scale):
    """rows = B x P straight out of q|k|v (token-major strides), bias row = query position; 222 (row, head) pairs: idle waves at the end."""
    from videotgb_amd import _lib as L
    B, P, H = 2, 37, 3
    HD = H * dk
    qkv = _randn((B * P, 3 * HD), 31 + dk, dev, dtype)
    bias = _randn((H, P, P), 32, dev, dtype)
    valid = torch.ones(B, P, dtype=torch.uint8, device=dev)
    outs = []
    for masked in (False, True):
        og = _out((B * P, HD), dtype, dev)
        a = L.LlmAttnRowsArgs(_code(dtype), B * P, H, dk, P, P, P, scale, qkv.data_ptr(), 3 * HD, qkv[:, HD:].data_ptr(), qkv[:, 2 * HD:].data_ptr(),
                              P * 3 * HD, dk, 3 * HD, bias.data_ptr(), P, P * P, None, og.ptr, HD)
        if masked:
            L.check(L.lib().vtgb_llm_attention_rows_masked(C.byref(a), valid.data_ptr(), P, _stream()))
        else:
            L.check(L.lib().vtgb_llm_attention_rows(C.byref(a), _stream()))
        torch.cuda.synchronize()
        assert og.intact() and torch.isfinite(og.t).all()
        outs.append(og.t)
    assert R.same_bits(outs[0], outs[1])
    # (and the values themselves, against fp64 with the same roundings)
    rnd = _rounder(dtype)
    x = qkv.double().view(B, P, 3, H, dk)
    q, k, v = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)
    s = rnd(rnd(q @ k.transpose(-1, -2) * scale) + bias.double()[None])
    ref = (rnd(torch.softmax(s, -1)) @ v).transpose(1, 2).reshape(B * P, HD)
    assert (outs[0].double() - ref).abs().max().item() <= _attn_tol(dtype) * ref.abs().max().item()


# -------------------------------------------------------------------------------------------------------------------- decode_attention
@pytest.mark.parametrize("B,nq,nkv", [(3, 3, 1), (2, 4, 2)])
@pytest.mark.parametrize("hd", [15, 16, 20, 256])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=_name)
def test_decode_attention_vs_fp64(dev, dtype, hd, B, nq, nkv):
    """hd 15: the odd, fully scalar bf16 path; 20: even but no multiple of 8 (scalar K loop, paired V loop); 16: narrower than a wave;
    256: the largest accepted.  B x nq = 9: three idle waves in the last workgroup.  pos 0 .. 127 walks the 16-, 4- and 1-key tails of
    the V loop.  Slots past *pos hold NaN."""
    from videotgb_amd import _lib as L
    tmax, scale = 128, float(hd) ** -0.5
    q = _randn((B, nq * hd), 41 + hd, dev, dtype)
    kc, vc = _randn((B, nkv, tmax, hd), 42, dev, dtype), _randn((B, nkv, tmax, hd), 43, dev, dtype)
    tol = 1e-5 if dtype == F32 else 1e-2
    for pos in (0, 2, 15, 16, 19, 63, 64, 127):
        n = pos + 1
        k_p, v_p = kc.clone(), vc.clone()
        k_p[:, :, n:], v_p[:, :, n:] = NAN, NAN
        pos_t = torch.tensor([pos], device=dev)
        og = _out((B, nq * hd), dtype, dev)
        L.check(L.lib().vtgb_llm_decode_attention(_code(dtype), q.data_ptr(), k_p.data_ptr(), v_p.data_ptr(), og.ptr, pos_t.data_ptr(), B, nq, nkv, hd,
                                                  tmax, scale, _stream()))
        torch.cuda.synchronize()
        assert og.intact() and torch.isfinite(og.t).all()
        K = kc[:, :, :n].double().repeat_interleave(nq // nkv, 1)
        V = vc[:, :, :n].double().repeat_interleave(nq // nkv, 1)
        s = torch.einsum("bhd,bhtd->bht", q.double().view(B, nq, hd), K) * scale
        ref = torch.einsum("bht,bhtd->bhd", torch.softmax(s, -1), V).reshape(B, nq * hd)
        err = (og.t.double() - ref).abs().max().item()
        print(f"pos {pos}: max err {err:.3e} of max |ref| {ref.abs().max().item():.3e}")
        assert err <= tol * ref.abs().max().item(), (pos, err)
