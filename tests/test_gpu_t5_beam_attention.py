"""-m gpu: vtgb_llm_attention_rows_beam (the T5 decoder's self-attention of beam rows through an int32 ancestry table) against
vtgb_llm_attention_rows on the gathered cache ``kc'[r, :, t] = kc[src_row[r, t], :, t]``, bit for bit, in bf16 and in fp32.  Every K/V slot
past *pos, and every slot no table entry points to, holds NaN in what the new entry reads; table entries past *pos point outside the caches.
The gathered reference itself is held to the fp64 statement and tolerance tests/test_gpu_llm_kernels.py has for this kernel's decode form
(``_rounder`` / ``_attn_tol``), so the comparison is not two copies of one mistake."""
import ctypes as C

import pytest
import torch

import llm_refs as R
from llm_refs import BF16, F32
from test_gpu_llm_kernels import _attn_tol, _rounder

pytestmark = pytest.mark.gpu
NAN = float("nan")
B, K = 2, 3
ROWS = B * K


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _randn(shape, seed, dev, dtype):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype).to(dev)


def _tables(T, dev):
    """name -> src_row [ROWS, T] int32: per slot from every row, per slot from the item's own K rows, the identity"""
    g = torch.Generator().manual_seed(7)
    every = torch.randint(0, ROWS, (ROWS, T), generator=g)
    own = torch.randint(0, K, (ROWS, T), generator=g) + (torch.arange(ROWS) // K * K)[:, None]
    ident = torch.arange(ROWS)[:, None].expand(ROWS, T)
    return {k: v.to(torch.int32).contiguous().to(dev) for k, v in (("every", every), ("own", own), ("identity", ident))}


def _args(L, dtype, H, dk, T, scale, q, k, v, bias, pos_t, out):
    code = L.BF16 if dtype == BF16 else L.F32
    return L.LlmAttnRowsArgs(code, ROWS, H, dk, 1, 0, T, scale, q.data_ptr(), H * dk, k.data_ptr(), v.data_ptr(), H * T * dk, T * dk, dk,
                             bias.data_ptr(), T, T * T, pos_t.data_ptr(), out.data_ptr(), H * dk)


@pytest.mark.parametrize("T", [64, 192])
@pytest.mark.parametrize("H,dk", [(4, 16), (4, 64)])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_equals_attention_rows_on_the_gathered_cache(dev, dtype, H, dk, T):
    from videotgb_amd import _lib as L
    scale = 1.0 if dk == 16 else 0.125
    q = _randn((ROWS, H * dk), 11 + dk, dev, dtype)
    kc, vc = _randn((ROWS, H, T, dk), 12, dev, dtype), _randn((ROWS, H, T, dk), 13, dev, dtype)
    bias = _randn((H, T, T), 14, dev, dtype)
    rnd = _rounder(dtype)
    slot = torch.arange(T, device=dev)
    for pos in sorted({0, 1, 63, 64, 65, T - 1} & set(range(T))):
        n = pos + 1
        pos_t = torch.tensor([pos], device=dev)
        for name, table in _tables(T, dev).items():
            idx = table.long()[:, None, :, None]                                        # [ROWS, 1, T, 1]
            kg = torch.take_along_dim(kc, idx.expand(ROWS, H, T, dk), 0)               # kc[src_row[r, t], h, t, :]
            vg = torch.take_along_dim(vc, idx.expand(ROWS, H, T, dk), 0)
            # what the new entry reads: NaN in every slot past *pos and in every (row, slot) no visible table entry points to; table entries
            # past *pos far outside the caches (they must not be read: clamped, they would reach a NaN row)
            used = torch.zeros(ROWS, T, dtype=torch.bool, device=dev)
            used[table.long()[:, :n].reshape(-1), slot[:n].repeat(ROWS)] = True
            k_p = torch.where(used[:, None, :, None], kc, torch.full_like(kc, NAN))
            v_p = torch.where(used[:, None, :, None], vc, torch.full_like(vc, NAN))
            t_p = table.clone()
            t_p[:, n:] = 1 << 30
            b_p = torch.full_like(bias, NAN)
            b_p[:, pos, :n] = bias[:, pos, :n]
            kg_p, vg_p = kg.clone(), vg.clone()
            kg_p[:, :, n:], vg_p[:, :, n:] = NAN, NAN
            ref, out = torch.full((ROWS, H * dk), NAN, dtype=dtype, device=dev), torch.full((ROWS, H * dk), NAN, dtype=dtype, device=dev)
            L.check(L.lib().vtgb_llm_attention_rows(C.byref(_args(L, dtype, H, dk, T, scale, q, kg_p, vg_p, b_p, pos_t, ref)), _stream()))
            L.check(L.lib().vtgb_llm_attention_rows_beam(C.byref(_args(L, dtype, H, dk, T, scale, q, k_p, v_p, b_p, pos_t, out)), t_p.data_ptr(), T, ROWS,
                                                         _stream()))
            torch.cuda.synchronize()
            assert torch.isfinite(out).all(), (name, pos)
            assert torch.equal(out, ref) and R.same_bits(out, ref), (name, pos, (out.float() - ref.float()).abs().max().item())
            # the gathered reference against fp64 with HF's roundings
            s = rnd(torch.einsum("bhd,bhtd->bht", q.double().view(ROWS, H, dk), kg[:, :, :n].double()) * scale)
            s = rnd(s + bias[:, pos, :n].double()[None])
            want = torch.einsum("bht,bhtd->bhd", rnd(torch.softmax(s, -1)), vg[:, :, :n].double()).reshape(ROWS, H * dk)
            err = (ref.double() - want).abs().max().item()
            assert err <= _attn_tol(dtype) * want.abs().max().item(), (name, pos, err)


def test_a_wrong_entry_at_a_visible_slot_is_clamped_and_a_wider_table_stride_is_taken(dev):
    """Entries below 0 read row 0, entries past the caches read the last row -- wrong numbers for a wrong table, never a read outside; the
    table's row stride may exceed t_pad (the decoder's is t_pad + 1)."""
    from videotgb_amd import _lib as L
    from videotgb_amd import ops
    dtype, H, dk, T, pos = BF16, 4, 64, 64, 40
    q = _randn((ROWS, H * dk), 21, dev, dtype)
    kc, vc = _randn((ROWS, H, T, dk), 22, dev, dtype), _randn((ROWS, H, T, dk), 23, dev, dtype)
    bias = _randn((H, T, T), 24, dev, dtype)
    pos_t = torch.tensor([pos], device=dev)
    wide = torch.full((ROWS, T + 1), -5, dtype=torch.int32, device=dev)
    wide[:, 1::2] = 1 << 20
    clamped = wide.clamp(0, ROWS - 1)[:, :T].contiguous()
    out = ops.attention_rows_beam(q, kc, vc, wide, pos_t, 0.125, bias=bias)
    ref = ops.attention_rows_beam(q, kc, vc, clamped, pos_t, 0.125, bias=bias)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.equal(out, ref)
    idx = clamped.long()[:, None, :, None].expand(ROWS, H, T, dk)
    plain = torch.empty_like(out)
    a = _args(L, dtype, H, dk, T, 0.125, q, torch.take_along_dim(kc, idx, 0), torch.take_along_dim(vc, idx, 0), bias, pos_t, plain)
    L.check(L.lib().vtgb_llm_attention_rows(C.byref(a), _stream()))
    torch.cuda.synchronize()
    assert torch.equal(out, plain)
