"""CPU-side checks of the entries of csrc/llm.hip: the rejections they make on the host before any launch.  A missing guard would let a
call reach a launch with these operands on the GPU."""
import ctypes as C

import pytest

EINVAL, EUNSUPPORTED = -1, -4      # include/vtgb.h
P = 0x1000                         # a 16-byte aligned non-NULL operand; never dereferenced: every case below is rejected on the host


@pytest.fixture(scope="module")
def lib():
    from videotgb_amd import build
    build.build()
    from videotgb_amd import _lib
    return _lib


def _rejected(lib, rc, code, word):
    assert rc == code
    assert word in lib.lib().vtgb_last_error()
    with pytest.raises(ValueError if code == EINVAL else NotImplementedError):
        lib.check(rc)


@pytest.mark.parametrize("kw", [dict(rows=0), dict(H=0), dict(x=None), dict(w=None), dict(h=None),
                                dict(x=None, delta=None, w=None, h=None)])
def test_rmsnorm_rejects(lib, kw):
    d = dict(dtype=lib.BF16, x=P, delta=P, w=P, h=P, rows=3, H=4096, eps=1e-6)
    d.update(kw)
    rc = lib.lib().vtgb_llm_rmsnorm(d["dtype"], d["x"], d["delta"], d["w"], d["h"], d["rows"], d["H"], d["eps"], None)
    _rejected(lib, rc, EINVAL, b"llm_rmsnorm: bad argument")


@pytest.mark.parametrize("kw,code,word", [
    (dict(dtype="f32"), EINVAL, b"llm_rmsnorm_parts: bad argument"), (dict(S=1), EINVAL, b"llm_rmsnorm_parts: bad argument"),
    (dict(rows=129), EINVAL, b"llm_rmsnorm_parts: bad argument"), (dict(x=None, part=None, w=None, h=None), EINVAL, b"llm_rmsnorm_parts: bad argument"),
    (dict(H=1024), EUNSUPPORTED, b"hidden size 1024"),
])
def test_rmsnorm_parts_rejects(lib, kw, code, word):
    d = dict(dtype="bf16", x=P, part=P, S=2, w=P, h=P, rows=3, H=4096, eps=1e-6)
    d.update(kw)
    dt = lib.BF16 if d["dtype"] == "bf16" else lib.F32
    rc = lib.lib().vtgb_llm_rmsnorm_parts(dt, d["x"], d["part"], d["S"], d["w"], d["h"], d["rows"], d["H"], d["eps"], None)
    _rejected(lib, rc, code, word)


@pytest.mark.parametrize("kw", [dict(hd=15), dict(cos=None), dict(sin=None), dict(qkv=None, q=None, kc=None, vc=None, cos=None, sin=None, pos=None)])
def test_rope_cache_rejects(lib, kw):
    d = dict(qkv=P, q=P, kc=P, vc=P, cos=P, sin=P, pos=P, B=2, nq=4, nkv=2, hd=16, tmax=64)
    d.update(kw)
    rc = lib.lib().vtgb_llm_rope_cache(lib.F32, d["qkv"], d["q"], d["kc"], d["vc"], d["cos"], d["sin"], d["pos"], d["B"], d["nq"], d["nkv"], d["hd"],
                                       d["tmax"], None)
    _rejected(lib, rc, EINVAL, b"llm_rope_cache: bad argument")


@pytest.mark.parametrize("kw", [dict(B=129), dict(dtype="f32"), dict(part=None, q=None, kc=None, vc=None, cos=None, sin=None, pos=None)])
def test_rope_cache_parts_rejects(lib, kw):
    d = dict(dtype="bf16", part=P, S=2, q=P, kc=P, vc=P, cos=P, sin=P, pos=P, B=2, nq=4, nkv=2, hd=64, tmax=64)
    d.update(kw)
    dt = lib.BF16 if d["dtype"] == "bf16" else lib.F32
    rc = lib.lib().vtgb_llm_rope_cache_parts(dt, d["part"], d["S"], d["q"], d["kc"], d["vc"], d["cos"], d["sin"], d["pos"], d["B"], d["nq"], d["nkv"],
                                             d["hd"], d["tmax"], None)
    _rejected(lib, rc, EINVAL, b"llm_rope_cache_parts: bad argument")


@pytest.mark.parametrize("kw,code,word", [
    (dict(S=65), EINVAL, b"llm_rope_cache_prefill: bad argument"),
    (dict(qkv=None, kc=None, vc=None, cos=None, sin=None), EINVAL, b"llm_rope_cache_prefill: bad argument"),
    (dict(dtype="bf16", hd=24), EUNSUPPORTED, b"head_dim=24"), (dict(dtype="f32", hd=12), EUNSUPPORTED, b"head_dim=12"),
])
def test_rope_cache_prefill_rejects(lib, kw, code, word):
    d = dict(dtype="bf16", qkv=P, kc=P, vc=P, cos=P, sin=P, B=2, S=8, nq=4, nkv=2, hd=64, tmax=64)
    d.update(kw)
    dt = lib.BF16 if d["dtype"] == "bf16" else lib.F32
    rc = lib.lib().vtgb_llm_rope_cache_prefill(dt, d["qkv"], d["kc"], d["vc"], d["cos"], d["sin"], d["B"], d["S"], d["nq"], d["nkv"], d["hd"], d["tmax"],
                                               None)
    _rejected(lib, rc, code, word)


@pytest.mark.parametrize("kw,code,word", [
    (dict(nq=4, nkv=3), EINVAL, b"llm_decode_attention: bad argument"),
    (dict(q=None, kc=None, vc=None, out=None, pos=None), EINVAL, b"llm_decode_attention: bad argument"),
    (dict(tmax=2049), EUNSUPPORTED, b"tmax=2049"), (dict(hd=257), EUNSUPPORTED, b"hd=257"),
])
def test_decode_attention_rejects(lib, kw, code, word):
    d = dict(q=P, kc=P, vc=P, out=P, pos=P, B=2, nq=4, nkv=2, hd=64, tmax=128, scale=0.125)
    d.update(kw)
    rc = lib.lib().vtgb_llm_decode_attention(lib.BF16, d["q"], d["kc"], d["vc"], d["out"], d["pos"], d["B"], d["nq"], d["nkv"], d["hd"], d["tmax"],
                                             d["scale"], None)
    _rejected(lib, rc, code, word)


def test_silu_mul_and_gated_act_reject(lib):
    L = lib.lib()
    _rejected(lib, L.vtgb_llm_silu_mul(lib.BF16, P, P, 3, 0, None), EINVAL, b"llm_silu_mul: bad argument")
    _rejected(lib, L.vtgb_llm_silu_mul(lib.BF16, None, None, 3, 8, None), EINVAL, b"llm_silu_mul: bad argument")
    for kind in (-1, 4):
        _rejected(lib, L.vtgb_llm_gated_act(lib.F32, P, P, 3, 8, kind, 1, None), EINVAL, b"llm_gated_act: bad argument")
    _rejected(lib, L.vtgb_llm_gated_act(lib.F32, None, None, 3, 8, 1, 1, None), EINVAL, b"llm_gated_act: bad argument")


@pytest.mark.parametrize("kw,code,word", [
    (dict(pos=None, n_keys=0), EINVAL, b"n_keys or pos"), (dict(q=None, k=None, v=None, out=None), EINVAL, b"llm_attention_rows: bad argument"),
    (dict(t_pad=36, n_keys=37), EUNSUPPORTED, b"t_pad=36"), (dict(t_pad=2049), EUNSUPPORTED, b"t_pad=2049"),
    (dict(head_dim=257), EUNSUPPORTED, b"head_dim=257"),
])
def test_attention_rows_rejects(lib, kw, code, word):
    d = dict(dtype=lib.F32, rows=4, heads=2, head_dim=16, rows_per_batch=4, n_keys=4, t_pad=4, scale=1.0, q=P, q_row=96, k=P, v=P, kv_batch=8 * 96,
             kv_head=16, kv_tok=96, bias=None, bias_pos=0, bias_head=0, pos=None, out=P, o_row=32)
    d.update(kw)
    a = lib.LlmAttnRowsArgs(*[d[name] for name, _ in lib.LlmAttnRowsArgs._fields_])
    _rejected(lib, lib.lib().vtgb_llm_attention_rows(C.byref(a), None), code, word)
