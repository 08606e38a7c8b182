"""CPU-side checks of the entries of csrc/train_llm.hip: the rejections they make on the host before any launch.  A missing guard would let a
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
    assert word in lib.lib().vtgb_last_error(), lib.lib().vtgb_last_error()
    with pytest.raises(ValueError if code == EINVAL else NotImplementedError):
        lib.check(rc)


def _attn(lib, **kw):
    d = dict(batch=2, heads=4, head_dim=64, s_q=10, s_kv=10, q=P, k=P, v=P, q_tok=768, kv_tok=768, q_batch=7680, kv_batch=7680, key_mask=None, drop=None,
             scale=0.125, out=P, o_tok=256, o_batch=2560, lse=P, dout=P, dq=P, dk=P, dv=P, delta=P)
    d.update(kw)
    return lib.AttnTrainArgs(*[d[n] for n, _ in lib.AttnTrainArgs._fields_])


@pytest.mark.parametrize("kw,kv_heads,code,word", [
    (dict(s_kv=11), 2, EINVAL, b"s_q=10 and s_kv=11 differ"),
    (dict(), 3, EINVAL, b"heads=4 is no multiple of kv_heads=3"),
    (dict(drop=P), 2, EINVAL, b"drop must be NULL"),
    (dict(head_dim=130), 2, EUNSUPPORTED, b"head_dim=130"),
    (dict(), 0, EINVAL, b"bad dims"),
    (dict(batch=0), 2, EINVAL, b"bad dims"),
    (dict(q=None), 2, EINVAL, b"NULL operand"),
    (dict(k=None), 2, EINVAL, b"NULL operand"),
    (dict(lse=None), 2, EINVAL, b"NULL operand"),
])
def test_causal_attention_rejects(lib, kw, kv_heads, code, word):
    a = _attn(lib, **kw)
    _rejected(lib, lib.lib().vtgb_attn_train_causal_forward(C.byref(a), kv_heads, None), code, word)
    _rejected(lib, lib.lib().vtgb_attn_train_causal_backward(C.byref(a), kv_heads, None), code, word)


def test_causal_attention_rejects_null_args_and_gradient_operands(lib):
    _rejected(lib, lib.lib().vtgb_attn_train_causal_forward(None, 2, None), EINVAL, b"NULL args")
    _rejected(lib, lib.lib().vtgb_attn_train_causal_backward(None, 2, None), EINVAL, b"NULL args")
    for name in ("dout", "dq", "dk", "dv", "delta"):
        a = _attn(lib, **{name: None})
        _rejected(lib, lib.lib().vtgb_attn_train_causal_backward(C.byref(a), 2, None), EINVAL, b"NULL gradient operand")


def _norm(lib, **kw):
    d = dict(rows=3, D=4096, eps=1e-6, x=P, delta=P, gamma=P, sum=P, y=P, rstd=P, dy=P, ds=P, dsum=None)
    d.update(kw)
    return lib.RmsNormTrainArgs(*[d[n] for n, _ in lib.RmsNormTrainArgs._fields_])


@pytest.mark.parametrize("kw,code,word", [
    (dict(D=8196), EUNSUPPORTED, b"D=8196"), (dict(D=30), EUNSUPPORTED, b"D=30"), (dict(rows=0), EINVAL, b"bad dims"),
    (dict(gamma=None), EINVAL, b"NULL argument"), (dict(rstd=None), EINVAL, b"NULL argument"),
])
def test_rmsnorm_rejects_both_ways(lib, kw, code, word):
    a = _norm(lib, **kw)
    _rejected(lib, lib.lib().vtgb_rmsnorm_train_forward(C.byref(a), None), code, word)
    _rejected(lib, lib.lib().vtgb_rmsnorm_train_backward(C.byref(a), None), code, word)


def test_rmsnorm_rejects_by_direction(lib):
    L = lib.lib()
    _rejected(lib, L.vtgb_rmsnorm_train_forward(None, None), EINVAL, b"NULL argument")
    _rejected(lib, L.vtgb_rmsnorm_train_backward(None, None), EINVAL, b"NULL argument")
    for kw in (dict(x=None), dict(y=None)):
        _rejected(lib, L.vtgb_rmsnorm_train_forward(C.byref(_norm(lib, **kw)), None), EINVAL, b"NULL x / y")
    _rejected(lib, L.vtgb_rmsnorm_train_forward(C.byref(_norm(lib, sum=None)), None), EINVAL, b"`sum` is required with a delta")
    _rejected(lib, L.vtgb_rmsnorm_train_forward(C.byref(_norm(lib, x=P + 4)), None), EINVAL, b"16-byte aligned")
    for kw in (dict(sum=None), dict(dy=None), dict(ds=None)):
        _rejected(lib, L.vtgb_rmsnorm_train_backward(C.byref(_norm(lib, **kw)), None), EINVAL, b"NULL sum / dy / ds")
    _rejected(lib, L.vtgb_rmsnorm_train_backward(C.byref(_norm(lib, dsum=P + 8)), None), EINVAL, b"16-byte aligned")


@pytest.mark.parametrize("kw,code,word", [
    (dict(hd=15), EINVAL, b"hd=15"), (dict(hd=130), EUNSUPPORTED, b"head_dim=130"), (dict(S=0), EINVAL, b"bad argument"), (dict(nkv=0), EINVAL, b"bad argument"),
    (dict(x=None), EINVAL, b"NULL operand"), (dict(y=None), EINVAL, b"NULL operand"), (dict(cos=None), EINVAL, b"NULL operand"),
    (dict(sin=None), EINVAL, b"NULL operand"), (dict(y=P), EINVAL, b"y must not be x"),
])
def test_rope_rejects(lib, kw, code, word):
    d = dict(x=P, y=2 * P, cos=P, sin=P, B=2, S=5, nh=4, nkv=2, hd=16)
    d.update(kw)
    for conjugate in (0, 1):
        rc = lib.lib().vtgb_rope_train(d["x"], d["y"], d["cos"], d["sin"], d["B"], d["S"], d["nh"], d["nkv"], d["hd"], conjugate, None)
        _rejected(lib, rc, code, word)


@pytest.mark.parametrize("kw", [dict(gu=None), dict(other=None), dict(M=0), dict(I=0), dict(gu=None, other=None, dgu=None)])
def test_swiglu_rejects(lib, kw):
    d = dict(gu=P, other=P, dgu=P, M=3, I=64)
    d.update(kw)
    _rejected(lib, lib.lib().vtgb_swiglu_train_forward(d["gu"], d["other"], d["M"], d["I"], None), EINVAL, b"swiglu_train_forward")
    _rejected(lib, lib.lib().vtgb_swiglu_train_backward(d["gu"], d["other"], d["dgu"], d["M"], d["I"], None), EINVAL, b"swiglu_train_backward")
    _rejected(lib, lib.lib().vtgb_swiglu_train_backward(P, P, None, 3, 64, None), EINVAL, b"swiglu_train_backward")


def test_struct_size_of_the_new_args(lib):
    assert C.sizeof(lib.RmsNormTrainArgs) == 2 * 4 + 4 + 4 + 9 * 8          # rows, D, eps (+ pad), nine pointers
