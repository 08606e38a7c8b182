"""CPU-side checks of vtgb_gemm_skinny_bias (the decode step's projections with a bias, either weight stream): declared in include/vtgb.h,
exported by the built library and bound in _lib.py; bad arguments are rejected on the host before any launch, the shape before the operands;
the argument structure and the ABI version are unchanged."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4      # include/vtgb.h
P = 0x1000      # never dereferenced: every case below is rejected on the host


@pytest.fixture(scope="module")
def lib():
    from videotgb_amd import build
    build.build()
    from videotgb_amd import _lib
    return _lib


def test_symbol_is_declared_exported_and_bound(lib):
    h = open(os.path.join(REPO, "include", "vtgb.h")).read()
    assert re.search(r"\bint\s+vtgb_gemm_skinny_bias\s*\(\s*const vtgb_gemm_skinny_args\* a, const float\* w_scale[^,]*, const float\* bias[^,]*,\s*vtgb_stream_t stream\)", h)
    L = lib.lib()
    assert "vtgb_gemm_skinny_bias" in lib.EXPORTS and L.vtgb_gemm_skinny_bias.restype is C.c_int and len(L.vtgb_gemm_skinny_bias.argtypes) == 4
    assert C.sizeof(lib.GemmSkinnyArgs) == 96      # M N K n_splits | x ldx | w ldw | out ldo | out_dtype w_tiled | workspace | bytes | defer_reduce (+ pad)
    assert L.vtgb_version() == 601


def _call(lib, w_scale=None, bias=P, **kw):
    d = dict(M=4, N=256, K=512, n_splits=1, x=P, ldx=512, w=P, ldw=512, out=P, ldo=256, out_dtype=lib.BF16, w_tiled=0, workspace=None, workspace_bytes=0,
             defer_reduce=0)
    d.update(kw)
    a = lib.GemmSkinnyArgs(*(d[k] for k, _ in lib.GemmSkinnyArgs._fields_))
    return lib.lib().vtgb_gemm_skinny_bias(C.byref(a), w_scale, bias, None)


@pytest.mark.parametrize("kw,code,word", [
    (dict(bias=None), EINVAL, b"NULL"), (dict(x=None), EINVAL, b"NULL"), (dict(w=None), EINVAL, b"NULL"), (dict(out=None), EINVAL, b"NULL"),
    (dict(bias=None, w_scale=P, w_tiled=1), EINVAL, b"NULL"),
    (dict(bias=0x1002), EUNSUPPORTED, b"4-byte aligned"), (dict(bias=0x1001, w_scale=P, w_tiled=1), EUNSUPPORTED, b"4-byte aligned"),
    (dict(w_scale=P, w_tiled=0), EINVAL, b"w_tiled"),
    # everything skinny_check checks, as the plain entries report it -- and before the operands
    (dict(M=129), EUNSUPPORTED, b"M=129"), (dict(M=0), EUNSUPPORTED, b"M=0"), (dict(K=100), EUNSUPPORTED, b"K=100"), (dict(N=0), EUNSUPPORTED, b"N=0"),
    (dict(M=129, bias=None), EUNSUPPORTED, b"M=129"),
    (dict(ldx=508), EINVAL, b"row pitches"), (dict(ldo=255), EINVAL, b"row pitches"), (dict(ldw=500), EINVAL, b"row pitches"),
    (dict(out_dtype=7), EINVAL, b"out_dtype"), (dict(n_splits=65), EINVAL, b"n_splits"), (dict(n_splits=-1), EINVAL, b"n_splits"),
    # a K split without its workspace
    (dict(n_splits=2), EWORKSPACE, b"gemm_skinny_bias: workspace"), (dict(n_splits=2, workspace=P, workspace_bytes=16), EWORKSPACE, b"workspace"),
])
def test_bad_arguments_are_rejected_on_the_host(lib, kw, code, word):
    assert _call(lib, **kw) == code
    assert word in lib.lib().vtgb_last_error(), lib.lib().vtgb_last_error()
    with pytest.raises({EINVAL: ValueError, EUNSUPPORTED: NotImplementedError}.get(code, Exception)):
        lib.check(code)


def test_null_args(lib):
    assert lib.lib().vtgb_gemm_skinny_bias(None, None, P, None) == EINVAL


def test_ops_takes_an_optional_bias():
    import inspect
    from videotgb_amd import ops
    assert inspect.signature(ops.gemm_skinny).parameters["bias"].default is None
