"""CPU-side checks of vtgb_llm_lora_parts (the K-split reduce of a deferred projection and the LoRA update in one launch): declared in
include/vtgb.h, exported by the built library and bound in _lib.py; every bad argument is rejected on the host, before any launch, with
its code and a message; the entry was added without an ABI version bump (the existing entries are unchanged)."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -4      # include/vtgb.h


@pytest.fixture(scope="module")
def lib():
    from videotgb_amd import build
    build.build()
    from videotgb_amd import _lib
    return _lib


def test_symbol_is_declared_exported_and_bound(lib):
    h = open(os.path.join(REPO, "include", "vtgb.h")).read()
    assert re.search(r"\bint\s+vtgb_llm_lora_parts\s*\(\s*const vtgb_llm_lora_args\*\s*a,\s*const float\*\s*part,\s*int32_t n_splits,\s*vtgb_stream_t stream\)", h)
    L = lib.lib()
    assert "vtgb_llm_lora_parts" in lib.EXPORTS and L.vtgb_llm_lora_parts is not None
    assert L.vtgb_llm_lora_parts.restype is C.c_int
    assert L.vtgb_llm_lora_parts.argtypes == [C.POINTER(lib.LlmLoraArgs), C.c_void_p, C.c_int32, C.c_void_p]
    assert L.vtgb_version() == 601
    from videotgb_amd import ops
    assert callable(ops.lora_update_parts)


P = 0x1000      # never dereferenced: every case below is rejected on the host


def _seg(**kw):
    s = dict(A=P, B=P, r=8, n=32, col0=0, scaling=4.0)
    s.update(kw)
    return s


def _call(lib, segs=None, part=P, n_splits=2, **kw):
    d = dict(dtype=lib.BF16, K=64, n_cols=112, n_seg=None, rows=5, ldx=64, ldy=112, x=P, y=P)
    d.update(kw)
    segs = [_seg(), _seg(n=40, col0=64)] if segs is None else segs
    a = lib.LlmLoraArgs(d["dtype"], d["K"], d["n_cols"], len(segs) if d["n_seg"] is None else d["n_seg"], d["rows"], d["ldx"], d["ldy"], d["x"], d["y"])
    for i, s in enumerate(segs[:4]):
        a.seg[i] = lib.LlmLoraSeg(s["A"], s["B"], s["r"], s["n"], s["col0"], s["scaling"])
    return lib.lib().vtgb_llm_lora_parts(C.byref(a), part, n_splits, None)


@pytest.mark.parametrize("kw,code,word", [
    # vtgb_llm_lora's own checks
    (dict(x=None), EINVAL, b"NULL"), (dict(y=None), EINVAL, b"NULL"),
    (dict(segs=[_seg(A=None)]), EINVAL, b"NULL"), (dict(segs=[_seg(B=None)]), EINVAL, b"NULL"),
    (dict(dtype=2), EINVAL, b"dtype"),
    (dict(n_seg=0), EINVAL, b"n_seg=0"), (dict(n_seg=5), EINVAL, b"n_seg=5"),
    (dict(segs=[_seg(r=0)]), EINVAL, b"r=0"), (dict(segs=[_seg(r=65)]), EINVAL, b"r=65"),
    (dict(rows=0), EINVAL, b"positive"), (dict(K=0), EINVAL, b"positive"),
    (dict(ldx=60), EINVAL, b"row stride"), (dict(ldy=104), EINVAL, b"row stride"),
    (dict(segs=[_seg(col0=96, n=32)]), EINVAL, b"past"), (dict(segs=[_seg(n=0)]), EINVAL, b"past"),
    (dict(segs=[_seg(col0=0, n=32), _seg(col0=31, n=8)]), EINVAL, b"overlap"),
    (dict(K=62, ldx=64), EUNSUPPORTED, b"multiples of 4"), (dict(x=0x1004), EUNSUPPORTED, b"aligned"), (dict(y=0x1001), EUNSUPPORTED, b"aligned"),
    (dict(segs=[_seg(A=0x1008)]), EUNSUPPORTED, b"aligned"), (dict(segs=[_seg(B=0x1002)]), EUNSUPPORTED, b"aligned"),
    # its own
    (dict(dtype=0), EINVAL, b"VTGB_BF16"),                                      # fp32 x / y: vtgb_llm_lora takes them, this entry does not
    (dict(rows=129), EINVAL, b"rows=129"),
    (dict(n_splits=1), EINVAL, b"n_splits=1"), (dict(n_splits=0), EINVAL, b"n_splits=0"), (dict(n_splits=65), EINVAL, b"n_splits=65"),
    (dict(n_splits=-2), EINVAL, b"n_splits"),
    (dict(part=None), EINVAL, b"NULL part"),
    (dict(part=0x1002), EUNSUPPORTED, b"4-byte aligned"),
])
def test_bad_arguments_are_rejected_on_the_host(lib, kw, code, word):
    assert _call(lib, **kw) == code
    assert word in lib.lib().vtgb_last_error()
    with pytest.raises(ValueError if code == EINVAL else NotImplementedError):
        lib.check(code)


def test_null_args_are_rejected(lib):
    assert lib.lib().vtgb_llm_lora_parts(None, P, 2, None) == EINVAL
    assert b"NULL" in lib.lib().vtgb_last_error()
