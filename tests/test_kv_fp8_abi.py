"""CPU-side checks of the fp8 K/V cache entries (vtgb_llm_decode_attention_split_fp8, vtgb_llm_rope_cache_fp8,
vtgb_llm_rope_cache_prefill_fp8): declared in include/vtgb.h, exported by the built library and bound in _lib.py; bad arguments are
rejected on the host before any launch, with the codes of the bf16 split entry; the workspace is the shared one; the ABI version is
unchanged."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -4      # include/vtgb.h
NAMES = ("vtgb_llm_decode_attention_split_fp8", "vtgb_llm_rope_cache_fp8", "vtgb_llm_rope_cache_prefill_fp8")
P = 0x1000      # never dereferenced: every case below is rejected on the host


@pytest.fixture(scope="module")
def lib():
    from videotgb_amd import build
    build.build()
    from videotgb_amd import _lib
    return _lib


def test_symbols_are_declared_exported_and_bound(lib):
    h = open(os.path.join(REPO, "include", "vtgb.h")).read()
    assert re.search(r"\bint\s+vtgb_llm_decode_attention_split_fp8\s*\(\s*int dtype, const void\* q, const uint8_t\* kc8, const uint8_t\* vc8, "
                     r"const float\* ks, const float\* vs, void\* out", h)
    assert re.search(r"\bint\s+vtgb_llm_rope_cache_fp8\s*\(\s*const vtgb_llm_rope_cache_fp8_args\* a, vtgb_stream_t stream\)", h)
    assert re.search(r"\bint\s+vtgb_llm_rope_cache_prefill_fp8\s*\(\s*int dtype, void\* qkv, uint8_t\* kc8, uint8_t\* vc8, float\* ks, float\* vs", h)
    assert "} vtgb_llm_rope_cache_fp8_args;" in h
    L = lib.lib()
    for n in NAMES:
        assert n in lib.EXPORTS and getattr(L, n).restype is C.c_int
    assert len(L.vtgb_llm_decode_attention_split_fp8.argtypes) == 17 and len(L.vtgb_llm_rope_cache_prefill_fp8.argtypes) == 16
    assert [f[0] for f in lib.LlmRopeCacheFp8Args._fields_] == ["dtype", "B", "nq", "nkv", "hd", "tmax", "n_splits", "qkv", "part", "q_out", "kc8",
                                                                 "vc8", "ks", "vs", "cos_t", "sin_t", "pos", "rope_off"]
    assert L.vtgb_version() == 601


def test_the_workspace_is_the_split_entrys(lib):
    """No workspace function of its own: ops.decode_attention_fp8 sizes its scratch with the bf16 split entry's."""
    from videotgb_amd import ops
    L = lib.lib()
    assert not hasattr(L, "vtgb_llm_decode_attention_split_fp8_workspace_bytes")
    for B, nq, hd, tmax in ((2, 4, 128, 1024), (124, 32, 128, 320), (1, 32, 64, 16384), (3, 16, 64, 64)):
        assert ops.decode_attention_workspace_bytes(B, nq, hd, tmax) == L.vtgb_llm_decode_attention_split_workspace_bytes(B, nq, hd, tmax) \
            == B * nq * -(-tmax // 256) * (hd + 2) * 4
    assert ops.decode_attention_fp8_ok(64, 128) and ops.decode_attention_fp8_ok(16384, 64)
    assert not ops.decode_attention_fp8_ok(100, 128) and not ops.decode_attention_fp8_ok(16448, 128) and not ops.decode_attention_fp8_ok(320, 96)


def _attn(lib, **kw):
    d = dict(dtype=lib.BF16, q=P, kc8=P, vc8=P, ks=P, vs=P, out=P, pos=P, key_valid=None, workspace=P, B=2, nq=4, nkv=2, hd=128, tmax=1024, scale=0.088)
    d.update(kw)
    return lib.lib().vtgb_llm_decode_attention_split_fp8(d["dtype"], d["q"], d["kc8"], d["vc8"], d["ks"], d["vs"], d["out"], d["pos"], d["key_valid"],
                                                         d["workspace"], d["B"], d["nq"], d["nkv"], d["hd"], d["tmax"], d["scale"], None)


@pytest.mark.parametrize("kw,code,word", [
    (dict(q=None), EINVAL, b"NULL"), (dict(kc8=None), EINVAL, b"NULL"), (dict(vc8=None), EINVAL, b"NULL"), (dict(ks=None), EINVAL, b"NULL"),
    (dict(vs=None), EINVAL, b"NULL"), (dict(out=None), EINVAL, b"NULL"), (dict(pos=None), EINVAL, b"NULL"), (dict(workspace=None), EINVAL, b"NULL"),
    (dict(nq=4, nkv=3), EINVAL, b"nkv"), (dict(B=0), EINVAL, b"bad argument"), (dict(dtype=0), EINVAL, b"VTGB_BF16"),      # 0 = VTGB_F32
    (dict(hd=96), EUNSUPPORTED, b"hd=96"), (dict(hd=256), EUNSUPPORTED, b"hd=256"),
    (dict(tmax=16448), EUNSUPPORTED, b"tmax=16448"), (dict(tmax=100), EUNSUPPORTED, b"tmax=100"),
    (dict(q=0x1008), EUNSUPPORTED, b"alignment"), (dict(kc8=0x1008), EUNSUPPORTED, b"alignment"), (dict(vc8=0x1004), EUNSUPPORTED, b"alignment"),
    (dict(ks=0x1002), EUNSUPPORTED, b"alignment"), (dict(vs=0x1001), EUNSUPPORTED, b"alignment"),
    (dict(out=0x1008), EUNSUPPORTED, b"alignment"), (dict(workspace=0x1004), EUNSUPPORTED, b"alignment"),
])
def test_attention_rejects_bad_arguments_on_the_host(lib, kw, code, word):
    assert lib.F32 == 0
    assert _attn(lib, **kw) == code
    assert word in lib.lib().vtgb_last_error()
    with pytest.raises(ValueError if code == EINVAL else NotImplementedError):
        lib.check(code)


def _append(lib, **kw):
    d = dict(dtype=lib.BF16, B=2, nq=4, nkv=2, hd=128, tmax=1024, n_splits=0, qkv=P, part=None, q_out=P, kc8=P, vc8=P, ks=P, vs=P, cos_t=P, sin_t=P,
             pos=P, rope_off=None)
    d.update(kw)
    a = lib.LlmRopeCacheFp8Args(*(d[f[0]] for f in lib.LlmRopeCacheFp8Args._fields_))
    return lib.lib().vtgb_llm_rope_cache_fp8(C.byref(a), None)


@pytest.mark.parametrize("kw,code,word", [
    (dict(q_out=None), EINVAL, b"NULL"), (dict(kc8=None), EINVAL, b"NULL"), (dict(vc8=None), EINVAL, b"NULL"), (dict(ks=None), EINVAL, b"NULL"),
    (dict(vs=None), EINVAL, b"NULL"), (dict(cos_t=None), EINVAL, b"NULL"), (dict(sin_t=None), EINVAL, b"NULL"), (dict(pos=None), EINVAL, b"NULL"),
    (dict(qkv=None), EINVAL, b"exactly one"), (dict(part=P, n_splits=2), EINVAL, b"exactly one"),
    (dict(qkv=None, part=P, n_splits=1), EINVAL, b"n_splits"), (dict(qkv=None, part=P, n_splits=2, B=129), EINVAL, b"n_splits"),
    (dict(dtype=0), EINVAL, b"VTGB_BF16"), (dict(B=0), EINVAL, b"bad argument"), (dict(tmax=0), EINVAL, b"bad argument"),
    (dict(hd=96), EUNSUPPORTED, b"hd=96"),
])
def test_append_rejects_bad_arguments_on_the_host(lib, kw, code, word):
    assert _append(lib, **kw) == code
    assert word in lib.lib().vtgb_last_error()
    assert lib.lib().vtgb_llm_rope_cache_fp8(None, None) == EINVAL


def _prefill(lib, **kw):
    d = dict(dtype=lib.BF16, qkv=P, kc8=P, vc8=P, ks=P, vs=P, cos_t=P, sin_t=P, pos_ids=None, B=2, S=9, nq=4, nkv=2, hd=128, tmax=64)
    d.update(kw)
    return lib.lib().vtgb_llm_rope_cache_prefill_fp8(d["dtype"], d["qkv"], d["kc8"], d["vc8"], d["ks"], d["vs"], d["cos_t"], d["sin_t"], d["pos_ids"],
                                                     d["B"], d["S"], d["nq"], d["nkv"], d["hd"], d["tmax"], None)


@pytest.mark.parametrize("kw,code,word", [
    (dict(qkv=None), EINVAL, b"NULL"), (dict(kc8=None), EINVAL, b"NULL"), (dict(vc8=None), EINVAL, b"NULL"), (dict(ks=None), EINVAL, b"NULL"),
    (dict(vs=None), EINVAL, b"NULL"), (dict(cos_t=None), EINVAL, b"NULL"), (dict(sin_t=None), EINVAL, b"NULL"),
    (dict(dtype=0), EINVAL, b"VTGB_BF16"), (dict(S=0), EINVAL, b"bad argument"), (dict(S=65), EINVAL, b"bad argument"),
    (dict(hd=96), EUNSUPPORTED, b"hd=96"),
])
def test_prefill_rejects_bad_arguments_on_the_host(lib, kw, code, word):
    assert _prefill(lib, **kw) == code
    assert word in lib.lib().vtgb_last_error()
