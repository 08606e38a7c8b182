"""CPU-side checks of the beam attention over fp8 K/V caches (vtgb_llm_decode_attention_beam_fp8): declared in include/vtgb.h, exported by the
built library and bound in _lib.py; bad arguments are rejected on the host before any launch (the pointers are never dereferenced); the ABI
version is unchanged."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -4      # include/vtgb.h
NAME = "vtgb_llm_decode_attention_beam_fp8"
POINTERS = ("q", "kp8", "vp8", "kps", "vps", "kg8", "vg8", "kgs", "vgs", "src_row", "out", "n_prompt", "pos", "key_valid", "workspace")


@pytest.fixture(scope="module")
def lib():
    from videotgb_amd import build
    build.build()
    from videotgb_amd import _lib
    return _lib


def test_the_entry_is_declared_exported_and_bound(lib):
    h = open(os.path.join(REPO, "include", "vtgb.h")).read()
    assert re.search(r"\bint\s+vtgb_llm_decode_attention_beam_fp8\s*\(\s*const vtgb_llm_decode_attention_beam_fp8_args\* a, vtgb_stream_t stream\)", h)
    assert "} vtgb_llm_decode_attention_beam_fp8_args;" in h
    L = lib.lib()
    fn = getattr(L, NAME)
    assert NAME in lib.EXPORTS and fn.restype is C.c_int and len(fn.argtypes) == 2
    # the struct as the header lays it out: 8 int32 + float, padding to 8, 15 pointers -- and field for field in the header's order
    S = lib.LlmDecodeAttentionBeamFp8Args
    assert C.sizeof(S) == 9 * 4 + 4 + 15 * 8
    body = h[h.rindex("typedef struct {", 0, h.index("} vtgb_llm_decode_attention_beam_fp8_args;")):h.index("} vtgb_llm_decode_attention_beam_fp8_args;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n for stmt in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", stmt.split("{")[-1].strip())]
    assert declared == [n for n, _ in S._fields_], (declared, [n for n, _ in S._fields_])
    assert [n for n, t in S._fields_ if t is C.c_void_p] == list(POINTERS)
    assert L.vtgb_version() == 601
    assert not hasattr(L, NAME + "_workspace_bytes")      # the workspace is vtgb_llm_decode_attention_split_workspace_bytes'


def _attn(lib, **kw):
    p = 0x1000      # never dereferenced: every case below is rejected on the host
    d = dict(dtype=lib.BF16, R=6, K=3, nq=4, nkv=2, hd=128, tmax_p=320, tmax_g=64, scale=0.088, key_valid=None)
    d.update({n: p for n in POINTERS if n != "key_valid"})
    d.update(kw)
    return lib.lib().vtgb_llm_decode_attention_beam_fp8(C.byref(lib.LlmDecodeAttentionBeamFp8Args(**d)), None)


REJECTED = [(dict([(n, None)]), EINVAL, b"NULL") for n in POINTERS if n != "key_valid"] + [
    (dict(dtype=0), EINVAL, b"VTGB_BF16"), (dict(dtype=3), EINVAL, b"bad argument"),
    (dict(R=0), EINVAL, b"bad argument"), (dict(K=0), EINVAL, b"bad argument"), (dict(nq=0), EINVAL, b"bad argument"), (dict(nkv=-1), EINVAL, b"bad argument"),
    (dict(tmax_p=0), EINVAL, b"bad argument"), (dict(tmax_g=0), EINVAL, b"bad argument"),
    (dict(R=7), EINVAL, b"K=3"), (dict(nq=4, nkv=3), EINVAL, b"nkv"),
    (dict(hd=96), EUNSUPPORTED, b"hd=96"), (dict(hd=256), EUNSUPPORTED, b"hd=256"), (dict(tmax_p=100), EUNSUPPORTED, b"tmax_p=100"),
    (dict(tmax_g=32), EUNSUPPORTED, b"tmax_g=32"), (dict(tmax_p=16384), EUNSUPPORTED, b"16384"),
] + [(dict([(n, 0x1008)]), EUNSUPPORTED, b"alignment") for n in ("q", "kp8", "vp8", "kg8", "vg8", "out", "workspace")] + [
    (dict([(n, 0x1002)]), EUNSUPPORTED, b"alignment") for n in ("kps", "vps", "kgs", "vgs", "src_row")]


@pytest.mark.parametrize("kw,code,word", REJECTED, ids=[f"{next(iter(k))}={next(iter(k.values()))}" for k, _, _ in REJECTED])
def test_bad_arguments_are_rejected_on_the_host(lib, kw, code, word):
    assert _attn(lib, **kw) == code
    assert word in lib.lib().vtgb_last_error() and b"llm_decode_attention_beam_fp8" in lib.lib().vtgb_last_error()
    with pytest.raises(ValueError if code == EINVAL else NotImplementedError):
        lib.check(code)


def test_null_args(lib):
    assert lib.lib().vtgb_llm_decode_attention_beam_fp8(None, None) == EINVAL


def test_limits_as_ops_states_them(lib):
    from videotgb_amd import ops
    assert ops.decode_attention_beam_fp8_ok(320, 64, 128) and ops.decode_attention_beam_fp8_ok(64, 64, 64) and ops.decode_attention_beam_fp8_ok(16320, 64, 128)
    assert not ops.decode_attention_beam_fp8_ok(320, 64, 96) and not ops.decode_attention_beam_fp8_ok(16384, 64, 128)
    assert not ops.decode_attention_beam_fp8_ok(300, 64, 64) and not ops.decode_attention_beam_fp8_ok(320, 32, 64) and not ops.decode_attention_beam_fp8_ok(320, 0, 64)
