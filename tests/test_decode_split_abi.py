"""CPU-side checks of vtgb_llm_decode_attention_split (the decode step's split-KV attention): declared in include/vtgb.h, exported by
the built library and bound in _lib.py; the workspace size follows the documented layout; bad arguments are rejected on the host before
any launch; the routing between the two decode-attention kernels as a pure function; the ABI version is unchanged."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -4      # include/vtgb.h
NAMES = ("vtgb_llm_decode_attention_split_workspace_bytes", "vtgb_llm_decode_attention_split")


@pytest.fixture(scope="module")
def lib():
    from videotgb_amd import build
    build.build()
    from videotgb_amd import _lib
    return _lib


def _header():
    return open(os.path.join(REPO, "include", "vtgb.h")).read()


def test_symbols_are_declared_exported_and_bound(lib):
    h = _header()
    assert re.search(r"\bint64_t\s+vtgb_llm_decode_attention_split_workspace_bytes\s*\(\s*int32_t B, int32_t nq, int32_t hd, int32_t tmax\)", h)
    assert re.search(r"\bint\s+vtgb_llm_decode_attention_split\s*\(\s*int dtype, const void\* q, const void\* kc, const void\* vc, void\* out", h)
    L = lib.lib()
    for n in NAMES:
        assert n in lib.EXPORTS and getattr(L, n) is not None
    assert L.vtgb_llm_decode_attention_split_workspace_bytes.restype is C.c_int64
    assert L.vtgb_llm_decode_attention_split.restype is C.c_int and len(L.vtgb_llm_decode_attention_split.argtypes) == 15
    assert L.vtgb_version() == 601


def test_workspace_bytes_follow_the_documented_layout(lib):
    # float O[B * nq][NC][hd] + float ml[B * nq][NC][2], NC = ceil(tmax / 256)
    ws = lib.lib().vtgb_llm_decode_attention_split_workspace_bytes
    assert ws(2, 4, 128, 2112) == 2 * 4 * 9 * (128 + 2) * 4
    assert ws(124, 32, 64, 4096) == 124 * 32 * 16 * (64 + 2) * 4
    assert 0 < ws(1, 32, 128, 256) < ws(1, 32, 128, 320) < ws(1, 32, 128, 16384)
    assert ws(1, 32, 128, 64) == ws(1, 32, 128, 256)      # one chunk


def _call(lib, **kw):
    p = 0x1000      # never dereferenced: every case below is rejected on the host
    d = dict(dtype=lib.BF16, q=p, kc=p, vc=p, out=p, pos=p, key_valid=None, workspace=p, B=2, nq=4, nkv=2, hd=128, tmax=2112, scale=0.088)
    d.update(kw)
    return lib.lib().vtgb_llm_decode_attention_split(d["dtype"], d["q"], d["kc"], d["vc"], d["out"], d["pos"], d["key_valid"], d["workspace"], d["B"],
                                                     d["nq"], d["nkv"], d["hd"], d["tmax"], d["scale"], None)


@pytest.mark.parametrize("kw,code,word", [
    (dict(q=None), EINVAL, b"NULL"), (dict(kc=None), EINVAL, b"NULL"), (dict(vc=None), EINVAL, b"NULL"), (dict(out=None), EINVAL, b"NULL"),
    (dict(pos=None), EINVAL, b"NULL"), (dict(workspace=None), EINVAL, b"NULL"),
    (dict(nq=4, nkv=3), EINVAL, b"nkv"), (dict(B=0), EINVAL, b"bad argument"),
    (dict(hd=96), EUNSUPPORTED, b"hd=96"), (dict(hd=256), EUNSUPPORTED, b"hd=256"),
    (dict(tmax=16448), EUNSUPPORTED, b"tmax=16448"), (dict(tmax=100), EUNSUPPORTED, b"tmax=100"),
    (dict(q=0x1008), EUNSUPPORTED, b"alignment"), (dict(kc=0x1002), EUNSUPPORTED, b"alignment"), (dict(vc=0x1004), EUNSUPPORTED, b"alignment"),
    (dict(out=0x1008), EUNSUPPORTED, b"alignment"), (dict(workspace=0x1004), EUNSUPPORTED, b"alignment"),
])
def test_bad_arguments_are_rejected_on_the_host(lib, kw, code, word):
    assert _call(lib, **kw) == code
    assert word in lib.lib().vtgb_last_error()
    with pytest.raises(ValueError if code == EINVAL else NotImplementedError):
        lib.check(code)


def test_routing_is_a_pure_monotone_function_of_the_cache_length(lib):
    from videotgb_amd import ops
    from videotgb_amd.decode import GreedyDecoder
    assert GreedyDecoder.DECODE_SPLIT_MIN_KEYS == ops.DECODE_SPLIT_MIN_KEYS
    assert 384 <= ops.DECODE_SPLIT_MIN_KEYS <= 2112 and ops.DECODE_SPLIT_MIN_KEYS % 64 == 0
    for hd in (64, 128):
        assert ops.decode_attention_route(128, hd) == "single" and ops.decode_attention_route(320, hd) == "single"
        assert ops.decode_attention_route(2112, hd) == "split" and ops.decode_attention_route(4096, hd) == "split"
        routes = [ops.decode_attention_route(t, hd) for t in range(64, 16384 + 64, 64)]
        first = routes.index("split")
        assert set(routes[:first]) == {"single"} and set(routes[first:]) == {"split"}      # monotone: one threshold
        assert (first + 1) * 64 == ops.DECODE_SPLIT_MIN_KEYS
        assert ops.decode_attention_route(16384 + 64, hd) is None
    # a head_dim only the one-wave kernel takes: that kernel to its 2048 slots, then neither (the decoder's torch step)
    assert ops.decode_attention_route(2048, 96) == "single" and ops.decode_attention_route(2112, 96) is None
    assert ops.decode_attention_route(128, 128, min_keys=64) == "split"
