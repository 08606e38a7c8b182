"""CPU-side checks of the beam-search entries (vtgb_llm_decode_attention_beam, vtgb_llm_beam_candidates): declared in include/vtgb.h, exported
by the built library and bound in _lib.py; bad arguments are rejected on the host before any launch (the pointers are never dereferenced);
the ABI version is unchanged."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -4      # include/vtgb.h
NAMES = ("vtgb_llm_decode_attention_beam", "vtgb_llm_beam_candidates")


@pytest.fixture(scope="module")
def lib():
    from videotgb_amd import build
    build.build()
    from videotgb_amd import _lib
    return _lib


def test_symbols_are_declared_exported_and_bound(lib):
    h = open(os.path.join(REPO, "include", "vtgb.h")).read()
    assert re.search(r"\bint\s+vtgb_llm_decode_attention_beam\s*\(\s*const vtgb_llm_decode_attention_beam_args\* a, vtgb_stream_t stream\)", h)
    assert re.search(r"\bint\s+vtgb_llm_beam_candidates\s*\(\s*const vtgb_llm_beam_candidates_args\* a, vtgb_stream_t stream\)", h)
    assert "} vtgb_llm_decode_attention_beam_args;" in h and "} vtgb_llm_beam_candidates_args;" in h
    L = lib.lib()
    for n in NAMES:
        assert n in lib.EXPORTS and getattr(L, n).restype is C.c_int and len(getattr(L, n).argtypes) == 2
    from videotgb_amd import build
    assert "beam.hip" in build.SOURCES
    assert C.sizeof(lib.LlmDecodeAttentionBeamArgs) == 9 * 4 + 4 + 11 * 8 and C.sizeof(lib.LlmBeamCandidatesArgs) == 8 * 4 + 8 * 8
    assert L.vtgb_version() == 601


def _attn(lib, **kw):
    p = 0x1000      # never dereferenced: every case below is rejected on the host
    d = dict(dtype=lib.BF16, R=6, K=3, nq=4, nkv=2, hd=128, tmax_p=320, tmax_g=64, scale=0.088, q=p, kp=p, vp=p, kg=p, vg=p, src_row=p, out=p,
             n_prompt=p, pos=p, key_valid=None, workspace=p)
    d.update(kw)
    return lib.lib().vtgb_llm_decode_attention_beam(C.byref(lib.LlmDecodeAttentionBeamArgs(**d)), None)


@pytest.mark.parametrize("kw,code,word", [
    (dict(q=None), EINVAL, b"NULL"), (dict(kp=None), EINVAL, b"NULL"), (dict(vp=None), EINVAL, b"NULL"), (dict(kg=None), EINVAL, b"NULL"),
    (dict(vg=None), EINVAL, b"NULL"), (dict(src_row=None), EINVAL, b"NULL"), (dict(out=None), EINVAL, b"NULL"), (dict(n_prompt=None), EINVAL, b"NULL"),
    (dict(pos=None), EINVAL, b"NULL"), (dict(workspace=None), EINVAL, b"NULL"),
    (dict(dtype=3), EINVAL, b"bad argument"), (dict(R=0), EINVAL, b"bad argument"), (dict(tmax_g=0), EINVAL, b"bad argument"),
    (dict(R=7), EINVAL, b"K=3"), (dict(nq=4, nkv=3), EINVAL, b"nkv"),
    (dict(hd=96), EUNSUPPORTED, b"hd=96"), (dict(tmax_p=100), EUNSUPPORTED, b"tmax_p=100"), (dict(tmax_g=32), EUNSUPPORTED, b"tmax_g=32"),
    (dict(tmax_p=16384), EUNSUPPORTED, b"16384"),
    (dict(q=0x1008), EUNSUPPORTED, b"alignment"), (dict(kg=0x1004), EUNSUPPORTED, b"alignment"), (dict(src_row=0x1002), EUNSUPPORTED, b"alignment"),
    (dict(workspace=0x1008), EUNSUPPORTED, b"alignment"),
])
def test_attention_rejects_bad_arguments_on_the_host(lib, kw, code, word):
    assert _attn(lib, **kw) == code
    assert word in lib.lib().vtgb_last_error()
    with pytest.raises(ValueError if code == EINVAL else NotImplementedError):
        lib.check(code)


def _cand(lib, **kw):
    p = 0x1000
    d = dict(dtype=lib.BF16, R=10, K=5, V=32000, N=64, eos=2, min_new=0, penalty=1.5, logits=p, seq=p, step=p, running=p, cand_score=p, cand_idx=p,
             workspace=p, workspace_bytes=10 * 32000 * 4 + 10 * 10 * 8)
    d.update(kw)
    return lib.lib().vtgb_llm_beam_candidates(C.byref(lib.LlmBeamCandidatesArgs(**d)), None)


@pytest.mark.parametrize("kw,code,word", [
    (dict(logits=None), EINVAL, b"NULL"), (dict(seq=None), EINVAL, b"NULL"), (dict(step=None), EINVAL, b"NULL"), (dict(running=None), EINVAL, b"NULL"),
    (dict(cand_score=None), EINVAL, b"NULL"), (dict(cand_idx=None), EINVAL, b"NULL"), (dict(workspace=None), EINVAL, b"NULL"),
    (dict(dtype=2), EINVAL, b"bad argument"), (dict(penalty=0.0), EINVAL, b"bad argument"), (dict(N=-1), EINVAL, b"bad argument"),
    (dict(R=11), EINVAL, b"K=5"),
    (dict(R=17, K=17), EUNSUPPORTED, b"K=17"), (dict(V=(1 << 20) + 1), EUNSUPPORTED, b"V=1048577"), (dict(V=9), EUNSUPPORTED, b"2 K=10"),
    (dict(workspace_bytes=10 * 32000 * 4), EUNSUPPORTED, b"workspace"), (dict(workspace=0x1004), EUNSUPPORTED, b"workspace"),
])
def test_candidates_reject_bad_arguments_on_the_host(lib, kw, code, word):
    assert _cand(lib, **kw) == code
    assert word in lib.lib().vtgb_last_error()


def test_workspace_and_limits_as_ops_states_them(lib):
    from videotgb_amd import ops
    assert ops.beam_candidates_workspace_bytes(10, 5, 32000) == 10 * 32000 * 4 + 10 * 10 * 8
    assert ops.BEAM_MAX_BEAMS == 16 and ops.BEAM_MAX_VOCAB == 1 << 20
    assert ops.decode_attention_beam_ok(320, 64, 128) and not ops.decode_attention_beam_ok(320, 64, 96)
    assert not ops.decode_attention_beam_ok(16384, 64, 128) and not ops.decode_attention_beam_ok(300, 64, 64)
