"""CPU-side checks of the eos-set entries (vtgb_llm_pick_greedy, vtgb_llm_beam_candidates_eos): declared in include/vtgb.h, exported by the
built library and bound in _lib.py; bad arguments are rejected on the host before any launch (the pointers are never dereferenced); the ABI
version is unchanged and the one-id beam entry keeps its structure."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -4      # include/vtgb.h
NAMES = ("vtgb_llm_pick_greedy", "vtgb_llm_beam_candidates_eos")


@pytest.fixture(scope="module")
def lib():
    from videotgb_amd import build
    build.build()
    from videotgb_amd import _lib
    return _lib


def test_symbols_are_declared_exported_and_bound(lib):
    h = open(os.path.join(REPO, "include", "vtgb.h")).read()
    assert re.search(r"\bint\s+vtgb_llm_pick_greedy\s*\(\s*const vtgb_llm_pick_greedy_args\* a, vtgb_stream_t stream\)", h)
    assert re.search(r"\bint\s+vtgb_llm_beam_candidates_eos\s*\(\s*const vtgb_llm_beam_candidates_eos_args\* a, vtgb_stream_t stream\)", h)
    assert "} vtgb_llm_pick_greedy_args;" in h and "} vtgb_llm_beam_candidates_eos_args;" in h
    assert re.search(r"#define\s+VTGB_LLM_EOS_MAX\s+8\b", h)
    assert "NaN" in h[h.index("vtgb_llm_pick_greedy:"):h.index("#define VTGB_LLM_EOS_MAX")]      # the header says what is not specified
    L = lib.lib()
    for n in NAMES:
        assert n in lib.EXPORTS and getattr(L, n).restype is C.c_int and len(getattr(L, n).argtypes) == 2
    from videotgb_amd import build, ops
    assert "emit.hip" in build.SOURCES and "beam.hip" in build.SOURCES
    assert ops.EOS_MAX == 8
    assert C.sizeof(lib.LlmPickGreedyArgs) == 6 * 4 + 8 + 6 * 8 and C.sizeof(lib.LlmBeamCandidatesEosArgs) == 8 * 4 + 9 * 8
    assert C.sizeof(lib.LlmBeamCandidatesArgs) == 8 * 4 + 8 * 8      # the one-id entry's structure is what it was
    assert L.vtgb_version() == 601


def test_the_header_and_the_binding_name_the_same_fields(lib):
    h = open(os.path.join(REPO, "include", "vtgb.h")).read()
    for struct, cls in (("vtgb_llm_pick_greedy_args", lib.LlmPickGreedyArgs), ("vtgb_llm_beam_candidates_eos_args", lib.LlmBeamCandidatesEosArgs)):
        body = h[:h.index("} " + struct + ";")]
        body = re.sub(r"/\*.*?\*/", "", body[body.rindex("typedef struct {"):], flags=re.S)
        declared = [n for line in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", line.split("{")[-1].strip())]
        assert declared == [n for n, _ in cls._fields_], (struct, declared)


def _pick(lib, **kw):
    p = 0x1000      # never dereferenced: every case below is rejected on the host
    d = dict(dtype=lib.BF16, B=3, V=32003, N=16, min_new=0, n_eos=3, pad=0, logits=p, step=p, eos_ids=p, fin=p, tok=p, out=p)
    d.update(kw)
    return lib.lib().vtgb_llm_pick_greedy(C.byref(lib.LlmPickGreedyArgs(**d)), None)


@pytest.mark.parametrize("kw,code,word", [
    (dict(logits=None), EINVAL, b"NULL"), (dict(step=None), EINVAL, b"NULL"), (dict(eos_ids=None), EINVAL, b"NULL"), (dict(fin=None), EINVAL, b"NULL"),
    (dict(tok=None), EINVAL, b"NULL"), (dict(out=None), EINVAL, b"NULL"),
    (dict(dtype=2), EINVAL, b"bad argument"), (dict(dtype=3), EINVAL, b"bad argument"), (dict(B=0), EINVAL, b"bad argument"),
    (dict(B=-1), EINVAL, b"bad argument"), (dict(V=0), EINVAL, b"bad argument"), (dict(V=-5), EINVAL, b"bad argument"), (dict(N=0), EINVAL, b"bad argument"),
    (dict(n_eos=-1), EINVAL, b"n_eos=-1"), (dict(n_eos=9), EINVAL, b"n_eos=9"),
    (dict(logits=0x1008), EUNSUPPORTED, b"alignment"), (dict(logits=0x1002), EUNSUPPORTED, b"alignment"), (dict(step=0x1004), EUNSUPPORTED, b"alignment"),
    (dict(tok=0x1004), EUNSUPPORTED, b"alignment"), (dict(out=0x1004), EUNSUPPORTED, b"alignment"), (dict(eos_ids=0x1002), EUNSUPPORTED, b"alignment"),
])
def test_pick_rejects_bad_arguments_on_the_host(lib, kw, code, word):
    assert _pick(lib, **kw) == code
    assert word in lib.lib().vtgb_last_error()
    with pytest.raises(ValueError if code == EINVAL else NotImplementedError):
        lib.check(code)


def test_null_args_are_rejected(lib):
    L = lib.lib()
    assert L.vtgb_llm_pick_greedy(None, None) == EINVAL and b"NULL args" in L.vtgb_last_error()
    assert L.vtgb_llm_beam_candidates_eos(None, None) == EINVAL and b"NULL args" in L.vtgb_last_error()


def _cand(lib, **kw):
    p = 0x1000
    d = dict(dtype=lib.BF16, R=10, K=5, V=32000, N=64, n_eos=3, min_new=0, penalty=1.5, logits=p, seq=p, step=p, running=p, eos_ids=p, cand_score=p,
             cand_idx=p, workspace=p, workspace_bytes=10 * 32000 * 4 + 10 * 10 * 8)
    d.update(kw)
    return lib.lib().vtgb_llm_beam_candidates_eos(C.byref(lib.LlmBeamCandidatesEosArgs(**d)), None)


@pytest.mark.parametrize("kw,code,word", [
    (dict(logits=None), EINVAL, b"NULL"), (dict(seq=None), EINVAL, b"NULL"), (dict(step=None), EINVAL, b"NULL"), (dict(running=None), EINVAL, b"NULL"),
    (dict(eos_ids=None), EINVAL, b"NULL"), (dict(cand_score=None), EINVAL, b"NULL"), (dict(cand_idx=None), EINVAL, b"NULL"),
    (dict(workspace=None), EINVAL, b"NULL"),
    (dict(n_eos=-1), EINVAL, b"n_eos=-1"), (dict(n_eos=9), EINVAL, b"n_eos=9"),
    (dict(dtype=2), EINVAL, b"bad argument"), (dict(penalty=0.0), EINVAL, b"bad argument"), (dict(N=-1), EINVAL, b"bad argument"),
    (dict(R=0), EINVAL, b"bad argument"), (dict(V=0), EINVAL, b"bad argument"), (dict(R=11), EINVAL, b"K=5"),
    (dict(R=17, K=17), EUNSUPPORTED, b"K=17"), (dict(V=(1 << 20) + 1), EUNSUPPORTED, b"V=1048577"), (dict(V=9), EUNSUPPORTED, b"2 K=10"),
    (dict(workspace_bytes=10 * 32000 * 4), EUNSUPPORTED, b"workspace"), (dict(workspace=0x1004), EUNSUPPORTED, b"workspace"),
    (dict(eos_ids=0x1002), EUNSUPPORTED, b"alignment"),
])
def test_candidates_eos_reject_bad_arguments_on_the_host(lib, kw, code, word):
    assert _cand(lib, **kw) == code
    assert word in lib.lib().vtgb_last_error()


def test_the_host_range_check_of_the_list():
    """The list lives on the device, so the range check is where it is built: ops.eos_list (here on the host device, where it only builds)."""
    from videotgb_amd import ops
    assert ops.eos_list([5, 5, 0, 31], 32, "cpu").tolist() == [5, 5, 0, 31] and ops.eos_list([], 32, "cpu").dtype.__str__() == "torch.int32"
    for ids in ([32], [-1], [3, 40], list(range(9))):
        with pytest.raises(ValueError):
            ops.eos_list(ids, 32, "cpu")
