"""CPU-side checks of the repetition-penalty entry (vtgb_llm_repetition_penalty): declared in include/vtgb.h, exported by the built library and
bound in _lib.py with the same fields; bad arguments are rejected on the host before any launch (the pointers are never dereferenced); the
ABI version is unchanged."""
import ctypes as C
import inspect
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -4      # include/vtgb.h
NAME = "vtgb_llm_repetition_penalty"


@pytest.fixture(scope="module")
def lib():
    from videotgb_amd import build
    build.build()
    from videotgb_amd import _lib
    return _lib


def test_the_symbol_is_declared_exported_and_bound(lib):
    h = open(os.path.join(REPO, "include", "vtgb.h")).read()
    assert re.search(r"\bint\s+vtgb_llm_repetition_penalty\s*\(\s*const vtgb_llm_repetition_penalty_args\* a, vtgb_stream_t stream\)", h)
    assert "} vtgb_llm_repetition_penalty_args;" in h
    L = lib.lib()
    assert NAME in lib.EXPORTS and getattr(L, NAME).restype is C.c_int and len(getattr(L, NAME).argtypes) == 2
    from videotgb_amd import build, ops
    assert "emit.hip" in build.SOURCES
    assert C.sizeof(lib.LlmRepetitionPenaltyArgs) == 6 * 4 + 4 * 8
    assert C.sizeof(lib.LlmPickGreedyArgs) == 6 * 4 + 8 + 6 * 8      # the neighbouring entry's structure is what it was
    assert L.vtgb_version() == 601
    assert list(inspect.signature(ops.repetition_penalty).parameters) == ["logits", "seq", "step", "penalty", "start_id", "out"]
    p = inspect.signature(ops.repetition_penalty).parameters
    assert p["start_id"].default is None and p["out"].default is None


def test_the_header_and_the_binding_name_the_same_fields(lib):
    h = open(os.path.join(REPO, "include", "vtgb.h")).read()
    body = h[:h.index("} vtgb_llm_repetition_penalty_args;")]
    body = re.sub(r"/\*.*?\*/", "", body[body.rindex("typedef struct {"):], flags=re.S)
    declared = [n for line in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", line.split("{")[-1].strip())]
    assert declared == [n for n, _ in lib.LlmRepetitionPenaltyArgs._fields_], declared
    assert declared == ["dtype", "R", "V", "N", "start_id", "penalty", "logits", "seq", "step", "out"]


def _call(lib, **kw):
    p = 0x1000      # never dereferenced: every case below is rejected on the host
    d = dict(dtype=lib.BF16, R=3, V=32003, N=16, start_id=-1, penalty=1.5, logits=p, seq=p, step=p, out=p)
    d.update(kw)
    return lib.lib().vtgb_llm_repetition_penalty(C.byref(lib.LlmRepetitionPenaltyArgs(**d)), None)


@pytest.mark.parametrize("kw,code,word", [
    (dict(logits=None), EINVAL, b"NULL"), (dict(seq=None), EINVAL, b"NULL"), (dict(step=None), EINVAL, b"NULL"), (dict(out=None), EINVAL, b"NULL"),
    (dict(dtype=2), EINVAL, b"bad argument"), (dict(dtype=3), EINVAL, b"bad argument"), (dict(dtype=-1), EINVAL, b"bad argument"),
    (dict(R=0), EINVAL, b"bad argument"), (dict(R=-1), EINVAL, b"bad argument"), (dict(V=0), EINVAL, b"bad argument"), (dict(V=-5), EINVAL, b"bad argument"),
    (dict(N=0), EINVAL, b"bad argument"), (dict(N=-3), EINVAL, b"bad argument"),
    (dict(penalty=0.0), EINVAL, b"penalty"), (dict(penalty=-1.5), EINVAL, b"penalty"), (dict(penalty=float("inf")), EINVAL, b"penalty"),
    (dict(penalty=float("nan")), EINVAL, b"penalty"), (dict(penalty=-0.0), EINVAL, b"penalty"),
    (dict(R=65536), EUNSUPPORTED, b"R=65536"),
    (dict(logits=0x1008), EUNSUPPORTED, b"alignment"), (dict(logits=0x1002), EUNSUPPORTED, b"alignment"), (dict(out=0x1008), EUNSUPPORTED, b"alignment"),
    (dict(out=0x1004), EUNSUPPORTED, b"alignment"), (dict(seq=0x1004), EUNSUPPORTED, b"alignment"), (dict(step=0x1004), EUNSUPPORTED, b"alignment"),
])
def test_bad_arguments_are_rejected_on_the_host(lib, kw, code, word):
    assert _call(lib, **kw) == code
    assert word in lib.lib().vtgb_last_error()
    with pytest.raises(ValueError if code == EINVAL else NotImplementedError):
        lib.check(code)


def test_null_args_are_rejected(lib):
    L = lib.lib()
    assert L.vtgb_llm_repetition_penalty(None, None) == EINVAL and b"NULL args" in L.vtgb_last_error()


def test_the_wrapper_takes_device_tensors_only():
    import torch
    from videotgb_amd import _lib, ops
    with pytest.raises(_lib.VtgbError):
        ops.repetition_penalty(torch.zeros(1, 8), torch.zeros(1, 4, dtype=torch.long), torch.zeros(1, dtype=torch.long), 1.5)
