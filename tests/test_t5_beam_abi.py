"""CPU-side checks of vtgb_llm_attention_rows_beam (beam search on the T5 decode step): declared in include/vtgb.h, exported by the built
library and bound in _lib.py; bad arguments are rejected on the host before any launch (the pointers are never dereferenced); the limit is a
named constant that ops.py states as well; the ABI version is unchanged."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -4      # include/vtgb.h
NAME = "vtgb_llm_attention_rows_beam"


@pytest.fixture(scope="module")
def lib():
    from videotgb_amd import build
    build.build()
    from videotgb_amd import _lib
    return _lib


def test_the_symbol_is_declared_exported_and_bound(lib):
    h = open(os.path.join(REPO, "include", "vtgb.h")).read()
    assert re.search(r"\bint\s+vtgb_llm_attention_rows_beam\s*\(\s*const vtgb_llm_attn_rows_args\* a, const int32_t\* src_row, int64_t src_row_stride, "
                     r"int32_t cache_rows,\s*vtgb_stream_t stream\)", h)
    L = lib.lib()
    fn = getattr(L, NAME)
    assert NAME in lib.EXPORTS and fn.restype is C.c_int and len(fn.argtypes) == 5
    assert L.vtgb_version() == 601


def test_the_limit_is_one_named_constant(lib):
    from videotgb_amd import ops
    h = open(os.path.join(REPO, "include", "vtgb.h")).read()
    m = re.search(r"#define\s+VTGB_LLM_ATTN_ROWS_BEAM_MAX_T\s+(\d+)", h)
    assert m and int(m.group(1)) == ops.ATTENTION_ROWS_BEAM_MAX_KEYS == 1920
    # four waves of (head_dim <= 256 floats of q, t_pad scores, t_pad table rows): what a launch gets without asking for more than 64 KiB
    assert 4 * (256 + 2 * ops.ATTENTION_ROWS_BEAM_MAX_KEYS) * 4 <= 64 * 1024 < 4 * (256 + 2 * (ops.ATTENTION_ROWS_BEAM_MAX_KEYS + 64)) * 4


def _call(lib, src_row=0x1000, stride=64, cache_rows=6, **kw):
    p = 0x1000      # never dereferenced: every case below is rejected on the host
    d = dict(dtype=lib.BF16, rows=6, heads=4, head_dim=64, rows_per_batch=1, n_keys=0, t_pad=64, scale=1.0, q=p, q_row=256, k=p, v=p, kv_batch=4 * 64 * 64,
             kv_head=64 * 64, kv_tok=64, bias=p, bias_pos=64, bias_head=64 * 64, pos=p, out=p, o_row=256)
    d.update(kw)
    return lib.lib().vtgb_llm_attention_rows_beam(C.byref(lib.LlmAttnRowsArgs(**d)), src_row, stride, cache_rows, None)


@pytest.mark.parametrize("kw,code,word", [
    (dict(src_row=None), EINVAL, b"llm_attention_rows_beam"), (dict(pos=None, n_keys=8), EINVAL, b"llm_attention_rows_beam"),
    (dict(pos=None), EINVAL, b"n_keys or pos"), (dict(cache_rows=0), EINVAL, b"cache_rows"), (dict(cache_rows=-3), EINVAL, b"cache_rows"),
    (dict(stride=63), EINVAL, b"stride"), (dict(t_pad=192, stride=191), EINVAL, b"stride"),
    # what attn_rows_check refuses
    (dict(q=None), EINVAL, b"bad argument"), (dict(k=None), EINVAL, b"bad argument"), (dict(out=None), EINVAL, b"bad argument"),
    (dict(rows=0), EINVAL, b"bad argument"), (dict(rows_per_batch=0), EINVAL, b"bad argument"),
    (dict(t_pad=0), EUNSUPPORTED, b"t_pad=0"), (dict(head_dim=257), EUNSUPPORTED, b"head_dim=257"), (dict(t_pad=2049, stride=4096), EUNSUPPORTED, b"t_pad=2049"),
    # the LDS limit of the staged table
    (dict(t_pad=1921, stride=1921), EUNSUPPORTED, b"t_pad=1921"), (dict(t_pad=2048, stride=2048), EUNSUPPORTED, b"t_pad=2048"),
])
def test_bad_arguments_are_rejected_on_the_host(lib, kw, code, word):
    assert _call(lib, **kw) == code
    assert word in lib.lib().vtgb_last_error(), lib.lib().vtgb_last_error()
    with pytest.raises(ValueError if code == EINVAL else NotImplementedError):
        lib.check(code)
