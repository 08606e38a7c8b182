"""CPU-side checks of the split TGB entries (vtgb_tgb_trunk / vtgb_tgb_resume, the clip sessions' kernels): exported, ctypes mirror
matches the header, host-side validation returns the documented codes, workspace queries work without a GPU."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vtgb_tgb_trunk_workspace_bytes", "vtgb_tgb_trunk", "vtgb_tgb_resume_workspace_bytes", "vtgb_tgb_resume")


@pytest.fixture(scope="module")
def lib():
    from videotgb_amd import build
    build.build()
    from videotgb_amd import _lib
    return _lib


def split_args(lib, B=1, n_text=14, mode=2, dtype=None, L=96):
    """BERT-base TGB geometry (hidden 768, 12 heads, 12 layers, fusion_layer 6) on 224 x 224 flow."""
    return lib.TgbSplitArgs(lib.BF16 if dtype is None else dtype, B, L, n_text, 768, 12, 3072, 12, 6, mode, 224, 16, 1e-12,
                            None, None, None, None, None, None, None, None, None, None, 0)


def test_new_symbols_exported_and_declared(lib):
    hdr = open(os.path.join(REPO, "include", "vtgb.h")).read()
    declared = set(re.findall(r"\b(vtgb_[a-z0-9_]+)\s*\(", hdr))
    L = lib.lib()
    for name in NEW:
        assert name in declared and name in lib.EXPORTS, name
        assert hasattr(L, name), name
    assert "vtgb_tgb_split_args" in hdr
    assert L.vtgb_version() == 601


def test_split_struct_size_follows_header(lib):
    # 12 int32 + float eps = 52 bytes, padded to 56; 9 pointers (of, of_mask, text_ids, text_mask, weights, trunk, trunk_act, seq_out,
    # logits); workspace pointer + size_t
    assert C.sizeof(lib.TgbSplitArgs) == 56 + 9 * 8 + 8 + 8
    assert C.sizeof(lib.TgbSplitArgs) == C.sizeof(lib.TgbArgs) + 2 * 8
    names = [f[0] for f in lib.TgbSplitArgs._fields_]
    assert names[names.index("weights") + 1:names.index("weights") + 3] == ["trunk", "trunk_act"]


def test_workspace_queries_reject_bad_mode(lib):
    L = lib.lib()
    for fn in (L.vtgb_tgb_trunk_workspace_bytes, L.vtgb_tgb_resume_workspace_bytes):
        a = split_args(lib, mode=7)
        assert fn(C.byref(a)) == 0
        assert b"INVALID MODE" in L.vtgb_last_error()


def test_workspace_queries_reject_empty_rows(lib):
    L = lib.lib()
    assert L.vtgb_tgb_trunk_workspace_bytes(C.byref(split_args(lib, B=0))) == 0
    assert L.vtgb_tgb_trunk_workspace_bytes(C.byref(split_args(lib, B=2))) == 0      # the trunk is one clip
    assert L.vtgb_tgb_resume_workspace_bytes(C.byref(split_args(lib, B=0))) == 0
    assert L.vtgb_tgb_resume_workspace_bytes(C.byref(split_args(lib, B=3, n_text=0))) == 0
    assert b"bad dims" in L.vtgb_last_error()
    assert L.vtgb_tgb_resume_workspace_bytes(C.byref(split_args(lib, dtype=5))) == 0


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("B", [1, 3, 25])
def test_resume_workspace_is_smaller_than_forward(lib, mode, B):
    L = lib.lib()
    for dt in (lib.BF16, lib.F32):
        fwd = lib.TgbArgs(dt, B, 96, 14, 768, 12, 3072, 12, 6, mode, 224, 16, 1e-12, None, None, None, None, None, None, None, None, 0)
        f = L.vtgb_tgb_workspace_bytes(C.byref(fwd))
        r = L.vtgb_tgb_resume_workspace_bytes(C.byref(split_args(lib, B=B, mode=mode, dtype=dt)))
        t = L.vtgb_tgb_trunk_workspace_bytes(C.byref(split_args(lib, B=1, mode=mode, dtype=dt)))
        assert 0 < r < f, (dt, mode, B, r, f)
        assert 0 < t, (dt, mode)
        if B == 1:
            assert t < f


def test_launch_entries_need_a_workspace(lib):
    L = lib.lib()
    a = split_args(lib)
    assert L.vtgb_tgb_trunk(C.byref(a), None) == -2
    assert b"workspace" in L.vtgb_last_error()
    a = split_args(lib, B=3)
    assert L.vtgb_tgb_resume(C.byref(a), None) == -2
    assert b"workspace" in L.vtgb_last_error()


def test_launch_entries_validate_pointers_before_launching(lib):
    """A workspace of the queried size but NULL tensors: VTGB_EINVAL on the host, nothing launched (a host buffer stands in for the
    workspace: it is never touched)."""
    L = lib.lib()
    for fn, q, B in ((L.vtgb_tgb_trunk, L.vtgb_tgb_trunk_workspace_bytes, 1), (L.vtgb_tgb_resume, L.vtgb_tgb_resume_workspace_bytes, 2)):
        a = split_args(lib, B=B)
        need = q(C.byref(a))
        buf = C.create_string_buffer(16)
        a.workspace, a.workspace_bytes = C.cast(buf, C.c_void_p), need
        assert fn(C.byref(a), None) == -1
        assert b"required" in L.vtgb_last_error()
