"""CPU-side checks of vtgb_raft_layer1_h8 (the unit entry of one layer1 convolution of the RAFT encoders at f16c8: variant 0 = the implicit GEMM, 1 = the
row-resident kernel, 2 = the row-resident kernel + the moments in the GEMM's order): declared in include/vtgb.h, exported by the built library and bound in
_lib.py with a struct of the declared layout; bad arguments are rejected on the host before any launch; the row-resident kernel refuses the sizes it does
not take while the implicit GEMM takes them; the ABI version is unchanged."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4      # include/vtgb.h
F32, PAIR_BF16, PAIR_F16C8 = 0, 1, 2               # VTGB_CONV_OUT_*


@pytest.fixture(scope="module")
def lib():
    from videotgb_amd import build
    build.build()
    from videotgb_amd import _lib
    return _lib


def test_symbols_are_declared_exported_and_bound(lib):
    h = open(os.path.join(REPO, "include", "vtgb.h")).read()
    assert re.search(r"\bint\s+vtgb_raft_layer1_h8\s*\(\s*const vtgb_raft_layer1_h8_args\* a, vtgb_stream_t stream\)", h)
    assert re.search(r"\bsize_t\s+vtgb_raft_layer1_h8_workspace_bytes\s*\(\s*const vtgb_raft_layer1_h8_args\* a\)", h)
    L = lib.lib()
    for name in ("vtgb_raft_layer1_h8", "vtgb_raft_layer1_h8_workspace_bytes"):
        assert name in lib.EXPORTS and getattr(L, name) is not None
    assert L.vtgb_raft_layer1_h8.restype is C.c_int and len(L.vtgb_raft_layer1_h8.argtypes) == 2
    assert L.vtgb_raft_layer1_h8_workspace_bytes.restype is C.c_size_t and len(L.vtgb_raft_layer1_h8_workspace_bytes.argtypes) == 1
    assert L.vtgb_version() == 601
    assert getattr(L, "vtgb_debug_set_l1_h8") is not None      # the same-process A/B switch of the encoders' dispatch


def test_struct_matches_the_header(lib):
    h = open(os.path.join(REPO, "include", "vtgb.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} vtgb_raft_layer1_h8_args;", h).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [x.strip().split()[-1].lstrip("*") for x in decl.split(",")]
    assert names == [f[0] for f in lib.RaftLayer1H8Args._fields_]
    assert C.sizeof(lib.RaftLayer1H8Args) == 5 * 4 + 4 + 8 * 8 + 8      # five int32 (+ padding), seven pointers + the workspace pointer, its size
    assert lib.RaftLayer1H8Args.x.offset == 24 and lib.RaftLayer1H8Args.workspace_bytes.offset == 88


def _args(lib, **kw):
    p = 0x1000      # never dereferenced: every call below ends on the host
    d = dict(n_images=2, H=32, W=32, variant=1, out_kind=F32, x=p, weights=p, bias=p, scale=p, resid=None, out=p, moments=None, workspace=0x10000,
             workspace_bytes=1 << 40)
    d.update(kw)
    return lib.RaftLayer1H8Args(*[d[f[0]] for f in lib.RaftLayer1H8Args._fields_])


def _call(lib, **kw):
    return lib.lib().vtgb_raft_layer1_h8(C.byref(_args(lib, **kw)), None)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("kw,word", [
    (dict(x=None), b"NULL"), (dict(weights=None), b"NULL"), (dict(bias=None), b"NULL"), (dict(scale=None), b"NULL"), (dict(out=None), b"NULL"),
    (dict(out_kind=PAIR_F16C8, out=None), b"NULL"),
    (dict(x=0x1004), b"misaligned"), (dict(weights=0x1008), b"misaligned"), (dict(bias=0x1004), b"misaligned"), (dict(out=0x1008), b"misaligned"),
    (dict(scale=0x1002), b"misaligned"), (dict(workspace=0x10008), b"misaligned"), (dict(out_kind=PAIR_F16C8, resid=0x1002), b"misaligned"),
    (dict(n_images=0), b"bad dims"), (dict(H=0), b"bad dims"), (dict(W=-1), b"bad dims"), (dict(variant=3), b"bad dims"), (dict(variant=-1), b"bad dims"),
    (dict(out_kind=3), b"out_kind"), (dict(out_kind=-1), b"out_kind"),
    (dict(resid=0x1000), b"resid belongs to pair rows"), (dict(out_kind=PAIR_BF16), b"residual tail"),
    (dict(out_kind=PAIR_F16C8, moments=0x1000, variant=0), b"moments belong"), (dict(H=8, W=16, moments=0x1000, variant=0), b"moments belong"),
])
def test_bad_arguments_are_rejected_on_the_host(lib, variant, kw, word):
    kw = dict(kw)
    kw.setdefault("variant", variant)
    assert _call(lib, **kw) == EINVAL
    assert word in lib.lib().vtgb_last_error()
    with pytest.raises(ValueError):
        lib.check(EINVAL)


def test_moments_and_the_variants(lib):
    L = lib.lib()
    assert _call(lib, variant=1, moments=0x1000) == EINVAL and b"variant 1 writes no moments" in L.vtgb_last_error()
    for kw in (dict(moments=None), dict(out_kind=PAIR_F16C8, moments=0x1000), dict(H=8, W=16, moments=0x1000), dict(H=15, W=17, moments=0x1000)):
        assert _call(lib, variant=2, **kw) == EINVAL
        assert b"variant 2" in L.vtgb_last_error()
    assert _call(lib, variant=2, H=16, W=16, moments=0x1000, workspace_bytes=16) == EWORKSPACE      # 256 pixels: taken
    assert _call(lib, variant=2, moments=0x1004) == EINVAL and b"misaligned" in L.vtgb_last_error()
    assert _call(lib, variant=0, moments=0x1000, workspace_bytes=16) == EWORKSPACE                  # the implicit GEMM writes them from its epilogue


def test_null_args_are_rejected(lib):
    assert lib.lib().vtgb_raft_layer1_h8(None, None) == EINVAL
    assert b"NULL" in lib.lib().vtgb_last_error()
    assert lib.lib().vtgb_raft_layer1_h8_workspace_bytes(None) == 0


# sizes the row-resident kernel does not take (16 <= W <= 112, H >= 4) -- the implicit GEMM does
@pytest.mark.parametrize("H,W", [(32, 113), (32, 128), (32, 15), (3, 32), (1, 1)])
@pytest.mark.parametrize("out_kind", [F32, PAIR_F16C8])
def test_row_resident_kernel_refuses_what_the_implicit_gemm_takes(lib, H, W, out_kind):
    L = lib.lib()
    assert _call(lib, H=H, W=W, variant=1, out_kind=out_kind) == EUNSUPPORTED
    assert b"row-resident" in L.vtgb_last_error()
    assert L.vtgb_raft_layer1_h8_workspace_bytes(C.byref(_args(lib, H=H, W=W, variant=1, out_kind=out_kind))) == 0
    need = L.vtgb_raft_layer1_h8_workspace_bytes(C.byref(_args(lib, H=H, W=W, variant=0, out_kind=out_kind)))
    assert need >= 256      # its zero page
    assert _call(lib, H=H, W=W, variant=0, out_kind=out_kind, workspace_bytes=16) == EWORKSPACE
    assert _call(lib, H=H, W=W, variant=0, out_kind=out_kind, workspace=None) == EWORKSPACE


@pytest.mark.parametrize("H,W", [(4, 16), (32, 32), (36, 52), (20, 112), (112, 112)])
def test_row_resident_kernel_takes_its_sizes(lib, H, W):
    L = lib.lib()
    for kw in (dict(), dict(out_kind=PAIR_F16C8), dict(out_kind=PAIR_F16C8, resid=0x1000), dict(out_kind=PAIR_BF16, resid=0x1000)):
        need = L.vtgb_raft_layer1_h8_workspace_bytes(C.byref(_args(lib, H=H, W=W, variant=1, **kw)))
        assert 0 < need <= 512      # no scratch of its own: the zero page the entry keeps for variant 0
        assert _call(lib, H=H, W=W, variant=1, workspace_bytes=16, **kw) == EWORKSPACE
    if H * W >= 256:
        need = L.vtgb_raft_layer1_h8_workspace_bytes(C.byref(_args(lib, H=H, W=W, variant=2, moments=0x1000)))
        assert need >= (2 * H * W // 256) * 64 * 4 * 4      # a slot of four sums per 256-row tile and channel
