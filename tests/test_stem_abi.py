"""CPU-side checks of vtgb_raft_stem (the unit entry of the RAFT encoders' stem at bf16x3 / f16c8: variant 0 = pack + implicit GEMM, 1 = the fused
kernel, 2 = the fused kernel + the moments in the GEMM's order): declared in include/vtgb.h, exported by the built library and bound in _lib.py with a
struct of the declared layout; bad arguments are rejected on the host before any launch; the fused form refuses the sizes stem7x7_supported rejects
while the fallback takes them; the ABI version is unchanged."""
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


def test_error_codes_match_the_header():
    h = open(os.path.join(REPO, "include", "vtgb.h")).read()
    for name, val in (("VTGB_EINVAL", EINVAL), ("VTGB_EUNSUPPORTED", EUNSUPPORTED), ("VTGB_EWORKSPACE", EWORKSPACE)):
        assert re.search(rf"#define {name} \({val}\)", h), name


def test_symbols_are_declared_exported_and_bound(lib):
    h = open(os.path.join(REPO, "include", "vtgb.h")).read()
    assert re.search(r"\bint\s+vtgb_raft_stem\s*\(\s*const vtgb_raft_stem_args\* a, vtgb_stream_t stream\)", h)
    assert re.search(r"\bsize_t\s+vtgb_raft_stem_workspace_bytes\s*\(\s*const vtgb_raft_stem_args\* a\)", h)
    L = lib.lib()
    for name in ("vtgb_raft_stem", "vtgb_raft_stem_workspace_bytes"):
        assert name in lib.EXPORTS and getattr(L, name) is not None
    assert L.vtgb_raft_stem.restype is C.c_int and len(L.vtgb_raft_stem.argtypes) == 2
    assert L.vtgb_raft_stem_workspace_bytes.restype is C.c_size_t and len(L.vtgb_raft_stem_workspace_bytes.argtypes) == 1
    assert L.vtgb_version() == 601


def test_struct_matches_the_header(lib):
    h = open(os.path.join(REPO, "include", "vtgb.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} vtgb_raft_stem_args;", h).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [x.strip().split()[-1].lstrip("*") for x in decl.split(",")]
    assert names == [f[0] for f in lib.RaftStemArgs._fields_]
    assert C.sizeof(lib.RaftStemArgs) == 5 * 4 + 4 + 6 * 8 + 8      # five int32 (+ padding), five pointers + the workspace pointer, its size
    assert lib.RaftStemArgs.images.offset == 24 and lib.RaftStemArgs.workspace_bytes.offset == 72


def _args(lib, **kw):
    p = 0x1000      # never dereferenced: every call below ends on the host
    d = dict(n_images=2, H=64, W=64, variant=1, out_kind=F32, images=p, weights=p, bias=p, out=p, moments=p, workspace=0x10000, workspace_bytes=1 << 40)
    d.update(kw)
    return lib.RaftStemArgs(*[d[f[0]] for f in lib.RaftStemArgs._fields_])


def _call(lib, **kw):
    return lib.lib().vtgb_raft_stem(C.byref(_args(lib, **kw)), None)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("kw,word", [
    (dict(images=None), b"NULL"), (dict(weights=None), b"NULL"), (dict(bias=None), b"NULL"), (dict(out=None), b"NULL"), (dict(moments=None), b"NULL"),
    (dict(out_kind=PAIR_BF16, out=None), b"NULL"),
    (dict(images=0x1004), b"misaligned"), (dict(weights=0x1008), b"misaligned"), (dict(bias=0x1004), b"misaligned"), (dict(out=0x1008), b"misaligned"),
    (dict(moments=0x1004), b"misaligned"), (dict(workspace=0x10008), b"misaligned"), (dict(out_kind=PAIR_F16C8, out=0x1002), b"misaligned"),
    (dict(n_images=0), b"bad dims"), (dict(H=63), b"bad dims"), (dict(W=0), b"bad dims"), (dict(W=65), b"bad dims"), (dict(variant=3), b"bad dims"),
    (dict(variant=-1), b"bad dims"), (dict(out_kind=3), b"out_kind"), (dict(out_kind=-1), b"out_kind"),
])
def test_bad_arguments_are_rejected_on_the_host(lib, variant, kw, word):
    kw = dict(kw)
    kw.setdefault("variant", variant)
    assert _call(lib, **kw) == EINVAL
    assert word in lib.lib().vtgb_last_error()
    with pytest.raises(ValueError):
        lib.check(EINVAL)


@pytest.mark.parametrize("kw", [dict(out_kind=PAIR_BF16), dict(out_kind=PAIR_F16C8), dict(H=8, W=32), dict(H=30, W=32)])
def test_tile_order_moments_belong_to_fp32_rows_of_large_enough_images(lib, kw):
    assert _call(lib, variant=2, **kw) == EINVAL
    assert b"variant 2" in lib.lib().vtgb_last_error()
    assert _call(lib, variant=2, H=32, W=32, workspace_bytes=16) == EWORKSPACE      # 16 x 16 = 256 pixels: taken


def test_null_args_are_rejected(lib):
    assert lib.lib().vtgb_raft_stem(None, None) == EINVAL
    assert b"NULL" in lib.lib().vtgb_last_error()
    assert lib.lib().vtgb_raft_stem_workspace_bytes(None) == 0


def test_pair_rows_need_no_moments(lib):
    """moments belong to the fp32 rows: a pair call with moments == NULL passes every host check and stops at the (short) workspace."""
    assert _call(lib, out_kind=PAIR_BF16, moments=None, variant=0, workspace_bytes=16) == EWORKSPACE


# sizes the fused kernel does not take (stem7x7_supported: H, W even, 16 <= W / 2 <= 112, H / 2 >= 4) -- the fallback does
@pytest.mark.parametrize("H,W", [(64, 256), (64, 226), (64, 30), (6, 64), (2, 2)])
@pytest.mark.parametrize("out_kind", [F32, PAIR_BF16, PAIR_F16C8])
def test_fused_form_refuses_what_the_fallback_takes(lib, H, W, out_kind):
    L = lib.lib()
    assert _call(lib, H=H, W=W, variant=1, out_kind=out_kind) == EUNSUPPORTED
    assert b"fused stem" in L.vtgb_last_error()
    assert L.vtgb_raft_stem_workspace_bytes(C.byref(_args(lib, H=H, W=W, variant=1, out_kind=out_kind))) == 0
    # variant 0 accepts the shape: it sizes its workspace, and a call gets past every argument check to the workspace it was not given
    need = L.vtgb_raft_stem_workspace_bytes(C.byref(_args(lib, H=H, W=W, variant=0, out_kind=out_kind)))
    assert need >= 2 * (H // 2) * (W // 2) * 128 * 2      # at least the packed image: 256 B per half-resolution pixel
    assert _call(lib, H=H, W=W, variant=0, out_kind=out_kind, workspace_bytes=need - 256) == EWORKSPACE
    assert _call(lib, H=H, W=W, variant=0, out_kind=out_kind, workspace=None) == EWORKSPACE


@pytest.mark.parametrize("H,W", [(8, 32), (64, 64), (72, 104), (40, 224), (224, 224)])
def test_fused_form_takes_its_sizes_and_needs_no_packed_image(lib, H, W):
    L = lib.lib()
    n = 2
    fused = L.vtgb_raft_stem_workspace_bytes(C.byref(_args(lib, H=H, W=W, variant=1)))
    packed = L.vtgb_raft_stem_workspace_bytes(C.byref(_args(lib, H=H, W=W, variant=0)))
    assert 0 < fused and packed >= fused + n * (H // 2) * (W // 2) * 256 - 256
    assert _call(lib, H=H, W=W, variant=1, workspace_bytes=16) == EWORKSPACE
    # cnet's pair rows: the fused form needs neither the packed image nor the fp32 rows
    assert L.vtgb_raft_stem_workspace_bytes(C.byref(_args(lib, H=H, W=W, variant=1, out_kind=PAIR_F16C8))) <= 512
    assert L.vtgb_raft_stem_workspace_bytes(C.byref(_args(lib, H=H, W=W, variant=0, out_kind=PAIR_F16C8))) >= n * (H // 2) * (W // 2) * (256 + 256)
