"""CPU-side checks of vtgb_raft_gru_half (the unit entry of the SepConvGRU gate launches of RAFT's refinement loop at f16c8 / bf16x3): declared in
include/vtgb.h, exported by the built library and bound in _lib.py with a struct of the declared size; bad arguments are rejected on the host before any
launch; the ABI version is unchanged; the refinement loop and the entry reach the launches through one helper.  Also the condition on the inputs of
tests/test_gpu_gru_half.py that needs no GPU: a single dropped correction product is far outside the bounds that test holds the device to."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1      # include/vtgb.h
F16C8, BF16X3 = 3, 2


@pytest.fixture(scope="module")
def lib():
    from videotgb_amd import build
    build.build()
    from videotgb_amd import _lib
    return _lib


def test_symbol_is_declared_exported_and_bound(lib):
    h = open(os.path.join(REPO, "include", "vtgb.h")).read()
    assert re.search(r"\bint\s+vtgb_raft_gru_half\s*\(\s*const vtgb_raft_gru_half_args\* a, vtgb_stream_t stream\)", h)
    L = lib.lib()
    assert "vtgb_raft_gru_half" in lib.EXPORTS and L.vtgb_raft_gru_half is not None
    assert L.vtgb_raft_gru_half.restype is C.c_int and len(L.vtgb_raft_gru_half.argtypes) == 2
    assert L.vtgb_version() == 601
    assert (lib.F16C8, lib.BF16X3) == (F16C8, BF16X3)


def test_struct_matches_the_header(lib):
    h = open(os.path.join(REPO, "include", "vtgb.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} vtgb_raft_gru_half_args;", h).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [x.strip().split()[-1].lstrip("*") for x in decl.split(",")]
    assert names == [f[0] for f in lib.RaftGruHalfArgs._fields_]
    assert C.sizeof(lib.RaftGruHalfArgs) == 6 * 4 + 11 * 8      # six int32, eleven pointers
    assert lib.RaftGruHalfArgs.h.offset == 24 and lib.RaftGruHalfArgs.scale_q.offset == 104


def test_the_loop_and_the_entry_share_one_helper():
    src = open(os.path.join(REPO, "videotgb_amd", "csrc", "raft_x3.hip")).read()
    assert len(re.findall(r"VTGB_EPI_X3ZR", src)) == 1 and len(re.findall(r"VTGB_EPI_X3Q", src)) == 1      # built in x3_gru_half only
    body = lambda name: src[src.index(name):].split("\n}\n")[0]
    assert "x3_gru_half(g, 2, s)" in body("int raft_x3_impl(")
    assert "x3_gru_half(g, a->stage" in body('extern "C" int vtgb_raft_gru_half(')


PTRS = ("h", "h_q", "x", "rh", "z", "start_zr", "start_q", "w_zr", "w_q", "scale_zr", "scale_q")


def _call(lib, **kw):
    p = 0x1000      # never dereferenced: every case below is rejected on the host
    d = dict(fmt=F16C8, n_images=2, H8=9, W8=13, half=0, stage=2, **{k: p for k in PTRS})
    d.update(kw)
    a = lib.RaftGruHalfArgs(*[d[f[0]] for f in lib.RaftGruHalfArgs._fields_])
    return lib.lib().vtgb_raft_gru_half(C.byref(a), None)


@pytest.mark.parametrize("kw,word", [(dict(fmt=f, **{k: None}), b"scale" if k.startswith("scale") else b"NULL") for f in (F16C8, BF16X3) for k in PTRS
                                     if not (f == BF16X3 and k.startswith("scale"))] + [
    (dict(stage=0, h=None), b"NULL"), (dict(stage=0, start_zr=None), b"NULL"), (dict(stage=0, w_zr=None), b"NULL"), (dict(stage=0, scale_zr=None), b"scale"),
    (dict(stage=1, h_q=None), b"NULL"), (dict(stage=1, start_q=None), b"NULL"), (dict(stage=1, w_q=None), b"NULL"), (dict(stage=1, scale_q=None), b"scale"),
    (dict(stage=0, z=None), b"NULL"), (dict(stage=1, rh=None), b"NULL"), (dict(stage=1, x=None), b"NULL"),
    (dict(fmt=0), b"bad fmt"), (dict(fmt=1), b"bad fmt"), (dict(fmt=4), b"bad fmt"), (dict(half=2), b"bad half"), (dict(half=-1), b"bad half"),
    (dict(stage=3), b"stage"), (dict(stage=-1), b"stage"), (dict(n_images=0), b"bad dims"), (dict(H8=7), b"bad dims"), (dict(W8=0), b"bad dims"),
    (dict(n_images=-3), b"bad dims"),
])
def test_bad_arguments_are_rejected_on_the_host(lib, kw, word):
    assert _call(lib, **kw) == EINVAL
    assert word in lib.lib().vtgb_last_error()
    with pytest.raises(ValueError):
        lib.check(EINVAL)


def test_null_args_are_rejected(lib):
    assert lib.lib().vtgb_raft_gru_half(None, None) == EINVAL
    assert b"NULL" in lib.lib().vtgb_last_error()


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("fmt", ["f16c8", "bf16x3"])
def test_gpu_test_inputs_show_every_correction_product(fmt, half):
    """On the inputs of tests/test_gpu_gru_half.py at (2, 9, 13) the fp64 reference with ONE correction product dropped (f16c8: xl' . Wh8 or xh8 . Wl';
    bf16x3: lo . Wh or hi . Wl) violates the bound that test asserts -- z in the z | r launch, h' in the q launch -- at some element by >= 4 x.  The q
    launch reads the reference's own z (as fp32) and r h (as a pair row) here."""
    import gru_ref as R
    f = R.FMT[fmt]
    shape = R.SHAPES[0]
    d = R.make_inputs(*shape, half)
    s0 = R.stage0(f, d, shape, half)
    e0 = R.e_f32(f, s0["h_rows"], s0["x_rows"], d["w_zr"], d["start_zr"], shape, half, s0["pre"])
    rh_rows, z32 = R.pack_pair(s0["rh"], f), s0["z"].float()
    s1 = R.stage1(f, d, shape, half, rh_rows, z32, s0["h_rows"], s0["x_rows"])
    e1 = R.e_f32(f, rh_rows, s0["x_rows"], d["w_q"], d["start_q"], shape, half, s1["pre"])
    print(f"[gru half {fmt} half={half}] pre-activation scale {float(s0['pre'].abs().max()):.1f} / {float(s1['pre'].abs().max()):.1f}, "
          f"e_f32 = {e0:.2e} / {e1:.2e}, z bound {R.bound_z(e0):.2e}")
    assert 0.0 < e0 < 1e-4 and 0.0 < e1 < 1e-4
    for drop in R.DROPS[f]:
        t0 = R.stage0(f, d, shape, half, drop=drop)
        t1 = R.stage1(f, d, shape, half, rh_rows, z32, s0["h_rows"], s0["x_rows"], drop=drop)
        vz = float(((t0["z"] - s0["z"]).abs() / R.bound_z(e0)).max())
        vh = float(((t1["h_new"] - s1["h_new"]).abs() / R.bound_h(e1, s1["z"], s1["hval"], s1["h_new"], f)).max())
        print(f"    without {drop}: pre moves by {float((t0['pre'] - s0['pre']).abs().max()):.2e} / {float((t1['pre'] - s1['pre']).abs().max()):.2e}; "
              f"z is {vz:.0f} x its bound away, h' {vh:.0f} x")
        assert vz >= 4.0 and vh >= 4.0
