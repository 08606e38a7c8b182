"""CPU-side checks of vtgb_raft_lookup_convc1 (the unit entry of RAFT's fused f16c8 lookup + convc1 launch): declared in include/vtgb.h, exported by
the built library and bound in _lib.py with a struct of the declared size; bad arguments are rejected on the host before any launch; the ABI version
is unchanged.  Also the condition on the inputs of tests/test_gpu_lookup_split.py that needs no GPU: they show the fp8 half of the arithmetic."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1      # include/vtgb.h


@pytest.fixture(scope="module")
def lib():
    from videotgb_amd import build
    build.build()
    from videotgb_amd import _lib
    return _lib


def test_symbol_is_declared_exported_and_bound(lib):
    h = open(os.path.join(REPO, "include", "vtgb.h")).read()
    assert re.search(r"\bint\s+vtgb_raft_lookup_convc1\s*\(\s*const vtgb_raft_lookup_convc1_args\* a, vtgb_stream_t stream\)", h)
    L = lib.lib()
    assert "vtgb_raft_lookup_convc1" in lib.EXPORTS and L.vtgb_raft_lookup_convc1 is not None
    assert L.vtgb_raft_lookup_convc1.restype is C.c_int and len(L.vtgb_raft_lookup_convc1.argtypes) == 2
    assert L.vtgb_version() == 601


def test_struct_matches_the_header(lib):
    h = open(os.path.join(REPO, "include", "vtgb.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} vtgb_raft_lookup_convc1_args;", h).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[\d+\]", "", x.strip().split()[-1].lstrip("*")) for x in decl.split(",")]
    assert names == [f[0] for f in lib.RaftLookupConvc1Args._fields_]
    assert C.sizeof(lib.RaftLookupConvc1Args) == 4 * 4 + 4 * 8 + 5 * 8 + 8      # four int32, corr[4], five pointers, the occupancy pointer
    assert lib.RaftLookupConvc1Args.corr.offset == 16 and lib.RaftLookupConvc1Args.occupancy.offset == 88


def _call(lib, **kw):
    p = 0x1000      # never dereferenced: every case below is rejected on the host
    d = dict(n_pairs=2, H8=9, W8=13, variant=1, corr=(p, p, p, p), flow=p, weights=p, scale=p, bias=p, out=p)
    d.update(kw)
    a = lib.RaftLookupConvc1Args(d["n_pairs"], d["H8"], d["W8"], d["variant"], (lib.vp * 4)(*d["corr"]), d["flow"], d["weights"], d["scale"], d["bias"],
                                 d["out"], None)
    return lib.lib().vtgb_raft_lookup_convc1(C.byref(a), None)


@pytest.mark.parametrize("kw,word", [
    (dict(flow=None), b"NULL"), (dict(weights=None), b"NULL"), (dict(scale=None), b"NULL"), (dict(bias=None), b"NULL"), (dict(out=None), b"NULL"),
    (dict(corr=(0x1000, 0x1000, None, 0x1000)), b"NULL"), (dict(n_pairs=0), b"bad dims"), (dict(H8=7), b"bad dims"), (dict(W8=0), b"bad dims"),
    (dict(variant=2), b"bad dims"), (dict(variant=-1), b"bad dims"),
])
def test_bad_arguments_are_rejected_on_the_host(lib, kw, word):
    assert _call(lib, **kw) == EINVAL
    assert word in lib.lib().vtgb_last_error()
    with pytest.raises(ValueError):
        lib.check(EINVAL)


def test_null_args_are_rejected(lib):
    assert lib.lib().vtgb_raft_lookup_convc1(None, None) == EINVAL
    assert b"NULL" in lib.lib().vtgb_last_error()


def test_gpu_test_inputs_show_the_fp8_half():
    """For the weight and pyramid scales of tests/lookup_ref.py the fp64 reference with both correction products dropped is far from the full one:
    >= 4 x 1.5 x 1.5 the error of the 14-bit output encoding alone (what both tiles' errors are dominated by; the last 1.5 is headroom for the fp32
    sums on top of it) -- measured 13-22 x.  The GPU test asserts the same against the whole-K tile's measured error."""
    import lookup_ref as R
    n, H8, W8 = R.SHAPES[0]
    for extremes in (False, True):
        pyr, w, b = R.make_inputs(n, H8, W8, extremes=extremes)
        for kind in ("uniform", "mix"):
            taps = R.taps_fp64(pyr, R.make_flow(kind, n, H8, W8), n, H8, W8)
            ref = R.c1_fp64(taps, w, b)
            d16, enc = R.rel_err(R.c1_fp64(taps, w, b, corrections=False), ref), R.rel_err(R.encode_decode(ref), ref)
            print(f"[lookup+convc1 inputs extremes={extremes} {kind}] fp16-only reference {d16:.3e}, output encoding {enc:.3e}: {d16 / enc:.1f} x")
            assert d16 >= 4 * 1.5 * 1.5 * enc
    # windows outside every level: nothing but the bias
    taps = R.taps_fp64(pyr, R.make_flow("outside", n, H8, W8), n, H8, W8)
    assert float(taps.abs().max()) == 0.0
