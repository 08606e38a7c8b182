"""CPU-side checks of vtgb_conv_launch (the unit entry of RAFT's implicit-GEMM convolution launches at bf16x3 / bf16 / fp32): declared in include/vtgb.h,
exported by the built library and bound in _lib.py with a struct of the declared layout; bad arguments are rejected on the host before any launch, with a
message; the ABI version is unchanged; the production callers and the entry build their descriptors with the same helpers (csrc/conv_descs.h)."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1      # include/vtgb.h
F32, BF16, BF16X3, F16C8 = 0, 1, 2, 3
OUT_F32, OUT_PAIR_BF16, OUT_PAIR_F16C8, OUT_BF16 = 0, 1, 2, 3


@pytest.fixture(scope="module")
def lib():
    from videotgb_amd import build
    build.build()
    from videotgb_amd import _lib
    return _lib


def test_symbol_is_declared_exported_and_bound(lib):
    h = open(os.path.join(REPO, "include", "vtgb.h")).read()
    assert re.search(r"\bint\s+vtgb_conv_launch\s*\(\s*const vtgb_conv_launch_args\* a, vtgb_stream_t stream\)", h)
    L = lib.lib()
    assert "vtgb_conv_launch" in lib.EXPORTS and L.vtgb_conv_launch is not None
    assert L.vtgb_conv_launch.restype is C.c_int and len(L.vtgb_conv_launch.argtypes) == 2
    assert L.vtgb_version() == 601
    for name, val in (("F32", OUT_F32), ("PAIR_BF16", OUT_PAIR_BF16), ("PAIR_F16C8", OUT_PAIR_F16C8), ("BF16", OUT_BF16)):
        assert re.search(rf"#define VTGB_CONV_OUT_{name} {val}\b", h) and getattr(lib, "CONV_OUT_" + name) == val
    assert (lib.CONV_SITE_ENCODER, lib.CONV_SITE_UPDATE) == (0, 1)


def test_struct_matches_the_header(lib):
    h = open(os.path.join(REPO, "include", "vtgb.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} vtgb_conv_launch_args;", h).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names, kinds = [], []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype = "ptr" if "*" in decl else decl.split()[0]
            for x in decl.split(","):
                names.append(x.strip().split()[-1].lstrip("*"))
                kinds.append(ctype)
    fields = lib.ConvLaunchArgs._fields_
    assert names == [f[0] for f in fields]
    want = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "ptr": C.c_void_p}
    assert [want[k] for k in kinds] == [f[1] for f in fields]
    assert C.sizeof(lib.ConvLaunchArgs) == 16 * 4 + 4 + 4 + 13 * 8      # sixteen int32, one float (+ 4 bytes of padding), thirteen 8-byte members
    assert lib.ConvLaunchArgs.out_scale.offset == 64 and lib.ConvLaunchArgs.a.offset == 72 and lib.ConvLaunchArgs.tail_out.offset == 168


def test_the_callers_and_the_entry_share_the_descriptor_builders():
    src = {f: open(os.path.join(REPO, "videotgb_amd", "csrc", f)).read() for f in ("raft.hip", "raft_enc.hip", "raft_x3.hip", "conv_descs.h")}
    for fn in ("conv_desc", "enc_conv", "enc_stem_conv", "x3_conv"):
        assert len(re.findall(rf"static inline GemmDesc {fn}\(", src["conv_descs.h"])) == 1
        assert not any(re.search(rf"GemmDesc {fn}\(int", src[f]) for f in ("raft.hip", "raft_enc.hip", "raft_x3.hip"))      # defined once, in the header
    entry = src["raft_x3.hip"][src["raft_x3.hip"].index('extern "C" int vtgb_conv_launch('):]
    for fn in ("conv_desc(", "enc_conv(", "enc_stem_conv(", "x3_conv(", "launch_conv_gemm(d, s)", "launch_stats_finish_tiles(d.col_stats"):
        assert fn in entry
    assert "memset(&d" not in entry                                      # no descriptor of its own
    assert "conv_desc(" in src["raft.hip"] and "enc_stem_conv(" in src["raft_enc.hip"] and "enc_conv(" in src["raft_enc.hip"]


PTRS = ("a", "weights", "out")


def _call(lib, **kw):
    p = 0x1000      # never dereferenced: every case below is rejected on the host
    d = dict(dtype=BF16X3, out_kind=OUT_F32, site=1, n_images=2, H=9, W=13, KH=3, KW=3, stride=1, Hi=0, Wi=0, C1=128, C2=0, N=64, act=0, post_relu=0,
             out_scale=0.0, a=p, a2=None, weights=p, bias=p, out=p, ld_out=64, moments=None, stats_part=None, stats_part_floats=0, resid=None, ld_resid=0,
             tail_w=None, tail_out=None)
    d.update(kw)
    a = lib.ConvLaunchArgs(*[d[f[0]] for f in lib.ConvLaunchArgs._fields_])
    return lib.lib().vtgb_conv_launch(C.byref(a), None)


MOM = dict(site=0, H=20, W=14, moments=0x1000, stats_part=0x1000, stats_part_floats=(2 * 280 // 256 + 2) * 512)

CASES = [(dict(**{k: None}), b"NULL operand") for k in PTRS] + [
    (dict(C2=128), b"NULL operand"), (dict(a2=0x1000), b"NULL operand"),                                   # a2 and C2 come together
    (dict(dtype=F16C8), b"bad dtype"), (dict(dtype=-1), b"bad dtype"), (dict(dtype=4), b"bad dtype"),
    (dict(out_kind=4), b"bad out_kind"), (dict(out_kind=-1), b"bad out_kind"),
    (dict(site=2), b"bad site"), (dict(act=3), b"bad site"), (dict(stride=3), b"bad site"), (dict(stride=0), b"bad site"),
    (dict(C1=96), b"multiples of 64"), (dict(C1=32), b"multiples of 64"), (dict(C2=32, a2=0x1000), b"multiples of 64"),
    (dict(n_images=0), b"bad dims"), (dict(H=0), b"bad dims"), (dict(W=-1), b"bad dims"), (dict(KH=0), b"bad dims"), (dict(N=0), b"bad dims"), (dict(C1=0), b"bad dims"),
    (dict(ld_out=60), b"ld_out"),
    (dict(dtype=BF16, out_kind=OUT_PAIR_BF16), b"pair rows"), (dict(dtype=F32, out_kind=OUT_PAIR_F16C8), b"pair rows"),
    (dict(dtype=BF16X3, out_kind=OUT_BF16), b"bf16 rows"), (dict(dtype=F32, out_kind=OUT_BF16), b"bf16 rows"),
    (dict(resid=0x1000, ld_resid=64), b"belong to VTGB_CONV_OUT_BF16"), (dict(tail_w=0x1000, tail_out=0x1000), b"belong to VTGB_CONV_OUT_BF16"),
    (dict(dtype=BF16, out_kind=OUT_BF16, tail_w=0x1000), b"tail_out"), (dict(dtype=BF16, out_kind=OUT_BF16, resid=0x1000, ld_resid=8), b"ld_resid"),
    (dict(dtype=BF16, out_kind=OUT_BF16, post_relu=1), b"post_relu"),
    (dict(out_scale=0.25), b"out_scale"), (dict(dtype=BF16, KH=3, KW=3, out_scale=0.25), b"out_scale"),
    (dict(site=0, KH=1, KW=5), b"encoder site"), (dict(site=0, C2=128, a2=0x1000), b"encoder site"), (dict(site=0, KH=4, KW=1, stride=2), b"encoder site"),
    (dict(site=1, stride=2, Hi=18, Wi=26), b"update-block site"), (dict(site=1, Hi=18, Wi=26), b"update-block site"),
    (dict(MOM, H=9, W=13), b">= 256 rows"), (dict(MOM, H=15, W=17), b">= 256 rows"),
    (dict(MOM, out_kind=OUT_PAIR_BF16), b"fp32 rows"), (dict(MOM, dtype=BF16, out_kind=OUT_BF16), b"fp32 rows"),
    (dict(MOM, site=1), b"encoder site"), (dict(MOM, N=256, ld_out=256), b"encoder site"), (dict(MOM, act=1), b"encoder site"),
    (dict(MOM, stats_part=None), b"stats_part"), (dict(MOM, stats_part_floats=MOM["stats_part_floats"] - 1), b"stats_part"),
]


@pytest.mark.parametrize("kw,word", CASES)
def test_bad_arguments_are_rejected_on_the_host(lib, kw, word):
    assert _call(lib, **kw) == EINVAL
    assert word in lib.lib().vtgb_last_error(), lib.lib().vtgb_last_error()
    with pytest.raises(ValueError):
        lib.check(EINVAL)


def test_null_args_are_rejected(lib):
    assert lib.lib().vtgb_conv_launch(None, None) == EINVAL
    assert b"NULL args" in lib.lib().vtgb_last_error()
