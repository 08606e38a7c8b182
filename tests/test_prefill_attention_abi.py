"""CPU-side checks of vtgb_attention_tiled (the prefill's tiled attention): declared in include/vtgb.h, exported by the built
library, bound in _lib.py with the header's struct layout, bad arguments rejected on the host before any launch; the ABI version is
unchanged."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -4      # include/vtgb.h


@pytest.fixture(scope="module")
def lib():
    from videotgb_amd import build
    build.build()
    from videotgb_amd import _lib
    return _lib


def _header():
    return open(os.path.join(REPO, "include", "vtgb.h")).read()


def test_symbol_is_declared_exported_and_bound(lib):
    assert re.search(r"\bint\s+vtgb_attention_tiled\s*\(\s*const\s+vtgb_attention_tiled_args\s*\*", _header())
    assert "vtgb_attention_tiled" in lib.EXPORTS
    L = lib.lib()
    fn = L.vtgb_attention_tiled
    assert fn.restype is C.c_int and fn.argtypes[0] is C.POINTER(lib.AttentionTiledArgs)
    assert L.vtgb_version() == 601


def test_struct_layout_follows_the_header(lib):
    body = re.search(r"typedef struct \{([^}]*)\}\s*vtgb_attention_tiled_args;", _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    kinds = {"int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        if "*" in decl:
            fields.append((decl.split("*")[-1].strip(), C.c_void_p))
            continue
        ctype, names = decl.split(None, 1)
        fields += [(n.strip(), kinds[ctype]) for n in names.split(",")]
    assert [(n, t) for n, t in lib.AttentionTiledArgs._fields_] == fields
    assert C.sizeof(lib.AttentionTiledArgs) == 6 * 4 + 3 * 8 + 4 * 8 + 8 + 4 + 4 + 8 + 2 * 8


def _args(lib, **kw):
    p = 0x1000      # never dereferenced: every case below is rejected on the host
    d = dict(batch=1, heads=4, kv_heads=2, head_dim=128, s_q=320, s_kv=320, q=p, k=p, v=p, q_tok_stride=512, kv_tok_stride=256,
             q_batch_stride=320 * 512, kv_batch_stride=320 * 256, key_mask=None, scale=0.088, causal=1, out=p, out_tok_stride=512,
             out_batch_stride=320 * 512)
    d.update(kw)
    return lib.AttentionTiledArgs(**d)


@pytest.mark.parametrize("kw,code,word", [
    (dict(q=None), EINVAL, b"NULL"), (dict(k=None), EINVAL, b"NULL"), (dict(v=None), EINVAL, b"NULL"), (dict(out=None), EINVAL, b"NULL"),
    (dict(heads=4, kv_heads=3), EINVAL, b"kv_heads"), (dict(kv_heads=0), EINVAL, b"empty"), (dict(s_q=0), EINVAL, b"empty"),
    (dict(head_dim=96), EUNSUPPORTED, b"head_dim"), (dict(head_dim=256), EUNSUPPORTED, b"head_dim"), (dict(head_dim=32), EUNSUPPORTED, b"head_dim"),
    (dict(s_kv=4097), EUNSUPPORTED, b"4096"), (dict(kv_tok_stride=252), EUNSUPPORTED, b"alignment"),
    (dict(q=0x1008), EUNSUPPORTED, b"alignment"), (dict(v=0x1002), EUNSUPPORTED, b"alignment"), (dict(out=0x1004), EUNSUPPORTED, b"alignment"),
    (dict(key_mask=0x1002), EUNSUPPORTED, b"alignment"),
])
def test_bad_arguments_are_rejected_on_the_host(lib, kw, code, word):
    L = lib.lib()
    assert L.vtgb_attention_tiled(C.byref(_args(lib, **kw)), None) == code
    assert word in L.vtgb_last_error()
    with pytest.raises(ValueError if code == EINVAL else NotImplementedError):
        lib.check(code)


def test_null_args_pointer(lib):
    L = lib.lib()
    assert L.vtgb_attention_tiled(None, None) == EINVAL and b"NULL" in L.vtgb_last_error()
