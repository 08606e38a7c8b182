"""CPU-side checks of vtgb_attention_cached (the chunked prefill's attention over the KV cache): declared in include/vtgb.h, exported by
the built library, bound in _lib.py with the header's struct layout, bad arguments rejected on the host before any launch; the ABI
version is unchanged.  And the chunk plan of the chunked prefill (decode.prefill_chunks), a pure function."""
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
    assert re.search(r"\bint\s+vtgb_attention_cached\s*\(\s*const\s+vtgb_attention_cached_args\s*\*", _header())
    assert "vtgb_attention_cached" in lib.EXPORTS
    L = lib.lib()
    fn = L.vtgb_attention_cached
    assert fn.restype is C.c_int and fn.argtypes[0] is C.POINTER(lib.AttentionCachedArgs)
    assert L.vtgb_version() == 601
    from videotgb_amd import build
    assert "attn_cached.hip" in build.SOURCES


def test_struct_layout_follows_the_header(lib):
    body = re.search(r"typedef struct \{([^}]*)\}\s*vtgb_attention_cached_args;", _header()).group(1)
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
    assert [(n, t) for n, t in lib.AttentionCachedArgs._fields_] == fields
    # 7 int32 + scale, q / kc / vc / ks / vs / key_valid, 2 q strides, out, 2 out strides: no padding
    assert C.sizeof(lib.AttentionCachedArgs) == 8 * 4 + 6 * 8 + 2 * 8 + 8 + 2 * 8


def _args(lib, **kw):
    p = 0x1000      # never dereferenced: every case below is rejected on the host
    d = dict(batch=1, heads=4, kv_heads=2, head_dim=128, s_q=128, q0=256, tmax=448, scale=0.088, q=p, kc=p, vc=p, ks=None, vs=None,
             key_valid=None, q_tok_stride=1024, q_batch_stride=128 * 1024, out=p, out_tok_stride=512, out_batch_stride=128 * 512)
    d.update(kw)
    return lib.AttentionCachedArgs(**d)


@pytest.mark.parametrize("kw,code,word", [
    (dict(q=None), EINVAL, b"NULL"), (dict(kc=None), EINVAL, b"NULL"), (dict(vc=None), EINVAL, b"NULL"), (dict(out=None), EINVAL, b"NULL"),
    (dict(batch=0), EINVAL, b"empty"), (dict(heads=0), EINVAL, b"empty"), (dict(kv_heads=0), EINVAL, b"empty"), (dict(s_q=0), EINVAL, b"empty"),
    (dict(s_q=-3), EINVAL, b"empty"), (dict(tmax=0), EINVAL, b"empty"), (dict(q0=-1), EINVAL, b"q0"),
    (dict(heads=4, kv_heads=3), EINVAL, b"kv_heads"),
    (dict(ks=0x2000), EINVAL, b"ks and vs"), (dict(vs=0x2000), EINVAL, b"ks and vs"),
    (dict(head_dim=96), EUNSUPPORTED, b"head_dim"), (dict(head_dim=256), EUNSUPPORTED, b"head_dim"), (dict(head_dim=32), EUNSUPPORTED, b"head_dim"),
    (dict(q0=321), EUNSUPPORTED, b"exceed the cache"), (dict(q0=0, s_q=449), EUNSUPPORTED, b"exceed the cache"),
    (dict(q0=2**31 - 64, s_q=128), EUNSUPPORTED, b"exceed the cache"),
    (dict(tmax=16385), EUNSUPPORTED, b"16384"), (dict(tmax=16448, q0=16000), EUNSUPPORTED, b"16384"),
    (dict(batch=65536), EUNSUPPORTED, b"grid"), (dict(heads=65536 * 2, kv_heads=2), EUNSUPPORTED, b"grid"),
    (dict(q_tok_stride=1020), EUNSUPPORTED, b"alignment"), (dict(q_batch_stride=1028), EUNSUPPORTED, b"alignment"),
    (dict(out_tok_stride=510), EUNSUPPORTED, b"alignment"), (dict(out_batch_stride=2), EUNSUPPORTED, b"alignment"),
    (dict(q=0x1008), EUNSUPPORTED, b"alignment"), (dict(kc=0x1008), EUNSUPPORTED, b"alignment"), (dict(vc=0x1002), EUNSUPPORTED, b"alignment"),
    (dict(out=0x1004), EUNSUPPORTED, b"alignment"), (dict(ks=0x2002, vs=0x2000), EUNSUPPORTED, b"alignment"),
    (dict(ks=0x2000, vs=0x2001), EUNSUPPORTED, b"alignment"),
])
def test_bad_arguments_are_rejected_on_the_host(lib, kw, code, word):
    L = lib.lib()
    assert L.vtgb_attention_cached(C.byref(_args(lib, **kw)), None) == code
    assert word in L.vtgb_last_error()
    with pytest.raises(ValueError if code == EINVAL else NotImplementedError):
        lib.check(code)


def test_null_args_pointer(lib):
    L = lib.lib()
    assert L.vtgb_attention_cached(None, None) == EINVAL and b"NULL" in L.vtgb_last_error()


@pytest.mark.parametrize("P,chunk,plan", [
    (2049, 2048, [(0, 2048), (2048, 1)]),
    (4096, 2048, [(0, 2048), (2048, 2048)]),
    (4097, 2048, [(0, 2048), (2048, 2048), (4096, 1)]),
    (16000, 2048, [(2048 * i, 2048) for i in range(7)] + [(14336, 1664)]),
    (300, 128, [(0, 128), (128, 128), (256, 44)]),
    (128, 128, [(0, 128)]),
    (5, 2048, [(0, 5)]),
])
def test_prefill_chunks(P, chunk, plan):
    from videotgb_amd.decode import GreedyDecoder, prefill_chunks
    got = prefill_chunks(P, chunk)
    assert got == plan
    assert sum(n for _, n in got) == P and all(0 < n <= chunk for _, n in got)
    assert all(a[0] + a[1] == b[0] for a, b in zip(got, got[1:])) and got[0][0] == 0      # consecutive, from row 0
    assert GreedyDecoder.PREFILL_CHUNK_TOKENS == 2048 and GreedyDecoder.PREFILL_MAX_TOKENS == 2048


def test_prefill_chunks_rejects_empty_plans():
    from videotgb_amd.decode import prefill_chunks
    with pytest.raises(ValueError):
        prefill_chunks(0, 128)
    with pytest.raises(ValueError):
        prefill_chunks(300, 0)
