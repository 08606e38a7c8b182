"""-m gpu: the split-KV decode attention (ops.decode_attention(split=True), ops.decode_attention_fp8, ops.decode_attention_beam) reproduces,
bit for bit, what the three separate pass-1 kernels of 08a9d4e computed on an MI355X.

tests/golden/decode_attention_bits.json holds sha256 digests recorded there by tools/decode_attention_bits.py, which this test runs again:
per case the output and the workspace pass 1 leaves (allocated zeroed and exactly decode_attention_workspace_bytes, so m, l, O and their
layout are pinned).  The cases (tools/decode_attention_bits.py) sit where pass 1 takes another path: nq / nkv = 4 / 4, 8 / 2 and 12 / 1 (one
full and one partial block of query heads), hd 64 and 128, bf16 and fp32; a cache of 576 slots (three chunks, the last a single wave) at
pos 0, 63, 64, 255, 256, 300 and 575, unmasked and with leading pads, a whole chunk masked, a row without a visible key; the beam gather
with the generated keys on both sides of a 256-key boundary (its "pads" cases at n_prompt = 1 have no key to pad: they run the MASKED
kernels under an all-ones key_valid and must repeat the "plain" digests).  Every slot the contract calls unread holds NaN, which the recorder asserts
does not reach an output.  The fixture's "device" is the name the runtime gave the card it was recorded on, an MI355X (gfx950), which it
reports as "AMD Radeon Graphics".  If a kernel does not reproduce a digest, the kernel is wrong: the fixture is not re-recorded."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location("decode_attention_bits", os.path.join(REPO, "tools", "decode_attention_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def got():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return _recorder().digests(torch.device("cuda:0"))      # every case once, shared by the tests below


@pytest.fixture(scope="module")
def want():
    with open(os.path.join(REPO, "tests", "golden", "decode_attention_bits.json")) as f:
        return json.load(f)


def test_fixture_covers_the_cases(want):
    rec = _recorder()
    assert want["recorded_at"] == "08a9d4e"
    assert sorted(want["cases"]) == sorted(rec.case_names()) and len(set(rec.case_names())) == len(rec.case_names())
    assert all(sorted(d) == ["out", "ws"] for d in want["cases"].values())
    # the cases the kernel can go wrong at, by name
    names = set(want["cases"])
    for entry, dts in (("split", ("bf16", "f32")), ("fp8", ("bf16",)), ("beam", ("bf16", "f32"))):
        for dt in dts:
            for nq, nkv in ((4, 4), (8, 2), (12, 1)):
                for hd in (64, 128):
                    g = f"{entry}_{dt}_nq{nq}_nkv{nkv}_hd{hd}_"
                    if entry == "beam":
                        sub = {f"P{tp}_n{n}_s{s}_{m}" for tp, n, steps in ((64, 1, (0, 1, 63)), (256, 250, (0, 5, 6, 63)), (256, 256, (0, 1, 63)))
                               for s in steps for m in ("plain", "pads")}
                    else:
                        sub = {f"pos{p}_{m}" for p in (0, 63, 64, 255, 256, 300, 575) for m in ("plain", "pads")} | {"pos300_blind"}
                    assert {g + c for c in sub} <= names, g
    assert len(names) == 12 * 15 + 6 * 15 + 12 * 20


@pytest.mark.parametrize("group", _recorder().groups(), ids=lambda g: _recorder().group_name(*g))
def test_bits_equal_the_recorded_kernels(got, want, group):
    rec = _recorder()
    names = [f"{rec.group_name(*group)}_{c}" for c in rec.group_cases(group[0])]
    assert {n: got[n] for n in names} == {n: want["cases"][n] for n in names}
    if group[0] == "beam":      # n_prompt = 1 leaves no key to pad: the MASKED kernels under an all-ones key_valid give the unmasked kernels' bits
        for n in names:
            if "_n1_" in n and n.endswith("_pads"):
                assert got[n] == got[n[:-len("pads")] + "plain"], n
