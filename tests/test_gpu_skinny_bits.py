"""-m gpu: ops.gemm_skinny reproduces, bit for bit, what the two kernels of 2f95aae (bf16 and fp8 weights) computed on an MI355X.

tests/golden/skinny_bits.json holds sha256 digests recorded there by tools/skinny_bits.py, which this test runs again: per case and weight form
(row-major bf16, SkinnyWeight, SkinnyWeightFp8) the fp32 output, the bf16 output and, where the case splits K, the fp32 fragments left under
defer_reduce=True.  The cases (tools/skinny_bits.py: CASES) sit where the kernel takes another path: one k-tile; M = 16 | 17 (x row blocks
1 | 2) with 10 k-tiles and N = 131 into a padded out of row pitch 136 (the unsplit epilogue's scalar tail store; the pad columns must keep their
prefill, which the recorder asserts); 17 k-tiles; uneven splits shorter than the weight ring; all 128 rows with splits of one k-tile; n_splits
above the k-tile count.  The fixture's "device" is the name the runtime gave the card it was recorded on, an MI355X (gfx950), which it
reports as "AMD Radeon Graphics"."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location("skinny_bits", os.path.join(REPO, "tools", "skinny_bits.py"))
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
    with open(os.path.join(REPO, "tests", "golden", "skinny_bits.json")) as f:
        return json.load(f)["cases"]


def test_fixture_covers_the_cases(want):
    rec = _recorder()
    assert sorted(want) == sorted(rec.case_name(*c) for c in rec.CASES)
    for name, forms in want.items():
        assert sorted(forms) == ["fp8", "rowmajor", "tiled"], name
        keys = {frozenset(d) for d in forms.values()}
        assert keys in ({frozenset(("f32", "bf16"))}, {frozenset(("f32", "bf16", "parts"))}), name
    split = {n for n, forms in want.items() if "parts" in forms["tiled"]}
    assert split == {"M33_N384_K1088_S0", "M65_N200_K1088_S3", "M128_N256_K128_S2", "M5_N100_K128_S5"}


@pytest.mark.parametrize("case", _recorder().CASES)
def test_skinny_bits_equal_the_recorded_kernels(got, want, case):
    name = _recorder().case_name(*case)
    assert got[name] == want[name]
    assert got[name]["rowmajor"] == got[name]["tiled"]      # the tiled bf16 layout: same products, same order
