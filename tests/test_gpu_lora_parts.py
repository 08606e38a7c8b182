"""-m gpu: vtgb_llm_lora_parts (ops.lora_update_parts) alone, bf16 -- the K-split reduce of a deferred vtgb_gemm_skinny projection and the
LoRA update in one launch.  The contract is bit equality with the two-launch form, ``lora_update(x, gemm_skinny(x, w, n_splits=S), segs)``,
for every row count, split count, rank and segment placement; columns outside every segment are the plain reduce; a row's bits do not
depend on the other rows; and one case is held to the rule of tests/lora_refs.py (fp64 reference, derived fp32 bound) applied to the reduced
base, so the equality does not rest on our own kernels alone.

Shapes: rows 1 / 7 / 8 / 9 / 128 (one row; the 8-row tile edge from both sides; the most the entry takes), K = 128 in 2 splits and K = 192 in
3, 288 columns with segments (0, 96) and (192, 96): 128-column fragment tiles end inside the first segment (at 128: in the gap) and inside the
second (at 256), and the last tile has 32 columns; ranks 1 / 8 / 9 / 64 (below the 8-rank pass, at it, just past it, the maximum)."""
import functools

import pytest
import torch

import lora_refs as R

pytestmark = pytest.mark.gpu

N_COLS, SEGMENTS, SCALING = 288, ((0, 96), (192, 96)), 4.0
ROWS, RANKS, SPLITS = (1, 7, 8, 9, 128), (1, 8, 9, 64), ((128, 2), (192, 3))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return "cuda:0"


def _bits(t):
    return t.contiguous().view(torch.int16)


@functools.lru_cache(maxsize=None)
def _case(dev, rows, K, r):
    """x [rows, K] (row stride K + 8), the projection's weight [288, K] and the two adapters, on the device."""
    x, _, segs = R.make_case(torch.bfloat16, K, r, rows, SCALING, seed=4, segments=SEGMENTS, n_cols=N_COLS)
    g = torch.Generator().manual_seed(9 * K + r + rows)
    w = (torch.randn(N_COLS, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    xd = torch.zeros(rows, x.stride(0), dtype=x.dtype, device=dev)[:, :K]
    xd.copy_(x)
    return xd, w.to(dev), [(c, A.to(dev), B.to(dev), s) for c, A, B, s in segs]


def _parts(x, w, S, segs, y=None):
    """The one-launch form over the fragments a deferred projection leaves; ``y`` starts as NaN: it is written, not read."""
    from videotgb_amd import ops
    out, S_got, part = ops.gemm_skinny(x, w, n_splits=S, defer_reduce=True)
    assert S_got == S and part is not None
    y = torch.full_like(out, float("nan")) if y is None else y
    got = ops.lora_update_parts(x, y, segs, part, S)
    assert got is y
    return y


@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("K,S", SPLITS)
def test_bit_equality_with_the_two_launch_form_and_the_plain_reduce(dev, K, S, r):
    from videotgb_amd import ops
    gap = torch.ones(N_COLS, dtype=torch.bool)
    for c0, n in SEGMENTS:
        gap[c0: c0 + n] = False
    for rows in ROWS:
        x, w, segs = _case(dev, rows, K, r)
        base = ops.gemm_skinny(x, w, n_splits=S)
        two = ops.lora_update(x, base.clone(), segs)
        one = _parts(x, w, S, segs)
        assert bool(torch.isfinite(one.float()).all()), rows
        assert torch.equal(_bits(one), _bits(two)), (rows, (_bits(one) != _bits(two)).nonzero()[:4].tolist())
        assert torch.equal(_bits(one[:, gap.to(dev)]), _bits(base[:, gap.to(dev)])), rows      # outside the segments: the reduce launch's bits
        assert not torch.equal(one[:, :96], base[:, :96]) and not torch.equal(one[:, 192:], base[:, 192:])      # (the adapters act)


@pytest.mark.parametrize("K,S,r", [(128, 2, 1), (192, 3, 8), (192, 3, 9), (128, 2, 64)])
def test_a_row_does_not_depend_on_the_batch(dev, K, S, r):
    """Rows of the 128-row and the 9-row call against the calls on each row alone (another fragment layout: the row count is part of it)."""
    for rows, picks in ((128, (0, 7, 8, 77, 127)), (9, (0, 8))):
        x, w, segs = _case(dev, rows, K, r)
        full = _parts(x, w, S, segs)
        for m in picks:
            one = _parts(x[m: m + 1], w, S, segs)
            assert torch.equal(_bits(one), _bits(full[m: m + 1])), (rows, m)


def test_y_with_a_row_stride_and_unsorted_segments(dev):
    """y as a column slice of a wider buffer (the padding keeps its bits); the segments handed over in descending column order."""
    from videotgb_amd import ops
    x, w, segs = _case(dev, 9, 192, 8)
    buf = torch.full((9, N_COLS + 8), 7.0, dtype=torch.bfloat16, device=dev)
    one = _parts(x, w, 3, segs[::-1], y=buf[:, :N_COLS])
    assert torch.equal(_bits(one), _bits(ops.lora_update(x, ops.gemm_skinny(x, w, n_splits=3), segs)))
    assert bool((buf[:, N_COLS:] == 7.0).all())


def test_one_case_obeys_the_rule_of_lora_refs(dev):
    """rows 9, K = 192 in 3 splits, r = 9: the update of the REDUCED base (the projection with its reduce launch) against the fp64 reference
    and the derived bound, columns outside the segments bit-identical to that base."""
    from videotgb_amd import ops
    x, w, segs = _case(dev, 9, 192, 9)
    base = ops.gemm_skinny(x, w, n_splits=3)
    got = _parts(x, w, 3, segs)
    why = R.verdict(x.cpu(), base.cpu(), [(c, A.cpu(), B.cpu(), s) for c, A, B, s in segs], got.cpu())
    assert why is None, why


def test_what_the_library_refuses_reaches_python(dev):
    """Every host-side rejection of the entry, through the wrapper (tests/test_lora_parts_abi.py has them at the C level without a device)."""
    from videotgb_amd import ops
    x, w, segs = _case(dev, 9, 192, 8)
    out, S, part = ops.gemm_skinny(x, w, n_splits=3, defer_reduce=True)
    for S_bad in (1, 0, 65):
        with pytest.raises(ValueError, match="n_splits"):
            ops.lora_update_parts(x, out, segs, torch.zeros(3 * 65 * 9 * 128, device=dev), S_bad)
    with pytest.raises(ValueError, match="VTGB_BF16"):
        ops.lora_update_parts(x.float(), out.float(), segs, part, S)
    big = torch.zeros(129, 192, dtype=torch.bfloat16, device=dev)
    with pytest.raises(ValueError, match="rows=129"):
        ops.lora_update_parts(big, torch.zeros(129, N_COLS, dtype=torch.bfloat16, device=dev), segs, torch.zeros(3 * 3 * 129 * 128, device=dev), 3)
    with pytest.raises(NotImplementedError, match="4-byte aligned"):
        ops.lora_update_parts(x, out, segs, torch.zeros(3 * 3 * 9 * 128 * 4 + 16, dtype=torch.uint8, device=dev)[2:], S)
    with pytest.raises(ValueError, match="overlap"):      # one of vtgb_llm_lora's own checks
        ops.lora_update_parts(x, out, [segs[0], (64, segs[1][1], segs[1][2], 4.0)], part, S)
    with pytest.raises(AssertionError, match="fragments"):      # too few fragments for (rows, n_cols, S): the wrapper's own check
        ops.lora_update_parts(x, out, segs, part.view(torch.uint8)[: 3 * 3 * 9 * 128 * 4 - 4], S)
