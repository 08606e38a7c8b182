"""-m gpu: ops.pick_greedy (vtgb_llm_pick_greedy) against its CPU statement -- torch.argmax on the CPU copy of the logits with the listed ids
at -inf while step < min_new, ``isin`` and ``where`` for the finished flag.  Every output is an integer or a boolean and must be EQUAL.

Shapes (B, V): (1, 1000), (5, 32003), (3, 128256): V that is no multiple of 256 or of 8, and an odd V whose bf16 rows do not start on 16
bytes (rows 1, 2, ... of V = 32003 start 2, 4, ... bytes off).  The logits are random integers in [-8, 8] / 4 -- exact in bf16, thousands of
exact ties per row, so the lowest-index rule decides every row -- with the cases' maxima planted on top."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1000), (5, 32003), (3, 128256)]
DTYPES = [torch.bfloat16, torch.float32]
N, SENTINEL, PAD = 7, -77, 31


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return "cuda:0"


@functools.lru_cache(maxsize=None)
def _logits(B, V, dtype):
    g = torch.Generator().manual_seed(B * 1000003 + V)
    return (torch.randint(-8, 9, (B, V), generator=g).float() / 4).to(dtype)


def statement(logits, step, eos, min_new, pad, fin, N):
    """The CPU statement: (tok [B], fin' [B], column) -- ``_GraphDecoder._pick``'s greedy branch with a set, on host tensors."""
    x = logits.clone()
    if step < min_new and len(eos):
        x[:, list(eos)] = float("-inf")
    nxt = x.argmax(-1)
    nxt = torch.where(fin, torch.full_like(nxt, pad), nxt)
    fin2 = fin | torch.isin(nxt, torch.tensor(list(eos), dtype=torch.long)) if len(eos) else fin.clone()
    return nxt, fin2, min(max(step, 0), N - 1)


def run(dev, logits, step, eos, min_new=0, pad=PAD, fin=None):
    """ops.pick_greedy on fresh buffers -> (tok, fin', out) on the host; checks them against the statement and that ``out`` is written in
    column ``step`` alone."""
    from videotgb_amd import ops
    B, V = logits.shape
    fin = torch.zeros(B, dtype=torch.bool) if fin is None else fin
    d_fin, d_tok = fin.to(dev), torch.full((B,), SENTINEL, dtype=torch.long, device=dev)
    d_out = torch.full((B, N), SENTINEL, dtype=torch.long, device=dev)
    ret = ops.pick_greedy(logits.to(dev), torch.tensor([step], device=dev), ops.eos_list(eos, V, dev), d_fin, d_tok, d_out, min_new, pad)
    assert ret is d_tok
    tok, fin2, col = statement(logits, step, eos, min_new, pad, fin, N)
    want_out = torch.full((B, N), SENTINEL, dtype=torch.long)
    want_out[:, col] = tok
    assert torch.equal(d_tok.cpu(), tok), (d_tok.cpu().tolist(), tok.tolist())
    assert torch.equal(d_fin.cpu(), fin2) and torch.equal(d_out.cpu(), want_out)
    return tok, fin2


def _plant(x, row, pairs, value=3.0):
    x = x.clone()
    for i in pairs:
        x[row, i] = value
    return x


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,V", SHAPES)
def test_ties_on_random_rows(dev, B, V, dtype):
    """No planting: the maximum 2.0 occurs ~ V / 17 times per row, the first occurrence wins; n_eos = 0 and a list that names no winner."""
    x = _logits(B, V, dtype)
    tok, fin = run(dev, x, 3, [])
    assert torch.equal(tok, (x == 2.0).int().argmax(-1)) and not fin.any()
    run(dev, x, 3, [V - 1] if (tok != V - 1).all() else [V - 2])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,V", SHAPES)
def test_the_maximum_planted_twice(dev, B, V, dtype):
    """(i, i + 256): the same thread on the element-wise path; (0, V - 1): the row's ends; neighbours: inside one 16-byte load or across two;
    others around the last whole vector.  The lower index wins."""
    base = _logits(B, V, dtype)
    tail = V - V % 8
    for lo, hi in ((5, 5 + 256), (0, V - 1), (V // 2, V // 2 + 1), (7, 8), (63, 64), (255, 256), (2047, 2048), (tail - 1, tail), (V - 2, V - 1), (V - 300, V - 1)):
        if hi >= V:      # (the pair does not exist at this V)
            continue
        for row in range(B):
            x = _plant(base, row, (lo, hi))
            tok, _ = run(dev, x, 0, [])
            assert tok[row] == lo, (lo, hi, row, int(tok[row]))
            x = _plant(base, row, (hi,))      # alone, the upper one is found as well
            assert run(dev, x, 0, [])[0][row] == hi


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,V", SHAPES)
def test_a_listed_id_holding_the_maximum(dev, B, V, dtype):
    base = _logits(B, V, dtype)
    min_new = 4
    for e, runner in ((V - 1, 11), (0, V - 2), (V // 3, V // 3 + 1)):
        x = base.clone()
        x[:, e], x[:, runner] = 5.0, 4.0
        other = next(i for i in (13, 14, 15) if i not in (e, runner))
        for eos in ([e], [other, e, e], [1, 2, 3, 4, 5, 6, 7, e]):      # n_eos 1, 3 with a duplicate, 8
            tok, fin = run(dev, x, min_new - 1, eos, min_new)      # blocked: the runner-up, fin stays clear
            assert (tok == runner).all() and not fin.any()
            tok, fin = run(dev, x, min_new, eos, min_new)          # free: picked, fin set
            assert (tok == e).all() and fin.all()
            tok, fin = run(dev, x, 0, eos, 0)                      # min_new 0 never blocks
            assert (tok == e).all() and fin.all()
    x = base.clone()      # two listed ids hold the two largest values: both are blocked, the third value wins
    x[:, 9], x[:, V - 9], x[:, 300] = 6.0, 5.0, 4.0
    tok, fin = run(dev, x, 0, [V - 9, 9, 17], 2)
    assert (tok == 300).all() and not fin.any()
    tok, fin = run(dev, x, 2, [V - 9, 9, 17], 2)
    assert (tok == 9).all() and fin.all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,V", [(5, 32003), (3, 128256)])
def test_finished_rows_emit_pad_and_keep_fin(dev, B, V, dtype):
    x = _logits(B, V, dtype).clone()
    x[:, 40] = 5.0
    fin = torch.zeros(B, dtype=torch.bool)
    fin[1] = True
    for eos in ([], [40], [3, 40, 40]):
        tok, fin2 = run(dev, x, 2, eos, 0, PAD, fin)
        assert tok[1] == PAD and fin2[1] and (tok[[0, 2]] == 40).all()
        assert bool(fin2[0]) == (40 in eos)
    tok, fin2 = run(dev, x, 2, [PAD], 0, PAD, fin)      # the pad a finished row emits is an id of the list: nothing changes for the others
    assert tok[1] == PAD and fin2.tolist() == fin.tolist()


def test_a_wrong_step_gives_a_wrong_column_never_a_write_outside(dev):
    x = _logits(5, 32003, torch.bfloat16)
    for step in (-3, N, N + 100, 2 ** 40):
        run(dev, x, step, [5])      # (``run`` compares the whole of ``out`` with the statement's clamped column)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_step_is_read_on_the_device_under_graph_replay(dev, dtype):
    from videotgb_amd import ops
    B, V = 5, 32003
    x = _logits(B, V, dtype).clone()
    e = 1234
    x[:, e], x[:, 77] = 5.0, 4.0
    min_new = 3
    d_x, step, eos = x.to(dev), torch.zeros(1, dtype=torch.long, device=dev), ops.eos_list([9, e], V, dev)
    fin, tok = torch.zeros(B, dtype=torch.bool, device=dev), torch.zeros(B, dtype=torch.long, device=dev)
    out = torch.full((B, N), SENTINEL, dtype=torch.long, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.pick_greedy(d_x, step, eos, fin, tok, out, min_new, PAD)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.pick_greedy(d_x, step, eos, fin, tok, out, min_new, PAD)
        step.add_(1)
    fin.zero_(), step.zero_(), out.fill_(SENTINEL)
    want = torch.full((B, N), SENTINEL, dtype=torch.long)
    for i in range(6):      # steps 0 .. 2 blocked (the runner-up), step 3 picks e and finishes, steps 4, 5 emit pad
        g.replay()
        t = 77 if i < min_new else e if i == min_new else PAD
        want[:, i] = t
        assert (tok.cpu() == t).all() and bool(fin.cpu().all()) == (i >= min_new), i
        assert torch.equal(out.cpu(), want), i
    step.fill_(5)      # the step changed on the device: the same graph writes that column, free of the block
    fin.zero_()
    g.replay()
    want[:, 5] = e
    assert torch.equal(out.cpu(), want) and int(step.item()) == 6 and bool(fin.cpu().all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_row_alone_and_inside_a_batch(dev, dtype):
    """The same row gives the same id alone and at every place of a batch of 5 (rows of V = 32003 start at five different offsets from a
    16-byte boundary in bf16)."""
    B, V = 5, 32003
    x = _logits(B, V, dtype)
    batch, _ = run(dev, x, 0, [3])
    for r in range(B):
        alone, _ = run(dev, x[r: r + 1].contiguous(), 0, [3])
        assert alone[0] == batch[r]
        moved = x.clone()
        moved[(r + 2) % B] = x[r]
        assert run(dev, moved, 0, [3])[0][(r + 2) % B] == batch[r]


def test_ops_asserts_its_operands(dev):
    from videotgb_amd import ops
    x = _logits(5, 32003, torch.bfloat16).to(dev)
    step, eos = torch.zeros(1, dtype=torch.long, device=dev), ops.eos_list([1], 32003, dev)
    fin, tok, out = torch.zeros(5, dtype=torch.bool, device=dev), torch.zeros(5, dtype=torch.long, device=dev), torch.zeros(5, N, dtype=torch.long, device=dev)
    with pytest.raises(AssertionError):
        ops.pick_greedy(x[:, :32000], step, eos, fin, tok, out)      # not contiguous
    with pytest.raises(AssertionError):
        ops.pick_greedy(x, step, eos.long(), fin, tok, out)
    with pytest.raises(AssertionError):
        ops.pick_greedy(x, step, eos, fin.to(torch.uint8), tok, out)
    with pytest.raises(AssertionError):
        ops.pick_greedy(x, step, eos, fin, tok[:4], out)
    with pytest.raises(ValueError):
        ops.eos_list([32003], 32003, dev)
    with pytest.raises(ValueError):
        ops.pick_greedy(x, step, torch.zeros(9, dtype=torch.int32, device=dev), fin, tok, out)      # 9 ids: the entry's refusal
