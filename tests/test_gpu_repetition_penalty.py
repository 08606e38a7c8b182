"""-m gpu: vtgb_llm_repetition_penalty (ops.repetition_penalty) against the CPU statement of HF's RepetitionPenaltyLogitsProcessor, BIT FOR BIT.
The inputs are finite normal values, +-0 and +-inf, so the one fp32 multiply or divide per seen index is correctly rounded on both sides and
the results must be the same 32 bits.  Shapes: the smallest case; a vocabulary that crosses the 8192-index chunk by 7 and is odd (bf16 rows
start 2 bytes off); more ids than threads of a workgroup; a large vocabulary.  Planted in every case: duplicate ids, ids 0, V-1, 8191 and
8192, ids behind ``step`` that would change the result if read, ids outside [0, V), and negative, zero, positive and infinite logits on seen
ids."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1000, 7), (3, 8199, 40), (2, 32003, 300), (1, 128256, 64)]
START = 3      # the always-seen id of the "present" cases; its logit is negative


def STEPS(N):
    return (0, 1, N, N + 5, -1)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from videotgb_amd import _lib
    _lib.lib()
    return "cuda:0"


def _case(R, V, N, dtype):
    """(logits [R, V] ``dtype``, seq [R, N] int64) on the host with the planted ids and logits."""
    g = torch.Generator().manual_seed(R * 1000003 + V * 31 + N)
    logits = (torch.randn(R, V, generator=g) * 8.0).to(dtype)
    seq = torch.randint(0, V, (R, N), generator=g)
    a, b = (8191, 8192) if V > 8192 else (5, 6)      # the last index of the first chunk and the first of the second, where there are two
    seq[:, 0], seq[:, 1], seq[:, 2], seq[:, 3], seq[:, 4], seq[:, 5], seq[:, 6] = 0, V - 1, a, b, 7, 0, V      # (0 twice: a duplicate; V: outside)
    if N > 9:
        seq[:, 7], seq[:, 8], seq[:, 9] = -1, 2 ** 40, -(2 ** 40)      # outside [0, V) on both sides, beyond 32 bits too
        seq[:, N - 1] = seq[:, N - 2]                                   # one more duplicate, at the end
    logits[:, 0], logits[:, V - 1], logits[:, a], logits[:, b], logits[:, 7] = float("-inf"), 2.5, -0.0, 0.0, float("inf")
    logits[:, START] = -3.0
    return logits, seq


def _statement(logits, seq, step, p, start_id):
    """HF's rule on the host in fp32: x < 0 ? x * p : x / p at every index among seq[r, :clamp(step, 0, N)] or equal to start_id, once."""
    x = logits.float()
    R, V = x.shape
    n = min(max(int(step), 0), seq.shape[1])
    pt = torch.tensor(p, dtype=torch.float32)
    out = x.clone()
    for r in range(R):
        ids = {i for i in seq[r, :n].tolist() if 0 <= i < V}
        if start_id is not None and 0 <= start_id < V:
            ids.add(start_id)
        if ids:
            idx = torch.tensor(sorted(ids))
            gth = x[r, idx]
            out[r, idx] = torch.where(gth < 0, gth * pt, gth / pt)
    return out


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("R,V,N", SHAPES)
def test_the_kernel_equals_the_statement_bit_for_bit(dev, R, V, N, dtype):
    from videotgb_amd import ops
    logits, seq = _case(R, V, N, dtype)
    dl, ds = logits.to(dev), seq.to(dev)
    assert dl.data_ptr() % 16 == 0      # (rows past the first of an odd V start off a 16-byte boundary)
    out = torch.full((R, V), float("nan"), device=dev)      # the caller's buffer: every element is overwritten
    step_t = torch.zeros(1, dtype=torch.long, device=dev)
    # the planted ids behind the step matter: read, they would change the result
    full = _statement(logits, seq, N, 1.5, None)
    for step in (0, 1):
        assert not torch.equal(_bits(_statement(logits, seq, step, 1.5, None)), _bits(full))
    assert not torch.equal(_bits(_statement(logits, seq, N, 1.5, START)), _bits(full))      # ... and so does the start id
    for step in STEPS(N):
        step_t.fill_(step)
        for start_id in (None, -1, START):
            for p in (1.5, 0.5, 1.0):
                want = _statement(logits, seq, step, p, None if start_id == -1 else start_id)
                out.fill_(float("nan"))
                got = ops.repetition_penalty(dl, ds, step_t, p, start_id, out=out)
                assert got is out
                assert torch.equal(_bits(got), _bits(want)), (R, V, N, dtype, step, start_id, p, int((_bits(got) != _bits(want)).sum()))
                if p == 1.0:      # the identity: float(logit), bit for bit
                    assert torch.equal(_bits(got), _bits(logits.float()))
    # seen ids with negative, zero, positive and infinite logits, at the full step with the start id
    step_t.fill_(N)
    got = ops.repetition_penalty(dl, ds, step_t, 1.5, START, out=out).cpu()
    a, b = (8191, 8192) if V > 8192 else (5, 6)
    for r in range(R):
        assert got[r, 0] == float("-inf") and got[r, V - 1] == torch.tensor(2.5) / torch.tensor(1.5) and got[r, 7] == float("inf") and got[r, START] == -4.5
        assert _bits(got[r, a]).item() == -2 ** 31 and _bits(got[r, b]).item() == 0      # -0 stays -0, +0 stays +0
    # without ``out`` the wrapper allocates, with the same bits
    assert torch.equal(_bits(ops.repetition_penalty(dl, ds, step_t, 1.5, START)), _bits(got))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("R,V,N", [s for s in SHAPES if s[0] > 1])
def test_every_row_alone_equals_its_bits_in_the_batch(dev, R, V, N, dtype):
    """Elementwise: a row's result depends on the row alone, not on R, the grid or the row's place (alone, an odd-V bf16 row is aligned)."""
    from videotgb_amd import ops
    logits, seq = _case(R, V, N, dtype)
    dl, ds = logits.to(dev), seq.to(dev)
    for step in (N // 2, N):
        step_t = torch.full((1,), step, dtype=torch.long, device=dev)
        batch = ops.repetition_penalty(dl, ds, step_t, 1.5, START)
        assert torch.equal(_bits(batch), _bits(_statement(logits, seq, step, 1.5, START)))
        for r in range(R):
            alone = ops.repetition_penalty(dl[r:r + 1].clone(), ds[r:r + 1].clone(), step_t, 1.5, START)
            assert torch.equal(_bits(alone[0]), _bits(batch[r])), (R, V, N, dtype, step, r)


def test_the_call_is_capturable(dev):
    """With ``out`` given nothing is allocated: the call is captured, and a replay follows the device step."""
    from videotgb_amd import ops
    R, V, N = 3, 8199, 40
    logits, seq = _case(R, V, N, torch.bfloat16)
    dl, ds = logits.to(dev), seq.to(dev)
    out = torch.zeros(R, V, device=dev)
    step_t = torch.full((1,), 2, dtype=torch.long, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.repetition_penalty(dl, ds, step_t, 1.5, START, out=out)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.repetition_penalty(dl, ds, step_t, 1.5, START, out=out)
    for step in (2, N, 0):
        step_t.fill_(step)
        out.zero_()
        g.replay()
        assert torch.equal(_bits(out), _bits(_statement(logits, seq, step, 1.5, START))), step
