"""References for the beam-search step (no GPU, no libvtgb): the candidate rule of ops.beam_candidates / vtgb_llm_beam_candidates in fp64 (and,
at fp32, as the literal torch statement of what transformers' ``_beam_search`` computes), the gather that materialises the cache
ops.decode_attention_beam reads, and the inputs of the GPU candidate test -- generated here so that their properties (the gap between
consecutive reference candidates) are asserted on the CPU as well."""
import functools

import torch

GAP = 1e-3      # the least gap between consecutive reference candidates among the first 2K + 1 of every generated case


def candidates_ref(logits, seq, step, running, penalty=1.0, eos=None, min_new=0, dtype=torch.float64, n=None):
    """logits [B*K, V], seq [B*K, N] int64 (the first ``step`` ids count), running [B, K] -> (score [B, n], idx [B, n] int64 = k * V + token),
    n = 2K by default: per row lp = log_softmax(logits) in ``dtype``; every distinct id of seq[r, :step] once: lp < 0 ? lp * p : lp / p;
    lp[eos] = -inf while step < min_new; + running; per batch item the n largest of the K * V values, descending, equal values in ascending
    index (a stable sort)."""
    B, K = running.shape
    R, V = logits.shape
    lp = torch.log_softmax(logits.detach().cpu().to(dtype), dim=-1)
    seq = seq.detach().cpu()
    p = torch.tensor(penalty, dtype=torch.float32).to(dtype)      # (the kernel's and HF's penalty is an fp32 number)
    for r in range(R):
        ids = torch.unique(seq[r, :step])
        ids = ids[(ids >= 0) & (ids < V)]
        v = lp[r, ids]
        lp[r, ids] = torch.where(v < 0, v * p, v / p)
    if eos is not None and step < min_new:
        lp[:, eos] = float("-inf")
    s = (lp.view(B, K, V) + running.detach().cpu().to(dtype)[:, :, None]).reshape(B, K * V)
    score, idx = torch.sort(s, dim=-1, descending=True, stable=True)
    n = 2 * K if n is None else n
    return score[:, :n], idx[:, :n]


def hf_statement(logits, seq, step, running, penalty=1.0, eos=None, min_new=0):
    """The same through transformers' own pieces at fp32, as ``_beam_search`` chains them: log_softmax, RepetitionPenaltyLogitsProcessor and
    MinNewTokensLengthLogitsProcessor on the log-probabilities, + running, torch.topk over K * V."""
    from transformers.generation.logits_process import MinNewTokensLengthLogitsProcessor, RepetitionPenaltyLogitsProcessor
    B, K = running.shape
    R, V = logits.shape
    lp = torch.nn.functional.log_softmax(logits.detach().cpu().float(), dim=-1)
    ids = seq.detach().cpu()[:, :step]
    if penalty != 1.0:
        lp = RepetitionPenaltyLogitsProcessor(penalty=penalty)(ids, lp)
    if eos is not None and min_new > 0:
        lp = MinNewTokensLengthLogitsProcessor(0, min_new, eos, device="cpu")(ids, lp)
    s = (lp.view(B, K, V) + running.detach().cpu().float()[:, :, None]).reshape(B, K * V)
    return torch.topk(s, k=2 * K)


def gather_cache(cp, cg, src_row, n_prompt, K):
    """cp [B, nkv, tmax_p, hd], cg [R, nkv, tmax_g, hd], src_row [R, tmax_g] -> [R, nkv, tmax_p + tmax_g, hd]: key t of row r is
    cp[r // K, :, t] for t < n_prompt and cg[src_row[r, t - n_prompt], :, t - n_prompt] after it (slots past the caches: zeros)."""
    B, nkv, tmax_p, hd = cp.shape
    R, _, tmax_g, _ = cg.shape
    out = torch.zeros(R, nkv, tmax_p + tmax_g, hd, dtype=cp.dtype, device=cp.device)
    out[:, :, :n_prompt] = cp[:, :, :n_prompt].repeat_interleave(K, 0)
    slots = torch.arange(tmax_g, device=cp.device)
    g = cg[src_row.long().clamp(0, R - 1), :, slots[None, :]]      # [R, tmax_g, nkv, hd]
    n = min(tmax_g, tmax_p + tmax_g - n_prompt)
    out[:, :, n_prompt: n_prompt + n] = g.permute(0, 2, 1, 3)[:, :, :n]
    return out


# ---- the inputs of tests/test_gpu_beam_candidates.py
VOCABS, BEAMS, BATCHES = (120, 1000, 32000, 32001), (2, 5, 8), (1, 3)
N_SEQ = 12


def _make(V, K, B, bf16, variant, seed):
    """variant 0: the decoder's first step -- step 0, running [0, -1e9, ...], penalty 1.5, eos blocked (min_new 3).
    variant 1 / 2: step 7 with repeated ids, random running scores with one row of item 0 at -1e9, one row's logits offset by +1e4 (1) or
    -1e4 (2); penalty 1.5 / 1.0; eos free / blocked.  Logits: N(0, 1) with 2K + 2 separated peaks per row, so that a row's best values are
    distinct numbers in bf16 as well."""
    g = torch.Generator().manual_seed(seed)
    R = B * K
    x = torch.randn(R, V, generator=g)
    npk = min(2 * K + 2, V)
    for r in range(R):
        tok = torch.randperm(V, generator=g)[:npk]
        x[r, tok] = 6.0 + 0.37 * torch.arange(npk, dtype=torch.float32) + 0.1 * torch.rand(npk, generator=g)
    seq = torch.randint(0, V, (R, N_SEQ), generator=g)
    eos = int(torch.randint(0, V, (1,), generator=g))
    if variant == 0:
        step, penalty, min_new = 0, 1.5, 3
        running = torch.full((B, K), -1e9)
        running[:, 0] = 0.0
        x[:, eos] = 20.0      # the blocked eos would win every row
    else:
        step, penalty, min_new = 7, (1.5 if variant == 1 else 1.0), (0 if variant == 1 else 9)
        seq[:, 3] = seq[:, 1]                                     # a duplicated id: penalised once
        seq[:, 5] = x.argmax(-1)                                  # the best token of every row has been generated
        seq[:, 8] = x.topk(2, -1).indices[:, 1]                   # (behind `step`: not counted)
        running = -3.0 * torch.rand(B, K, generator=g)
        if K > 2:
            running[0, K - 1] = -1e9
        off = 1e4 if variant == 1 else -1e4
        if bf16:      # (1e4 + x has 64 between neighbouring bf16 numbers: that row's values tie, so it is kept out of the candidates)
            running[B - 1, 1] -= 40.0
        x[R - K + 1] += off
        if variant == 2:
            x[:, eos] = 20.0
    if bf16:
        x = x.bfloat16()
    return dict(logits=x, seq=seq, step=step, running=running, penalty=penalty, eos=eos, min_new=min_new)


def _gap(case, K):
    s, _ = candidates_ref(n=2 * K + 1, **case)
    return float((s[:, :-1] - s[:, 1:]).min())


@functools.lru_cache(maxsize=None)
def candidate_case(V, K, B, bf16, variant):
    """The case's inputs: the first seed from a fixed base whose reference candidates are GAP apart (the search reads the reference alone)."""
    base = 1000 * variant + 100 * BEAMS.index(K) + 10 * VOCABS.index(V) + 2 * B + int(bf16)
    for t in range(64):
        case = _make(V, K, B, bf16, variant, 7919 * base + t)
        if _gap(case, K) >= GAP:
            return case
    raise AssertionError(f"no seed with a gap of {GAP} for V={V} K={K} B={B} bf16={bf16} variant={variant}")


def tie_case(V, K, B, bf16):
    """Identical rows with equal running scores inside every batch item: every score occurs K times, exactly."""
    g = torch.Generator().manual_seed(V + 17 * K + B)
    x = torch.randn(B, 1, V, generator=g).expand(B, K, V).reshape(B * K, V).contiguous()
    seq = torch.randint(0, V, (B, 1, N_SEQ), generator=g).expand(B, K, N_SEQ).reshape(B * K, N_SEQ).contiguous()
    running = (-torch.rand(B, 1, generator=g)).expand(B, K).contiguous()
    return dict(logits=x.bfloat16() if bf16 else x, seq=seq, step=5, running=running, penalty=1.5, eos=None, min_new=0)
