#!/usr/bin/env python3
"""A one-beam repetition penalty on the Llama graph decoder (penalty_decode="graph") against the unpenalised path and HF generate, same process.

    python tools/penalty_decode_bench.py [--layers 32] [--batches 1,8] [--penalty 1.5] [--prompt 52] [--new-tokens 64] [--rounds 3] [--out FILE]

A random-init language model of Vicuna-7B geometry (--layers of its 32 layers), bf16, greedy, no eos (all --new-tokens steps run).  For every
batch size B, four whole calls -- prefill included -- over the same prompt embeddings:
  p1         GreedyDecoder(penalty=True).generate(repetition_penalty=1.0): the path of a decoder without the opt-in (no penalty operands, no launch)
  kernel     the same decoder with repetition_penalty=--penalty: vtgb_llm_repetition_penalty in front of the emission of the captured step
  statement  a second decoder with PENALTY_KERNEL = False: the torch gather / scatter statement in the captured step
  hf         lm.generate(repetition_penalty=--penalty, ...): the same request on HF generate (penalty_decode="hf", the behaviour of before)
After one warm-up call each (graph capture, allocator), --rounds rounds run the four alternately; a call is timed between two synchronisations
on the host clock.  Reported: ms per generated token (call time / new tokens) per round and its median, the ratios kernel / p1, statement /
kernel and hf / kernel with the spread over the rounds, and whether the legs returned the same ids (bf16: recorded, not gated).  Llama only.
Prints one JSON line and writes it to --out (default profiles/penalty_decode_bench.json)."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import torch  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--penalty", type=float, default=1.5)
    ap.add_argument("--prompt", type=int, default=52)
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "penalty_decode_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("penalty_decode_bench needs a GPU")
    from videotgb_amd import llm
    from videotgb_amd.decode import GreedyDecoder
    dev = torch.device("cuda:0")
    lm = llm.build_llama("vicuna-7b", torch.bfloat16, dev, seed=0, num_hidden_layers=args.layers).eval()
    with torch.no_grad():      # (N(0, 0.02) leaves near-uniform logits: a wider lm_head and embedding make the rows differ and repeat ids)
        lm.lm_head.weight.mul_(4.0)
        lm.model.embed_tokens.weight.mul_(20.0)
    dec, dec_stmt = GreedyDecoder(lm, penalty=True), GreedyDecoder(lm, penalty=True)
    dec_stmt.PENALTY_KERNEL = False
    p, P, N = args.penalty, args.prompt, args.new_tokens
    out = {"workload": f"{args.layers}-layer LM of Vicuna-7B geometry, bf16, prompt {P}, {N} new tokens, greedy, no eos; repetition_penalty 1 / {p} on the "
                       f"kernel / {p} on the torch statement / HF generate with {p}; whole calls", "points": {}}
    g = torch.Generator(device=dev).manual_seed(5)
    for B in [int(b) for b in args.batches.split(",")]:
        emb = (torch.randn(B, P, lm.config.hidden_size, generator=g, device=dev) * 0.5).bfloat16()
        mask = torch.ones(B, P, dtype=torch.long, device=dev)

        def p1():
            return dec.generate(emb, N, eos_token_id=None, pad_token_id=0)

        def kernel():
            return dec.generate(emb, N, eos_token_id=None, pad_token_id=0, repetition_penalty=p)

        def statement():
            return dec_stmt.generate(emb, N, eos_token_id=None, pad_token_id=0, repetition_penalty=p)

        def hf():
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                return lm.generate(inputs_embeds=emb, attention_mask=mask, do_sample=False, max_new_tokens=N, eos_token_id=None, pad_token_id=0,
                                   repetition_penalty=p)
        runs = {"p1": p1, "kernel": kernel, "statement": statement, "hf": hf}
        got = {k: fn() for k, fn in runs.items()}      # warm-up: graph capture, workspaces
        rounds = []
        for _ in range(args.rounds):
            rounds.append({k: timed(fn)[0] / N for k, fn in runs.items()})
        med = {k: statistics.median(r[k] for r in rounds) for k in runs}
        out["points"][f"B{B}"] = {
            "tokens_returned": {k: int(v.shape[1]) for k, v in got.items()},
            "ms_per_token": {k: round(v, 4) for k, v in med.items()}, "rounds": [{k: round(v, 4) for k, v in r.items()} for r in rounds],
            "kernel_over_p1": spread([r["kernel"] / r["p1"] for r in rounds]),
            "statement_over_kernel": spread([r["statement"] / r["kernel"] for r in rounds]),
            "hf_over_kernel": spread([r["hf"] / r["kernel"] for r in rounds]),
            "kernel_minus_p1_us_per_token": round((med["kernel"] - med["p1"]) * 1e3, 1),
            "penalty_changes_ids": bool(not torch.equal(got["kernel"], got["p1"])),
            "kernel_ids_equal_statement": bool(torch.equal(got["kernel"], got["statement"])),
            "kernel_ids_equal_hf": bool(got["kernel"].shape == got["hf"].shape and torch.equal(got["kernel"], got["hf"]))}
    out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
