#!/usr/bin/env python3
"""Beam search on the Llama graph decoder (beam_search="graph") against HF generate and against the decoder's own greedy step, same process.

    python tools/beam_decode_bench.py [--layers 32] [--batches 1,8] [--beams 5] [--prompt 52] [--new-tokens 64] [--pairs 3] [--out FILE]

A random-init language model of Vicuna-7B geometry (--layers of its 32 layers), bf16.  For every batch size B, three whole calls -- prefill
included -- over the same prompt embeddings, each asked for exactly --new-tokens tokens (min_new_tokens = max_new_tokens: fixed work):
  graph   GreedyDecoder.generate(num_beams=K, repetition_penalty=1.5): the prompt prefilled on B rows, B * K beam rows per step
  hf      lm.generate(num_beams=K, repetition_penalty=1.5, ...): the same request on HF generate (beam_search="hf", the behaviour of before)
  greedy  GreedyDecoder.generate on B * K rows: the decoder's plain step at the beam rows' batch size (no beam bookkeeping, K/V per row)
After one warm-up call each (graph capture, allocator), --pairs rounds run the three alternately; a call is timed between two
synchronisations on the host clock.  Reported: ms per generated token (call time / new tokens) per round and its median, the ratios
hf / graph and graph / greedy with the spread over the rounds, and whether graph and hf returned the same ids (bf16: recorded, not
gated).  Prints one JSON line and writes it to --out (default profiles/beam_decode_bench.json)."""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--beams", type=int, default=5)
    ap.add_argument("--prompt", type=int, default=52)
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "beam_decode_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("beam_decode_bench needs a GPU")
    from videotgb_amd import llm
    from videotgb_amd.decode import GreedyDecoder
    dev = torch.device("cuda:0")
    lm = llm.build_llama("vicuna-7b", torch.bfloat16, dev, seed=0, num_hidden_layers=args.layers).eval()
    with torch.no_grad():      # (N(0, 0.02) leaves near-uniform logits: a wider lm_head and embedding make the beams differ)
        lm.lm_head.weight.mul_(4.0)
        lm.model.embed_tokens.weight.mul_(20.0)
    dec = GreedyDecoder(lm)
    K, P, N = args.beams, args.prompt, args.new_tokens
    out = {"workload": f"{args.layers}-layer LM of Vicuna-7B geometry, bf16, prompt {P}, {N} new tokens, {K} beams, repetition_penalty 1.5; whole calls",
           "batches": {}}
    g = torch.Generator(device=dev).manual_seed(5)
    for B in [int(b) for b in args.batches.split(",")]:
        emb = (torch.randn(B, P, lm.config.hidden_size, generator=g, device=dev) * 0.5).bfloat16()
        mask = torch.ones(B, P, dtype=torch.long, device=dev)
        wide = emb.repeat_interleave(K, 0).contiguous()

        def graph():
            return dec.generate(emb, N, eos_token_id=2, pad_token_id=0, min_new_tokens=N, num_beams=K, repetition_penalty=1.5, length_penalty=1.0)

        def hf():
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                return lm.generate(inputs_embeds=emb, attention_mask=mask, do_sample=False, num_beams=K, repetition_penalty=1.5, length_penalty=1.0,
                                   max_new_tokens=N, min_new_tokens=N, eos_token_id=2, pad_token_id=0)

        def greedy():
            return dec.generate(wide, N, eos_token_id=2, pad_token_id=0, min_new_tokens=N)
        runs = {"graph": graph, "hf": hf, "greedy": greedy}
        ids = {k: fn() for k, fn in runs.items()}      # warm-up: graph capture, workspaces
        rounds = []
        for _ in range(args.pairs):
            rounds.append({k: timed(fn)[0] / N for k, fn in runs.items()})
        med = {k: statistics.median(r[k] for r in rounds) for k in runs}
        r1, r2 = [r["hf"] / r["graph"] for r in rounds], [r["graph"] / r["greedy"] for r in rounds]
        out["batches"][str(B)] = {
            "ms_per_token": {k: round(v, 4) for k, v in med.items()}, "rounds": [{k: round(v, 4) for k, v in r.items()} for r in rounds],
            "hf_over_graph": {"median": round(statistics.median(r1), 3), "min": round(min(r1), 3), "max": round(max(r1), 3)},
            "graph_over_greedy_at_BK_rows": {"median": round(statistics.median(r2), 3), "min": round(min(r2), 3), "max": round(max(r2), 3)},
            "graph_ids_equal_hf": bool(ids["graph"].shape == ids["hf"].shape and torch.equal(ids["graph"], ids["hf"]))}
    out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
