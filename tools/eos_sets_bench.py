#!/usr/bin/env python3
"""Eos-id sets on the Llama graph decoder (eos_sets="graph") against the single-eos path and against HF generate, same process.

    python tools/eos_sets_bench.py [--layers 32] [--batches 1,8] [--beams 5] [--prompt 52] [--new-tokens 64] [--rounds 3] [--out FILE]

A random-init language model of Vicuna-7B geometry (--layers of its 32 layers), bf16.  For every batch size B, greedy and with --beams beams
(repetition_penalty 1.5), three whole calls -- prefill included -- over the same prompt embeddings:
  one   GreedyDecoder.generate(eos_token_id=e): one eos id, today's path (the chain of torch ops in the greedy step, vtgb_llm_beam_candidates)
  set   GreedyDecoder(eos_sets=True).generate(eos_token_id=[e, f, g]): three ids on vtgb_llm_pick_greedy / vtgb_llm_beam_candidates_eos
  hf    lm.generate(eos_token_id=[e, f, g], ...): the same request on HF generate (eos_sets="hf", the behaviour of before)
The ids are ones the model does not emit on these prompts (taken from outside its eos-free output), so that all --new-tokens steps run; the
number of tokens every leg returned is recorded.  After one warm-up call each (graph capture, allocator), --rounds rounds run the three
alternately; a call is timed between two synchronisations on the host clock.  Reported: ms per generated token (call time / new tokens) per
round and its median, the ratios set / one and hf / set with the spread over the rounds, and whether the legs returned the same ids (bf16:
recorded, not gated).  Prints one JSON line and writes it to --out (default profiles/eos_sets_bench.json)."""
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "eos_sets_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eos_sets_bench needs a GPU")
    from videotgb_amd import llm
    from videotgb_amd.decode import GreedyDecoder
    dev = torch.device("cuda:0")
    lm = llm.build_llama("vicuna-7b", torch.bfloat16, dev, seed=0, num_hidden_layers=args.layers).eval()
    with torch.no_grad():      # (N(0, 0.02) leaves near-uniform logits: a wider lm_head and embedding make the rows and beams differ)
        lm.lm_head.weight.mul_(4.0)
        lm.model.embed_tokens.weight.mul_(20.0)
    dec_one, dec_set = GreedyDecoder(lm), GreedyDecoder(lm, eos_sets=True)
    K, P, N = args.beams, args.prompt, args.new_tokens
    out = {"workload": f"{args.layers}-layer LM of Vicuna-7B geometry, bf16, prompt {P}, {N} new tokens; greedy and {K} beams with "
                       f"repetition_penalty 1.5; one eos id / a set of three / HF generate with the set; whole calls", "points": {}}
    g = torch.Generator(device=dev).manual_seed(5)
    for B in [int(b) for b in args.batches.split(",")]:
        emb = (torch.randn(B, P, lm.config.hidden_size, generator=g, device=dev) * 0.5).bfloat16()
        mask = torch.ones(B, P, dtype=torch.long, device=dev)
        for mode, kw in (("greedy", {}), (f"beams{K}", dict(num_beams=K, repetition_penalty=1.5, length_penalty=1.0))):
            free = dec_one.generate(emb, N, eos_token_id=None, pad_token_id=0, **kw)
            emitted = set(free.flatten().tolist())
            ids = [v for v in range(lm.config.vocab_size - 1, 0, -1) if v not in emitted][:3]      # ids the model does not emit here

            def one():
                return dec_one.generate(emb, N, eos_token_id=ids[0], pad_token_id=0, **kw)

            def eos_set():
                return dec_set.generate(emb, N, eos_token_id=ids, pad_token_id=0, **kw)

            def hf():
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    return lm.generate(inputs_embeds=emb, attention_mask=mask, do_sample=False, max_new_tokens=N, eos_token_id=ids, pad_token_id=0, **kw)
            runs = {"one": one, "set": eos_set, "hf": hf}
            got = {k: fn() for k, fn in runs.items()}      # warm-up: graph capture, workspaces
            rounds = []
            for _ in range(args.rounds):
                rounds.append({k: timed(fn)[0] / N for k, fn in runs.items()})
            med = {k: statistics.median(r[k] for r in rounds) for k in runs}
            r1, r2 = [r["set"] / r["one"] for r in rounds], [r["hf"] / r["set"] for r in rounds]
            out["points"][f"B{B}_{mode}"] = {
                "eos_ids": ids, "tokens_returned": {k: int(v.shape[1]) for k, v in got.items()},
                "ms_per_token": {k: round(v, 4) for k, v in med.items()}, "rounds": [{k: round(v, 4) for k, v in r.items()} for r in rounds],
                "set_over_one": {"median": round(statistics.median(r1), 3), "min": round(min(r1), 3), "max": round(max(r1), 3)},
                "hf_over_set": {"median": round(statistics.median(r2), 3), "min": round(min(r2), 3), "max": round(max(r2), 3)},
                "set_ids_equal_one": bool(got["set"].shape == got["one"].shape and torch.equal(got["set"], got["one"])),
                "set_ids_equal_hf": bool(got["set"].shape == got["hf"].shape and torch.equal(got["set"], got["hf"]))}
    out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
