#!/usr/bin/env python3
"""Time to first token of prompts past the one-shot prefill's 2048 tokens: the chunked prefill against the torch route, same process.

    python tools/long_prefill_bench.py [--layers 32] [--prompts 2304,4096,8192] [--pairs 3] [--kv-cache bf16] [--out profiles/long_prefill_bench.json]

A random-init language model of Vicuna-7B geometry (--layers of its 32 layers; llm.build_llama), bf16, B = 1.  For every prompt length two
decoders over the same weights -- GreedyDecoder(lm) (chunked prefill: vtgb_gemm + vtgb_attention_cached + vtgb_llm_*, chunks of
PREFILL_CHUNK_TOKENS rows) and the same with PREFILL_MAX_TOKENS = 0 (the torch route: F.linear + SDPA under a materialised mask) -- each run
one warm-up ``generate(emb, 1)``; then --pairs times, alternating, one ``generate(emb, 1)`` (prefill, lm_head, the first token's pick) is
timed with a host clock between two device synchronisations.  Reported per prompt length: ms per leg and pair, the medians, the
chunked / torch ratio with the spread of the pairs, the peak device memory of one call per leg, and whether the first tokens agree.
The JSON (one record per prompt length) is printed and written to --out.  No threshold hangs on it."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import torch  # noqa: E402


def first_token_ms(dec, emb):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ids = dec.generate(emb, 1)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, ids


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--prompts", default="2304,4096,8192")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--kv-cache", default="bf16", choices=("bf16", "fp8"))
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "long_prefill_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("long_prefill_bench needs a GPU")
    from videotgb_amd import llm
    from videotgb_amd.decode import GreedyDecoder, prefill_chunks
    dev = torch.device("cuda:0")
    lm = llm.build_llama("vicuna-7b", torch.bfloat16, dev, seed=0, num_hidden_layers=args.layers)
    cfg = lm.config
    g = torch.Generator(device=dev).manual_seed(5)
    decs = {"chunked": GreedyDecoder(lm, kv_cache=args.kv_cache), "torch": GreedyDecoder(lm, kv_cache=args.kv_cache)}
    decs["torch"].PREFILL_MAX_TOKENS = 0
    records = []
    for P in [int(p) for p in args.prompts.split(",")]:
        emb = (torch.randn(1, P, cfg.hidden_size, generator=g, device=dev) * 0.5).bfloat16()
        first, peak = {}, {}
        for k, d in decs.items():      # warm-up: code objects, the state and its graph, the allocator's blocks
            d.generate(emb, 1)
            st = next(reversed(d.graphs.values()))
            assert d._use_chunked_prefill(st, emb, P) == (k == "chunked") and not d._use_hip_prefill(emb, P)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            first[k] = d.generate(emb, 1)
            torch.cuda.synchronize()
            peak[k] = torch.cuda.max_memory_allocated()
        pairs = [{k: round(first_token_ms(d, emb)[0], 3) for k, d in decs.items()} for _ in range(args.pairs)]
        ratios = [p["chunked"] / p["torch"] for p in pairs]
        med = {k: round(statistics.median(p[k] for p in pairs), 3) for k in decs}
        rec = {"workload": f"{args.layers}-layer LM of Vicuna-7B geometry, bf16, kv_cache={args.kv_cache}, B=1: generate(emb, 1), prefill to the first token",
               "device": torch.cuda.get_device_name(0), "P": P, "chunks": prefill_chunks(P, GreedyDecoder.PREFILL_CHUNK_TOKENS),
               "first_token_ms": med, "pairs": pairs,
               "chunked_over_torch": {"median": round(statistics.median(ratios), 4), "min": round(min(ratios), 4), "max": round(max(ratios), 4)},
               "peak_allocated_MiB": {k: round(v / 2 ** 20) for k, v in peak.items()},
               "first_tokens_agree": bool(torch.equal(first["chunked"], first["torch"]))}
        print(json.dumps(rec), flush=True)
        records.append(rec)
        for d in decs.values():      # the caches of this length go before the next one is built
            for st in d.graphs.values():
                st.clear()
            d.graphs.clear()
        del emb
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
