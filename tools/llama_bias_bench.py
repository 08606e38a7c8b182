#!/usr/bin/env python3
"""One decode step of the Llama graph decoder with and without projection biases: same process, same weights, graph replay.

    python tools/llama_bias_bench.py [--layers 32] [--batches 1,124] [--prompt 52] [--new-tokens 64] [--pairs 3] [--out profiles/llama_bias_bench.json]

A random-init language model of Vicuna-7B geometry (--layers of its 32 layers; llm.build_llama) with ``attention_bias`` and ``mlp_bias``, bf16,
biases drawn N(0, 0.02).  Two decoders over it share one copy of the packed weights: "with" carries the biases (every projection of the step
goes through vtgb_gemm_skinny_bias), "without" is the same decoder with its bias table removed -- the same model without biases, which launches
what a model built without the switches launches (vtgb_gemm_skinny).  Per batch size the captured step is replayed --new-tokens - 1 times
between two events, --pairs times alternating the two decoders; medians, every pair and the with / without ratio with its spread are
written as one JSON document to --out and printed.  No ratio is promised: the bias is 4 bytes per output row next to K weight bytes."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import torch  # noqa: E402


def replay_ms(st, P, n):
    """n replays of the captured step from cache row P on (what generate's loop runs after the prefill), ms per token"""
    keep = {k: st[k].clone() for k in ("tok", "pos", "step", "out", "fin", "len")}
    st["step"].fill_(1)
    st["pos"].fill_(P)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(n):
        st["graph"].replay()
    t1.record()
    torch.cuda.synchronize()
    for k, v in keep.items():
        st[k].copy_(v)
    return t0.elapsed_time(t1) / n


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--batches", default="1,124")
    ap.add_argument("--prompt", type=int, default=52)
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "llama_bias_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("llama_bias_bench needs a GPU")
    from videotgb_amd import llm
    from videotgb_amd.decode import GreedyDecoder
    dev = torch.device("cuda:0")
    lm = llm.build_llama("vicuna-7b", torch.bfloat16, dev, seed=0, num_hidden_layers=args.layers, attention_bias=True, mlp_bias=True)
    g = torch.Generator(device=dev).manual_seed(5)
    with torch.no_grad():
        for n, p in lm.named_parameters():
            if n.endswith("proj.bias"):
                p.normal_(0.0, 0.02, generator=g)
    cfg = lm.config
    N, P = args.new_tokens, args.prompt
    biased = GreedyDecoder(lm)
    assert biased.bias is not None
    plain = GreedyDecoder(lm)
    plain.bias = None      # the same model without biases
    plain.layers, plain.head_w = biased.layers, biased.head_w      # one copy of the concatenated weights serves both legs
    plain._skinny = biased._skinny_weights()
    decs = {"without": plain, "with": biased}
    bias_bytes = sum(b.numel() * 4 for t in biased.bias for b in t if b is not None)
    records = []
    for B in [int(b) for b in args.batches.split(",")]:
        emb = (torch.randn(B, P, cfg.hidden_size, generator=g, device=dev) * 0.5).bfloat16()
        ids, sts = {}, {}
        for k, d in decs.items():
            ids[k] = d.generate(emb, N)
            sts[k] = next(reversed(d.graphs.values()))
        pairs = [{k: replay_ms(sts[k], P, N - 1) for k in decs} for _ in range(args.pairs)]
        ratios = [p["with"] / p["without"] for p in pairs]
        rec = {"B": B, "P": P, "new_tokens": N,
               "decode_ms_per_token": {k: round(statistics.median(p[k] for p in pairs), 4) for k in decs},
               "decode_pairs": [{k: round(v, 4) for k, v in p.items()} for p in pairs],
               "with_over_without": {"median": round(statistics.median(ratios), 4), "min": round(min(ratios), 4), "max": round(max(ratios), 4)},
               "ids_agree_with_unbiased": round(float((ids["with"] == ids["without"]).float().mean()), 4)}
        print(json.dumps(rec), flush=True)
        records.append(rec)
        for d in decs.values():
            for st in d.graphs.values():
                st.clear()
            d.graphs.clear()
        del sts, emb
        torch.cuda.empty_cache()
    doc = {"workload": f"{args.layers}-layer LM of Vicuna-7B geometry with attention_bias and mlp_bias, bf16, prompt {P}, {N} new tokens; one captured decode "
                       f"step, {args.pairs} alternating pairs ({bias_bytes} bytes of fp32 biases)",
           "device": torch.cuda.get_device_name(0), "launches_per_layer": {"without": 10, "with": 10}, "batches": records}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": args.out}))


if __name__ == "__main__":
    main()
