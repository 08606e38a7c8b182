#!/usr/bin/env python3
"""The decode step with bf16 and with fp8 weights (decode_weights="fp8"), same process, same box.

    python tools/fp8_decode_bench.py [--layers 32] [--batches 1,124] [--pairs 3] [--replays 64] [--new-tokens 16]

A random-init language model of Vicuna-7B geometry (--layers of its 32 layers), bf16, prompts of 40 positions.  For every batch size the
two decoders (GreedyDecoder(lm) and GreedyDecoder(lm, weights="fp8")) each run one generate call (prefill, graph capture), then --pairs
times, alternating, --replays replays of their captured decode step between two events: ms per step, per pair and its median, the
fp8 / bf16 ratio with the spread of the pairs, and the weight bytes per step over the time (TB/s; the projections and lm_head only).
Recorded, not gated (random weights say nothing about a trained model): rel-RMS of the fp8 decoder's first-step logits against the bf16
decoder's, and the share of greedy ids that agree over --new-tokens tokens.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import torch  # noqa: E402


def replay_ms(st, n):
    g = st["graph"]
    keep = {k: st[k].clone() for k in ("tok", "pos", "step", "out", "fin", "len")}
    st["step"].fill_(1)      # (every replay advances step / pos: stay inside the buffers)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    room = st["out"].shape[1] - 1
    torch.cuda.synchronize()
    t0.record()
    for i in range(n):
        if i % room == 0:
            st["step"].fill_(1)
            st["pos"].fill_(40)
        g.replay()
    t1.record()
    torch.cuda.synchronize()
    for k, v in keep.items():
        st[k].copy_(v)
    return t0.elapsed_time(t1) / n


def first_logits(dec):
    seen = []
    pick = dec._pick

    def recorder(st, logits, step):
        if not isinstance(step, torch.Tensor):
            seen.append(logits.float().clone())
        return pick(st, logits, step)
    dec._pick = recorder
    return seen


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--batches", default="1,124")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--replays", type=int, default=64)
    ap.add_argument("--new-tokens", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fp8_decode_bench needs a GPU")
    from videotgb_amd import llm
    from videotgb_amd.decode import GreedyDecoder
    dev = torch.device("cuda:0")
    lm = llm.build_llama("vicuna-7b", torch.bfloat16, dev, seed=0, num_hidden_layers=args.layers)
    decs = {"bf16": GreedyDecoder(lm), "fp8": GreedyDecoder(lm, weights="fp8")}
    seen = {k: first_logits(d) for k, d in decs.items()}
    n_w = sum(w.numel() for layer in decs["bf16"].layers for w in (layer[1], layer[2], layer[4], layer[5])) + lm.lm_head.weight.numel()
    out = {"workload": f"{args.layers}-layer LM of Vicuna-7B geometry, bf16 activations, prompt 40, hipGraph replay of one decode step",
           "weights_per_step": n_w, "batches": {}}
    g = torch.Generator(device=dev).manual_seed(5)
    N = args.new_tokens
    for B in [int(b) for b in args.batches.split(",")]:
        emb = (torch.randn(B, 40, lm.config.hidden_size, generator=g, device=dev) * 0.5).bfloat16()
        ids, sts = {}, {}
        for k, d in decs.items():
            del seen[k][:]
            ids[k] = d.generate(emb, N)
            sts[k] = next(reversed(d.graphs.values()))
        pairs = [{k: replay_ms(sts[k], args.replays) for k in ("bf16", "fp8")} for _ in range(args.pairs)]
        ratios = [p["fp8"] / p["bf16"] for p in pairs]
        med = {k: statistics.median(p[k] for p in pairs) for k in ("bf16", "fp8")}
        a, b = seen["fp8"][0], seen["bf16"][0]
        out["batches"][str(B)] = {
            "ms_per_step": {k: round(v, 4) for k, v in med.items()}, "pairs": [{k: round(v, 4) for k, v in p.items()} for p in pairs],
            "fp8_over_bf16": {"median": round(statistics.median(ratios), 4), "min": round(min(ratios), 4), "max": round(max(ratios), 4)},
            "weight_TB_per_s": {"bf16": round(2 * n_w / med["bf16"] * 1e-9, 3), "fp8": round(n_w / med["fp8"] * 1e-9, 3)},
            "first_logits_rel_rms": round(float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()), 5),
            "greedy_ids_agree": round(float((ids["fp8"] == ids["bf16"]).float().mean()), 4)}
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
