#!/usr/bin/env python3
"""The decode step with bf16, fp8 and MXFP4 weights (decode_weights="fp8" / "mxfp4"), same process, same box.

    python tools/mxfp4_decode_bench.py [--layers 32] [--batches 1,124] [--rounds 3] [--replays 64] [--new-tokens 16]
                                       [--limit 420] [--out profiles/mxfp4_decode_bench.json]

A random-init language model of Vicuna-7B geometry (--layers of its 32 layers), bf16, prompts of 40 positions.  For every batch size a
fresh child process under its own time limit (--limit seconds; a child that fails or runs out of time ends the run: nothing more is
started) builds the three decoders (GreedyDecoder(lm), weights="fp8", weights="mxfp4"); each runs one generate call (prefill, graph
capture), then --rounds times, alternating bf16, fp8, mxfp4, --replays replays of its captured decode step between two events: ms per
step per round and its median, the mxfp4 / bf16 and mxfp4 / fp8 ratios with the spread of the rounds, and the weight bytes per step over
the time (TB/s; the projections and lm_head only: 2, 1 and 17 / 32 bytes per weight).  Recorded, not gated (random weights say nothing about
a trained model): rel-RMS of the quantised decoders' first-step logits against the bf16 decoder's, and the share of greedy ids that
agree over --new-tokens tokens.  Writes the JSON to --out and prints it as one line."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

MODES = ("bf16", "fp8", "mxfp4")
BYTES_PER_WEIGHT = {"bf16": 2.0, "fp8": 1.0, "mxfp4": 17.0 / 32.0}


def replay_ms(st, n):
    import torch
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
        import torch
        if not isinstance(step, torch.Tensor):
            seen.append(logits.float().clone())
        return pick(st, logits, step)
    dec._pick = recorder
    return seen


def spread(ratios):
    return {"median": round(statistics.median(ratios), 4), "min": round(min(ratios), 4), "max": round(max(ratios), 4)}


def child(args):
    """One batch size: prints one JSON line."""
    import torch
    if not torch.cuda.is_available():
        sys.exit("mxfp4_decode_bench needs a GPU")
    from videotgb_amd import llm
    from videotgb_amd.decode import GreedyDecoder
    dev = torch.device("cuda:0")
    B, N = args.child, args.new_tokens
    lm = llm.build_llama("vicuna-7b", torch.bfloat16, dev, seed=0, num_hidden_layers=args.layers)
    decs = {"bf16": GreedyDecoder(lm), "fp8": GreedyDecoder(lm, weights="fp8"), "mxfp4": GreedyDecoder(lm, weights="mxfp4")}
    seen = {k: first_logits(d) for k, d in decs.items()}
    n_w = sum(w.numel() for layer in decs["bf16"].layers for w in (layer[1], layer[2], layer[4], layer[5])) + lm.lm_head.weight.numel()
    g = torch.Generator(device=dev).manual_seed(5 + B)
    emb = (torch.randn(B, 40, lm.config.hidden_size, generator=g, device=dev) * 0.5).bfloat16()
    ids, sts = {}, {}
    for k, d in decs.items():
        ids[k] = d.generate(emb, N)
        sts[k] = next(reversed(d.graphs.values()))
        assert sts[k]["graph"] is not None and "sk_ws" in sts[k], k
    rounds = [{k: replay_ms(sts[k], args.replays) for k in MODES} for _ in range(args.rounds)]
    med = {k: statistics.median(r[k] for r in rounds) for k in MODES}
    ref = seen["bf16"][0]
    print(json.dumps({
        "weights_per_step": n_w, "device": torch.cuda.get_device_name(0),
        "ms_per_step": {k: round(v, 4) for k, v in med.items()}, "rounds": [{k: round(v, 4) for k, v in r.items()} for r in rounds],
        "mxfp4_over_bf16": spread([r["mxfp4"] / r["bf16"] for r in rounds]), "mxfp4_over_fp8": spread([r["mxfp4"] / r["fp8"] for r in rounds]),
        "fp8_over_bf16": spread([r["fp8"] / r["bf16"] for r in rounds]),
        "weight_TB_per_s": {k: round(BYTES_PER_WEIGHT[k] * n_w / med[k] * 1e-9, 3) for k in MODES},
        "first_logits_rel_rms": {k: round(float((seen[k][0] - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()), 5) for k in ("fp8", "mxfp4")},
        "greedy_ids_agree": {k: round(float((ids[k] == ids["bf16"]).float().mean()), 4) for k in ("fp8", "mxfp4")}}))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--batches", default="1,124")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--replays", type=int, default=64)
    ap.add_argument("--new-tokens", type=int, default=16)
    ap.add_argument("--limit", type=int, default=420, help="seconds for each batch size's process")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mxfp4_decode_bench.json"))
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    out = {"workload": f"{args.layers}-layer LM of Vicuna-7B geometry, bf16 activations, prompt 40, hipGraph replay of one decode step; bf16, fp8 and "
                       f"mxfp4 alternating in one process per batch size, {args.rounds} rounds of {args.replays} replays", "batches": {}}
    for B in [int(b) for b in args.batches.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(B), "--layers", str(args.layers), "--rounds", str(args.rounds),
               "--replays", str(args.replays), "--new-tokens", str(args.new_tokens)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"mxfp4_decode_bench: batch {B} did not finish within {args.limit} s; nothing more is started")
        if p.returncode != 0:
            sys.exit(f"mxfp4_decode_bench: batch {B} ended with status {p.returncode}; nothing more is started")
        res = json.loads(p.stdout.strip().splitlines()[-1])
        out["weights_per_step"], out["device"] = res.pop("weights_per_step"), res.pop("device")
        out["batches"][str(B)] = res
        print(f"batch {B}: ms per step {res['ms_per_step']}", file=sys.stderr, flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
