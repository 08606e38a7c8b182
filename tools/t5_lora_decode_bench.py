#!/usr/bin/env python3
"""LoRA adapters on the T5 graph decoder: the one-launch and the two-launch form, the adapter-free decoder and HF generate, same process.

    python tools/t5_lora_decode_bench.py [--layers 24] [--batches 1,8] [--encoder 96] [--new-tokens 64] [--rounds 3] [--out FILE]

A random-init T5ForConditionalGeneration of Flan-T5-XL geometry (tools/t5_beam_decode_bench.py: d_model 2048, 24 + 24 blocks, 32 heads, d_kv
64, d_ff 5120), bf16.  The adapter-free decoder is built first; then the reference's adapters (train.apply_lora: r = 8, alpha = 32 on q and v
of every attention block, lora_B ~ N(0, 0.02)) wrap the same model.  For every batch size B, four whole greedy calls -- encoder included --
over the same encoder input of --encoder positions, each asked for exactly --new-tokens tokens:
  parts    T5GreedyDecoder with LORA_PARTS = True: the step's q|k|v and cross-q projections leave their K-split fragments and ONE
           vtgb_llm_lora_parts launch each reduces them and applies the adapters
  two      LORA_PARTS = False: projection + reduce launches, then vtgb_llm_lora on the materialised projection
  base     the adapter-free decoder over the same base weights (what the adapters cost)
  hf       lm.generate over the LoraLinear model: where the request went before
After one warm-up call each (graph capture, allocator), --rounds rounds run the four alternately; a call is timed between two
synchronisations on the host clock.  Reported: ms per generated token (call time / new tokens) per round and its median, the ratios two /
parts, parts / base and hf / parts with their spread over the rounds, and whether parts and two returned the same ids (they must) and parts
and hf (bf16: recorded, not gated).  Prints one JSON line and writes it to --out (default profiles/t5_lora_decode_bench.json)."""
import argparse
import json
import os
import statistics
import sys
import warnings

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from t5_beam_decode_bench import build_flan_t5_xl, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--encoder", type=int, default=96)
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "t5_lora_decode_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("t5_lora_decode_bench needs a GPU")
    from videotgb_amd import train
    from videotgb_amd.decode import T5GreedyDecoder, lora_state
    dev = torch.device("cuda:0")
    lm = build_flan_t5_xl(args.layers, dev)
    base = T5GreedyDecoder(lm)
    assert base.lora is None
    train.apply_lora(lm, r=8, lora_alpha=32, lora_dropout=0.1)
    g = torch.Generator(device=dev).manual_seed(5)
    with torch.no_grad():
        for n, p in lm.named_parameters():
            if "lora_B" in n:
                p.normal_(0.0, 0.02, generator=g)
    lm.eval()
    assert lora_state(lm) == "ok"
    decs = {"parts": T5GreedyDecoder(lm), "two": T5GreedyDecoder(lm), "base": base}
    decs["parts"].LORA_PARTS, decs["two"].LORA_PARTS = True, False
    for d in (decs["parts"], decs["two"]):
        d._sk = base._sk      # (one tiled copy of every unconcatenated base weight serves the three decoders)
    P, N = args.encoder, args.new_tokens
    out = {"workload": f"{args.layers}+{args.layers}-layer T5 of Flan-T5-XL geometry, bf16, encoder input {P}, {N} new tokens, greedy; adapters r=8 "
                       "alpha=32 on q / v of every attention block; whole calls", "shipped_LORA_PARTS": bool(T5GreedyDecoder.LORA_PARTS), "batches": {}}
    for B in [int(b) for b in args.batches.split(",")]:
        emb = (torch.randn(B, P, lm.config.d_model, generator=g, device=dev) * 0.5).bfloat16()
        mask = torch.ones(B, P, dtype=torch.long, device=dev)

        def hf():
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                return lm.generate(inputs_embeds=emb, attention_mask=mask, do_sample=False, max_new_tokens=N, min_new_tokens=N, eos_token_id=1, pad_token_id=0)
        runs = {k: (lambda d=d: d.generate(emb, N, eos_token_id=1, pad_token_id=0, min_new_tokens=N)) for k, d in decs.items()}
        runs["hf"] = hf
        ids = {k: fn() for k, fn in runs.items()}      # warm-up: graph capture, workspaces
        rounds = [{k: timed(fn)[0] / N for k, fn in runs.items()} for _ in range(args.rounds)]
        med = {k: statistics.median(r[k] for r in rounds) for k in runs}

        def ratio(a, b):
            v = [r[a] / r[b] for r in rounds]
            return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        out["batches"][str(B)] = {
            "ms_per_token": {k: round(v, 4) for k, v in med.items()}, "rounds": [{k: round(v, 4) for k, v in r.items()} for r in rounds],
            "two_over_parts": ratio("two", "parts"), "parts_over_base": ratio("parts", "base"), "hf_over_parts": ratio("hf", "parts"),
            "parts_ids_equal_two": bool(torch.equal(ids["parts"], ids["two"])),
            "parts_ids_agree_with_hf": round(float((ids["parts"] == ids["hf"]).float().mean()), 4) if ids["parts"].shape == ids["hf"].shape else None,
            "parts_ids_agree_with_base": round(float((ids["parts"] == ids["base"]).float().mean()), 4)}
    out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
