#!/usr/bin/env python3
"""Beam search on the Llama graph decoder over the fp8 K/V cache (beam_search="graph+kv8", kv_cache="fp8") against the same search over the
bf16 cache (beam_search="graph"), same process, same box.

    python tools/beam_kv_fp8_bench.py [--layers 32] [--batches 1,8] [--prompts 52,308] [--beams 5] [--new-tokens 64] [--rounds 3]
                                      [--weights bf16] [--out FILE]

A random-init language model of Vicuna-7B geometry (--layers of its 32 layers), bf16 activations, synthetic weights.  For every weight mode,
batch size B and prompt length P two whole calls -- prefill included -- over the same prompt embeddings, each asked for exactly --new-tokens
tokens (min_new_tokens = max_new_tokens: fixed work) with the shipped SF request's num_beams / repetition_penalty:
  bf16   GreedyDecoder(lm, weights=w).generate(num_beams=K, ...): the bf16-cache beam decoder (vtgb_llm_decode_attention_beam)
  fp8    GreedyDecoder(lm, weights=w, kv_cache="fp8", fp8_beams=True).generate(...): code caches (vtgb_llm_decode_attention_beam_fp8)
After one warm-up call each (graph capture, allocator), --rounds rounds run the two alternately; a call is timed between two
synchronisations on the host clock.  Reported: ms per generated token (call time / new tokens) per round and its median, the ratio
fp8 / bf16 with the spread over the rounds, the bytes of K/V either state holds, and how many ids the two searches share (they decode
different models: recorded, not gated).  Prints one JSON line and writes it to --out (default profiles/beam_kv_fp8_bench.json)."""
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

KV_KEYS = ("kc", "vc", "kc8", "vc8", "ks", "vs", "kg", "vg", "kg8", "vg8", "kgs", "vgs")


def kv_bytes(st):
    """The K/V a beam state holds: the prompt state's caches (B rows) and the generated caches (B * K rows)."""
    return sum(t.numel() * t.element_size() for s in (st, st["prompt"]) for k in KV_KEYS for t in s.get(k, ()))


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
    ap.add_argument("--prompts", default="52,308")
    ap.add_argument("--beams", type=int, default=5)
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--weights", default="bf16", help="comma-separated decode_weights modes (bf16, fp8, mxfp4)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "beam_kv_fp8_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("beam_kv_fp8_bench needs a GPU")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from videotgb_amd import llm
    from videotgb_amd.decode import GreedyDecoder
    dev = torch.device("cuda:0")
    lm = llm.build_llama("vicuna-7b", torch.bfloat16, dev, seed=0, num_hidden_layers=args.layers).eval()
    with torch.no_grad():      # (N(0, 0.02) leaves near-uniform logits: a wider lm_head and embedding make the beams differ)
        lm.lm_head.weight.mul_(4.0)
        lm.model.embed_tokens.weight.mul_(20.0)
    K, N = args.beams, args.new_tokens
    out = {"workload": f"{args.layers}-layer LM of Vicuna-7B geometry, synthetic weights, bf16 activations, {N} new tokens, {K} beams, "
                       "repetition_penalty 1.5; whole calls (prefill + hipGraph replay of the beam step)", "cases": []}
    g = torch.Generator(device=dev).manual_seed(5)
    for w in args.weights.split(","):
        decs = {"bf16": GreedyDecoder(lm, weights=w), "fp8": GreedyDecoder(lm, weights=w, kv_cache="fp8", fp8_beams=True)}
        # (both legs multiply by the same matrices: one copy of the re-packed weight streams serves both)
        decs["fp8"].layers, decs["fp8"].head_w = decs["bf16"].layers, decs["bf16"].head_w
        decs["fp8"]._skinny = decs["bf16"]._skinny_weights()
        for B in [int(b) for b in args.batches.split(",")]:
            for P in [int(p) for p in args.prompts.split(",")]:
                emb = (torch.randn(B, P, lm.config.hidden_size, generator=g, device=dev) * 0.5).bfloat16()

                def call(dec):
                    return dec.generate(emb, N, eos_token_id=2, pad_token_id=0, min_new_tokens=N, num_beams=K, repetition_penalty=1.5, length_penalty=1.0)
                ids, held = {}, {}
                for k, d in decs.items():      # warm-up: graph capture, workspaces
                    ids[k] = call(d)
                    st = next(reversed(d.graphs.values()))
                    assert st["attn"] == ("beam_fp8" if k == "fp8" else "beam") and st["graph"] is not None
                    held[k] = kv_bytes(st)
                rounds = [{k: timed(lambda d=d: call(d))[0] / N for k, d in decs.items()} for _ in range(args.rounds)]
                ratios = [r["fp8"] / r["bf16"] for r in rounds]
                rec = {"weights": w, "B": B, "K": K, "P": P, "kv_bytes_per_state": held,
                       "ms_per_token": {k: round(statistics.median(r[k] for r in rounds), 4) for k in decs},
                       "rounds": [{k: round(v, 4) for k, v in r.items()} for r in rounds],
                       "fp8_over_bf16": {"median": round(statistics.median(ratios), 4), "min": round(min(ratios), 4), "max": round(max(ratios), 4)},
                       "ids_shared": round(float((ids["fp8"] == ids["bf16"]).float().mean()), 4) if ids["fp8"].shape == ids["bf16"].shape else None}
                print(json.dumps(rec), file=sys.stderr, flush=True)
                out["cases"].append(rec)
                for d in decs.values():      # the caches of this shape go before the next one is built
                    for st in d.graphs.values():
                        st.clear()
                    d.graphs.clear()
                del emb
                torch.cuda.empty_cache()
        del decs
        torch.cuda.empty_cache()
    out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
