#!/usr/bin/env python3
"""The decode step over a bf16 and over an fp8 K/V cache (kv_cache="fp8"), same process, same box.

    python tools/kv_fp8_bench.py [--layers 32] [--batches 1,16,124] [--prompts 288,1024,2000] [--new-tokens 32] [--pairs 3] [--out FILE]

A random-init language model of Vicuna-7B geometry (--layers of its 32 layers; llm.build_llama), bf16 activations.  For every weight mode
(bf16, fp8), batch size and prompt length the two decoders -- GreedyDecoder(lm, weights=w) and GreedyDecoder(lm, weights=w, kv_cache="fp8")
-- each run one generate call of --new-tokens tokens (prefill, graph capture); then --pairs times, alternating, the --new-tokens - 1
replays of their captured decode step from the prompt's end are timed between two events: ms per token per leg, per pair and its
median, and the fp8 / bf16 ratio with the spread of the pairs.  Below 2112 cache slots the bf16 leg runs the one-wave attention kernel
and the fp8 leg the split kernel; from there both run split kernels.  Also printed: the bytes of K/V a state holds in both modes.  A
shape whose two states do not fit in the free device memory is skipped and says so.  One JSON line per shape (--out: appended to FILE
too), then a summary line."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import torch  # noqa: E402

KV_KEYS = ("kc", "vc", "kc8", "vc8", "ks", "vs")


def kv_bytes(st):
    return sum(t.numel() * t.element_size() for k in KV_KEYS for t in st.get(k, ()))


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
    ap.add_argument("--batches", default="1,16,124")
    ap.add_argument("--prompts", default="288,1024,2000")
    ap.add_argument("--new-tokens", type=int, default=32)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--weights", default="bf16,fp8")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("kv_fp8_bench needs a GPU")
    from videotgb_amd import llm
    from videotgb_amd.decode import GreedyDecoder
    dev = torch.device("cuda:0")
    lm = llm.build_llama("vicuna-7b", torch.bfloat16, dev, seed=0, num_hidden_layers=args.layers)
    cfg = lm.config
    N = args.new_tokens
    g = torch.Generator(device=dev).manual_seed(5)
    lines = []

    def emit(rec):
        rec["device"] = torch.cuda.get_device_name(0)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(rec)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    for w in args.weights.split(","):
        decs = {"bf16": GreedyDecoder(lm, weights=w), "fp8": GreedyDecoder(lm, weights=w, kv_cache="fp8")}
        # (both legs multiply by the same matrices: one copy of the re-packed weight streams serves both, to leave the memory to the caches)
        decs["fp8"].layers, decs["fp8"].head_w = decs["bf16"].layers, decs["bf16"].head_w
        for B in [int(b) for b in args.batches.split(",")]:
            if B <= GreedyDecoder.SKINNY_MAX_BATCH:
                decs["fp8"]._skinny = decs["bf16"]._skinny_weights()
            for P in [int(p) for p in args.prompts.split(",")]:
                tmax = -(-(P + N) // 64) * 64
                rows = B * cfg.num_key_value_heads * tmax * cfg.num_hidden_layers
                hd = cfg.hidden_size // cfg.num_attention_heads
                need = {"bf16": 2 * rows * hd * 2, "fp8": 2 * rows * (hd + 4)}
                # the prefill's activations (decode.py: B * P x intermediate_size bf16, + twice that for gate | up) and some room
                act = 3 * B * P * cfg.intermediate_size * 2 + 6 * B * P * cfg.hidden_size * 2 + (2 << 30)
                free = torch.cuda.mem_get_info()[0]
                rec = {"workload": f"{args.layers}-layer LM of Vicuna-7B geometry, bf16 activations, {N} new tokens, hipGraph replay of the decode step",
                       "weights": w, "B": B, "P": P, "cache_slots": tmax, "kv_bytes_per_state": need,
                       "bf16_leg_attention": "one-wave" if decs["bf16"]._attn_route(tmax) == "single" else "split"}
                if sum(need.values()) + act > free:
                    rec["skipped"] = f"both states need {sum(need.values()) / 2 ** 30:.1f} GiB of K/V + {act / 2 ** 30:.1f} GiB to prefill, {free / 2 ** 30:.1f} GiB free"
                    emit(rec)
                    continue
                emb = (torch.randn(B, P, cfg.hidden_size, generator=g, device=dev) * 0.5).bfloat16()
                ids, sts = {}, {}
                for k, d in decs.items():
                    ids[k] = d.generate(emb, N)
                    sts[k] = next(reversed(d.graphs.values()))
                    assert kv_bytes(sts[k]) == need[k], (k, kv_bytes(sts[k]), need[k])
                assert sts["fp8"]["attn"] == "split_fp8"
                del emb
                pairs = [{k: replay_ms(sts[k], P, N - 1) for k in ("bf16", "fp8")} for _ in range(args.pairs)]
                ratios = [p["fp8"] / p["bf16"] for p in pairs]
                med = {k: statistics.median(p[k] for p in pairs) for k in ("bf16", "fp8")}
                rec.update({"ms_per_token": {k: round(v, 4) for k, v in med.items()}, "pairs": [{k: round(v, 4) for k, v in p.items()} for p in pairs],
                            "fp8_over_bf16": {"median": round(statistics.median(ratios), 4), "min": round(min(ratios), 4), "max": round(max(ratios), 4)},
                            "greedy_ids_agree": round(float((ids["fp8"] == ids["bf16"]).float().mean()), 4)})
                emit(rec)
                for d in decs.values():      # the caches of this shape go before the next one is built
                    for st in d.graphs.values():
                        st.clear()
                    d.graphs.clear()
                del sts
                torch.cuda.empty_cache()
        del decs
        torch.cuda.empty_cache()
    print(json.dumps({"summary": [{k: r.get(k) for k in ("weights", "B", "P", "ms_per_token", "fp8_over_bf16", "skipped") if k in r} for r in lines]}))


if __name__ == "__main__":
    main()
