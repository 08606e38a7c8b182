#!/usr/bin/env python3
"""The graph decoder with and without LoRA adapters, and HF generate over the LoraLinear model: same process, same box.

    python tools/lora_decode_bench.py [--layers 32] [--batches 1,124] [--prompt 52] [--new-tokens 64] [--pairs 3] [--out FILE]

A random-init language model of Vicuna-7B geometry (--layers of its 32 layers; llm.build_llama), bf16.  The adapter-free decoder is built
first (the parent's path: the baseline); then the reference's adapters (train.apply_lora: r = 8, alpha = 32 on q_proj and v_proj, lora_B ~
N(0, 0.02)) wrap the same model and a second decoder is built over it -- both multiply by the same packed base weights.  Per batch size:
  * ms per token of the captured decode step (--new-tokens - 1 replays between two events), --pairs times alternating, medians and the
    with / without ratio with the spread of the pairs;
  * the prefill (generate of ONE token: prefill, head, first pick) of both decoders, median of --pairs alternating runs;
  * HF generate over the LoraLinear model: (time of --new-tokens tokens - time of one token) / (--new-tokens - 1) ms per token.
One JSON line per batch size (--out: appended to FILE too), then a summary line."""
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


def timed_ms(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--batches", default="1,124")
    ap.add_argument("--prompt", type=int, default=52)
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lora_decode_bench needs a GPU")
    from videotgb_amd import llm, train
    from videotgb_amd.decode import GreedyDecoder, lora_state
    dev = torch.device("cuda:0")
    lm = llm.build_llama("vicuna-7b", torch.bfloat16, dev, seed=0, num_hidden_layers=args.layers)
    cfg = lm.config
    N, P = args.new_tokens, args.prompt
    g = torch.Generator(device=dev).manual_seed(5)
    base = GreedyDecoder(lm)
    assert base.lora is None
    train.apply_lora(lm, r=8, lora_alpha=32, lora_dropout=0.1)
    with torch.no_grad():
        for n, p in lm.named_parameters():
            if "lora_B" in n:
                p.normal_(0.0, 0.02, generator=g)
    lm.eval()
    assert lora_state(lm) == "ok"
    lora = GreedyDecoder(lm)
    lora.layers, lora.head_w = base.layers, base.head_w      # one copy of the concatenated base weights serves both legs
    lora._skinny = base._skinny_weights()
    decs = {"without": base, "with": lora}
    adapter_bytes = sum(t.numel() * 4 for segs in lora.lora for _, A, B_, _ in segs for t in (A, B_))
    lines = []

    def emit(rec):
        rec["device"] = torch.cuda.get_device_name(0)
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(rec)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    for B in [int(b) for b in args.batches.split(",")]:
        emb = (torch.randn(B, P, cfg.hidden_size, generator=g, device=dev) * 0.5).bfloat16()
        mask = torch.ones(B, P, dtype=torch.long, device=dev)
        ids, sts = {}, {}
        for k, d in decs.items():
            ids[k] = d.generate(emb, N)
            sts[k] = next(reversed(d.graphs.values()))
            d.generate(emb, 1)      # (the one-token state of the prefill timing, built outside it)
        pairs = [{k: replay_ms(sts[k], P, N - 1) for k in decs} for _ in range(args.pairs)]
        pre = [{k: timed_ms(lambda d=d: d.generate(emb, 1)) for k, d in decs.items()} for _ in range(args.pairs)]
        ratios = [p["with"] / p["without"] for p in pairs]

        def hf(n):
            return lm.generate(inputs_embeds=emb, attention_mask=mask, do_sample=False, max_new_tokens=n, min_new_tokens=n, use_cache=True)
        hf(2)      # warm-up
        hf_1, hf_n = timed_ms(lambda: hf(1)), timed_ms(lambda: hf(N))
        hf_ids = hf(N)
        med = {k: statistics.median(p[k] for p in pairs) for k in decs}
        pmed = {k: statistics.median(p[k] for p in pre) for k in decs}
        emit({"workload": f"{args.layers}-layer LM of Vicuna-7B geometry, bf16, prompt {P}, {N} new tokens; adapters r=8 alpha=32 on q_proj / v_proj "
                          f"({adapter_bytes} bytes of fp32 adapters)", "B": B, "P": P, "new_tokens": N,
              "launches_per_layer": {"without": 10, "with": 12},
              "decode_ms_per_token": {k: round(v, 4) for k, v in med.items()}, "decode_pairs": [{k: round(v, 4) for k, v in p.items()} for p in pairs],
              "with_over_without": {"median": round(statistics.median(ratios), 4), "min": round(min(ratios), 4), "max": round(max(ratios), 4)},
              "prefill_ms": {k: round(v, 3) for k, v in pmed.items()}, "prefill_runs": [{k: round(v, 3) for k, v in p.items()} for p in pre],
              "hf_generate_lora_ms_per_token": round((hf_n - hf_1) / (N - 1), 4), "hf_generate_lora_first_token_ms": round(hf_1, 3),
              "ids_agree_with_hf_generate": round(float((ids["with"] == hf_ids).float().mean()), 4),
              "ids_agree_with_adapter_free": round(float((ids["with"] == ids["without"]).float().mean()), 4)})
        for d in decs.values():
            for st in d.graphs.values():
                st.clear()
            d.graphs.clear()
        del sts, emb
        torch.cuda.empty_cache()
    print(json.dumps({"summary": [{k: r.get(k) for k in ("B", "decode_ms_per_token", "with_over_without", "prefill_ms", "hf_generate_lora_ms_per_token")}
                                  for r in lines]}))


if __name__ == "__main__":
    main()
