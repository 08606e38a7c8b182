#!/usr/bin/env python3
"""Beam search on the T5 graph decoder (beam_search="graph+t5") against HF generate and against the decoder's own greedy step, same process.

    python tools/t5_beam_decode_bench.py [--layers 24] [--batches 1,8] [--beams 5] [--encoder 96] [--new-tokens 64] [--pairs 3] [--out FILE]

A random-init T5ForConditionalGeneration of Flan-T5-XL geometry (d_model 2048, --layers encoder + --layers decoder blocks of its 24 + 24, 32
heads, d_kv 64, d_ff 5120, gated-gelu, vocabulary 32128), bf16.  For every batch size B, three whole calls -- encoder included -- over the
same encoder input of --encoder positions, each asked for exactly --new-tokens tokens (min_new_tokens = max_new_tokens: fixed work):
  graph   T5GreedyDecoder.generate(num_beams=K, repetition_penalty=1.5): the encoder and the cross-attention K | V on B rows, B * K beam
          rows per decoder step, self-attention through the ancestry table (vtgb_llm_attention_rows_beam)
  hf      lm.generate(num_beams=K, repetition_penalty=1.5, ...): the same request on HF generate (beam_search="hf", the behaviour of before)
  greedy  T5GreedyDecoder.generate on B * K rows: the decoder's plain step at the beam rows' batch size (no beam bookkeeping; its encoder
          runs on B * K rows)
After one warm-up call each (graph capture, allocator), --pairs rounds run the three alternately; a call is timed between two
synchronisations on the host clock.  Reported: ms per generated token (call time / new tokens) per round and its median, the ratios
hf / graph and graph / greedy with the spread over the rounds, and whether graph and hf returned the same ids (bf16: recorded, not
gated).  Prints one JSON line and writes it to --out (default profiles/t5_beam_decode_bench.json)."""
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


def build_flan_t5_xl(layers: int, dev, seed: int = 0):
    """Random-init T5ForConditionalGeneration of Flan-T5-XL geometry, created on the device in bf16 (N(0, 0.02) matrices, unit norms)."""
    from transformers import T5Config, T5ForConditionalGeneration
    cfg = T5Config(vocab_size=32128, d_model=2048, d_kv=64, d_ff=5120, num_layers=layers, num_decoder_layers=layers, num_heads=32,
                   feed_forward_proj="gated-gelu", tie_word_embeddings=False, decoder_start_token_id=0, pad_token_id=0, eos_token_id=1)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device(dev):
            lm = T5ForConditionalGeneration(cfg)
    finally:
        torch.set_default_dtype(prev)
    g = torch.Generator(device=dev).manual_seed(seed)
    with torch.no_grad():
        for n, p in lm.named_parameters():
            if p.dim() >= 2:
                p.normal_(0.0, 0.02, generator=g)
            else:
                p.fill_(1.0)      # (T5LayerNorm weights: the model has no biases)
        lm.lm_head.weight.mul_(4.0)      # (N(0, 0.02) leaves near-uniform logits: a wider lm_head and embedding make the beams differ)
        lm.shared.weight.mul_(20.0)
    lm.generation_config.pad_token_id = 0
    return lm.eval()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--beams", type=int, default=5)
    ap.add_argument("--encoder", type=int, default=96)
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "t5_beam_decode_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("t5_beam_decode_bench needs a GPU")
    from videotgb_amd.decode import T5GreedyDecoder
    dev = torch.device("cuda:0")
    lm = build_flan_t5_xl(args.layers, dev)
    dec = T5GreedyDecoder(lm)
    K, P, N = args.beams, args.encoder, args.new_tokens
    out = {"workload": f"{args.layers}+{args.layers}-layer T5 of Flan-T5-XL geometry, bf16, encoder input {P}, {N} new tokens, {K} beams, "
                       "repetition_penalty 1.5; whole calls", "batches": {}}
    g = torch.Generator(device=dev).manual_seed(5)
    for B in [int(b) for b in args.batches.split(",")]:
        emb = (torch.randn(B, P, lm.config.d_model, generator=g, device=dev) * 0.5).bfloat16()
        mask = torch.ones(B, P, dtype=torch.long, device=dev)
        wide = emb.repeat_interleave(K, 0).contiguous()

        def graph():
            return dec.generate(emb, N, eos_token_id=1, pad_token_id=0, min_new_tokens=N, num_beams=K, repetition_penalty=1.5, length_penalty=1.0)

        def hf():
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                return lm.generate(inputs_embeds=emb, attention_mask=mask, do_sample=False, num_beams=K, repetition_penalty=1.5, length_penalty=1.0,
                                   max_new_tokens=N, min_new_tokens=N, eos_token_id=1, pad_token_id=0)

        def greedy():
            return dec.generate(wide, N, eos_token_id=1, pad_token_id=0, min_new_tokens=N)
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
