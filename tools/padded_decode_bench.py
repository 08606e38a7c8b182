#!/usr/bin/env python3
"""Padded prompt batches: the graph decoder vs HF generate, and several questions in one session call.

    python tools/padded_decode_bench.py [--batches 1,8,32,124] [--new-tokens 32] [--reps 5] [--questions 8] [--no-session]

Decoder: a 4-layer language model of Vicuna-7B width (as tools/session_bench.py), bf16, prompts = a 32-token prefix (all ones) | a question
of ragged length 14..30 right-padded to the longest (the tokenizer's padding="longest"), greedy with min_new_tokens = max_new_tokens.
For every batch size, ms per generated token (the call's time, prefill included, over --new-tokens) of
  hf        lm.generate(inputs_embeds=..., attention_mask=...)            (what ran for padded batches before)
  padded    GreedyDecoder.generate(..., attention_mask=...)               (hipGraph replay, masked kernels)
  unpadded  GreedyDecoder.generate(...) on the same embeddings, no mask   (today's path at the same padded length)
Every number is the median of --reps timed calls after one untimed call (graph capture), with min and max.

Session (unless --no-session): the bench geometry clip of tools/session_bench.py, K questions of different lengths answered as K
single-question sess.generate calls vs ONE call with the K questions padded (question, sampler and Q-Former text); ms per question,
median / min / max over --reps passes after an untimed one.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from session_bench import BE, build, make_questions, timed  # noqa: E402


def stats(xs, scale=1.0):
    return {"median": round(statistics.median(xs) * scale, 3), "min": round(min(xs) * scale, 3), "max": round(max(xs) * scale, 3)}


def pad_right(rows, value=0):
    n = max(r.shape[1] for r in rows)
    ids = torch.full((len(rows), n), value, dtype=rows[0].dtype, device=rows[0].device)
    mask = torch.zeros(len(rows), n, dtype=torch.long, device=rows[0].device)
    for i, r in enumerate(rows):
        ids[i, : r.shape[1]], mask[i, : r.shape[1]] = r[0], 1
    return ids, mask


def decoder_bench(dev, batches, N, reps):
    from videotgb_amd import llm
    from videotgb_amd.decode import GreedyDecoder
    lm = llm.build_llama("vicuna-7b", torch.bfloat16, dev, seed=0, num_hidden_layers=4)
    dec = GreedyDecoder(lm)
    g = torch.Generator(device=dev).manual_seed(11)
    out = {}
    for B in batches:
        lens = [14 + (7 * b) % 17 for b in range(B)]
        q, qm = pad_right([torch.randint(3, 32000, (1, n), generator=g, device=dev) for n in lens])
        prefix = torch.randn(B, 32, 4096, generator=g, device=dev).bfloat16() * 0.02
        emb = torch.cat([prefix, lm.get_input_embeddings()(q)], 1)
        am = torch.cat([torch.ones(B, 32, dtype=torch.long, device=dev), qm], 1)
        runs = {
            "hf": lambda: lm.generate(inputs_embeds=emb, attention_mask=am, do_sample=False, max_new_tokens=N, min_new_tokens=N),
            "padded": lambda: dec.generate(emb, N, attention_mask=am),
            "unpadded": lambda: dec.generate(emb, N),
        }
        res, ids = {}, {}
        for name, fn in runs.items():
            _, ids[name] = timed(fn)
            res[name] = [timed(fn)[0] for _ in range(reps)]
        row = {k: stats(v, 1.0 / N) for k, v in res.items()}
        row["padded_over_unpadded"] = round(statistics.median(res["padded"]) / statistics.median(res["unpadded"]), 3)
        row["hf_over_padded"] = round(statistics.median(res["hf"]) / statistics.median(res["padded"]), 2)
        row["padded_ids_equal_hf_first_tokens"] = int((ids["padded"][:, :4] == ids["hf"][:, :4]).all(-1).sum().item())
        row["P"] = emb.shape[1]
        out[str(B)] = row
    return out


def session_bench(dev, K, N, reps, T=96, nframe=8):
    m, cfg = build(dev)
    g = torch.Generator(device=dev).manual_seed(3)
    frames = torch.randn(32, 3, 224, 224, generator=g, device=dev)
    flow_frames = torch.rand(1, T, 3, 224, 224, generator=g, device=dev) * 255
    qs = make_questions(cfg, dev, K, T)
    kw = dict(do_sample=False, temperature=None, max_new_tokens=N, min_new_tokens=N, fast_decode=True)
    ids, mask = pad_right([te["input_ids"] for te, _, _ in qs])
    qids, qmask = pad_right([te["qformer_input_ids"] for te, _, _ in qs])
    sids, smask = pad_right([se["input_ids"] for _, se, _ in qs])
    te_all = BE(input_ids=ids, attention_mask=mask, qformer_input_ids=qids, qformer_attention_mask=qmask)
    se_all = BE(input_ids=sids, attention_mask=smask)
    noise = torch.cat([torch.stack([q[2][:, 0] for q in qs], 1), torch.stack([q[2][:, 1] for q in qs], 1)], 1)
    sess = m.clip_session(frames, flow_frames)

    def singles():
        return [sess.generate(nframe, te, se, noise=nz, **kw) for te, se, nz in qs]

    def one_call():
        return sess.generate(nframe, te_all, se_all, noise=noise, **kw)
    singles()
    one_call()
    t_single = [timed(singles)[0] / K for _ in range(reps)]
    t_one = [timed(one_call)[0] / K for _ in range(reps)]
    return {"questions": K, "single_calls_ms_per_question": stats(t_single), "one_call_ms_per_question": stats(t_one),
            "speedup": round(statistics.median(t_single) / statistics.median(t_one), 2)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batches", default="1,8,32,124")
    ap.add_argument("--new-tokens", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--questions", type=int, default=8)
    ap.add_argument("--no-session", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("padded_decode_bench needs a GPU")
    if args.reps < 1 or args.new_tokens < 1 or args.questions < 2:
        ap.error("--reps >= 1, --new-tokens >= 1, --questions >= 2")
    dev = torch.device("cuda:0")
    batches = [int(b) for b in args.batches.split(",")]
    out = {"workload": f"4-layer LM of Vicuna-7B width, bf16, prefix 32 + right-padded questions of 14..30 tokens, greedy {args.new_tokens} tokens",
           "ms_per_token": decoder_bench(dev, batches, args.new_tokens, args.reps)}
    if not args.no_session:
        out["session"] = session_bench(dev, args.questions, 16, args.reps)
    out.update(reps=args.reps, device=torch.cuda.get_device_name(0))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
