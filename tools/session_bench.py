#!/usr/bin/env python3
"""Clip sessions vs independent generate calls: K questions about ONE clip.

    python tools/session_bench.py [--questions K] [--reps R] [--T 96] [--new-tokens 16]

One synthetic clip at the bench's geometry (InstructBLIP-Vicuna-7B + TGB: EVA-ViT-g, Q-Former, BERT-base TGB, RAFT in its default mode
f16c8 at T = 96 flow frames, 32 candidate frames, 8 selected), a 4-layer language model of Vicuna-7B width (as tests/test_gpu_scale.py),
bf16 stages, greedy decode of 16 new tokens on the graph decoder (min_new_tokens = max_new_tokens: every question decodes the same number
of steps).  K questions of different token lengths are answered two ways:

  generate   K independent model.generate(frames, flow_frames, ...) calls (RAFT, TGB, ViT-g over the selected frames every time);
  session    one model.clip_session(frames, flow_frames) and K sess.generate(...) calls; the first question's time includes building the
             session (RAFT + the TGB trunk).

Both ways run once untimed first (graph captures per prompt length, workspaces), then R timed passes; every number is the median over
the passes.  Prints one JSON line: ms per question (generate; session first question; session questions 2..K), the ratio of a later
session question to a generate call, the speed-up of the whole K-question pass, RAFT calls and ViT frames encoded per pass."""
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


class BE(dict):
    __getattr__ = dict.__getitem__


def build(dev):
    from videotgb_amd import llm, models, synth
    cfg = synth.full_cfg("instructblip")
    lm = llm.build_llama("vicuna-7b", torch.bfloat16, dev, seed=0, num_hidden_layers=4)
    m = models.LSTP(cfg, dev, language_model=lm, compute_dtype="bf16")
    m.load_state_dict(synth.path_state_dict(cfg, seed=0, with_raft=True), strict=False)
    m.to(dev)
    return m, cfg


def make_questions(cfg, dev, K, T, seed=7):
    """K questions of different lengths: (text_encoding, sampler_text_encoding, Gumbel noise)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    out = []
    for i in range(K):
        ls, lp, lq = 8 + (3 * i) % 13, 14 + (5 * i) % 17, 8 + (4 * i) % 11
        sids = torch.randint(3, cfg.tgb.vocab, (1, ls), generator=g, device=dev)
        pids = torch.randint(3, 32000, (1, lp), generator=g, device=dev)
        qids = torch.randint(3, cfg.qformer.vocab, (1, lq), generator=g, device=dev)
        te = BE(input_ids=pids, attention_mask=torch.ones_like(pids), qformer_input_ids=qids, qformer_attention_mask=torch.ones_like(qids))
        se = BE(input_ids=sids, attention_mask=torch.ones_like(sids))
        out.append((te, se, -torch.empty(2, 2, T, device=dev).exponential_(generator=g).log()))
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--questions", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--T", type=int, default=96)
    ap.add_argument("--new-tokens", type=int, default=16)
    ap.add_argument("--nframe", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("session_bench needs a GPU")
    dev = torch.device("cuda:0")
    K, T, N, nframe = args.questions, args.T, 32, args.nframe
    if K < 2:
        ap.error("--questions must be at least 2")
    m, cfg = build(dev)
    g = torch.Generator(device=dev).manual_seed(3)
    frames = torch.randn(N, 3, 224, 224, generator=g, device=dev)
    flow_frames = torch.rand(1, T, 3, 224, 224, generator=g, device=dev) * 255
    qs = make_questions(cfg, dev, K, T)
    kw = dict(do_sample=False, temperature=None, max_new_tokens=args.new_tokens, min_new_tokens=args.new_tokens, fast_decode="auto")

    counts = {"raft": 0, "vit_frames": 0}
    raft_fwd, vit_fwd = m.of_extractor.forward_clips, m.model.vision_model.forward

    def raft_counted(x, *a, **k):
        counts["raft"] += 1
        return raft_fwd(x, *a, **k)

    def vit_counted(pixel_values=None, *a, **k):
        counts["vit_frames"] += pixel_values.shape[0]
        return vit_fwd(pixel_values, *a, **k)

    m.of_extractor.forward_clips = raft_counted
    m.model.vision_model.forward = vit_counted

    def generate_pass():
        counts.update(raft=0, vit_frames=0)
        ms, ids = [], []
        for te, se, noise in qs:
            t, (out, _) = timed(lambda: m.generate(frames, flow_frames, nframe, te, se, noise=noise, **kw))
            ms.append(t)
            ids.append(out)
        return ms, ids, dict(counts)

    def session_pass():
        counts.update(raft=0, vit_frames=0)
        ms, ids = [], []
        sess = None
        for i, (te, se, noise) in enumerate(qs):
            def one():
                nonlocal sess
                if sess is None:
                    sess = m.clip_session(frames, flow_frames)
                return sess.generate(nframe, te, se, noise=noise, **kw)
            t, (out, _) = timed(one)
            ms.append(t)
            ids.append(out)
        return ms, ids, dict(counts)

    _, ref_ids, _ = generate_pass()                      # untimed: graph captures, workspaces
    session_pass()
    gen_q, s_first, s_later, gen_total, s_total = [], [], [], [], []
    same = True
    for _ in range(args.reps):
        ms, ids_g, c_gen = generate_pass()
        gen_q.append(statistics.mean(ms))
        gen_total.append(sum(ms))
        ms, ids_s, c_sess = session_pass()
        s_first.append(ms[0])
        s_later.append(statistics.mean(ms[1:]))
        s_total.append(sum(ms))
        same = same and all(torch.equal(a, b) for a, b in zip(ids_g, ids_s)) and all(torch.equal(a, b) for a, b in zip(ids_g, ref_ids))
    med = statistics.median
    out = {
        "workload": f"one clip, {K} questions: InstructBLIP-Vicuna-7B geometry (4-layer LM), TGB BERT-base, RAFT f16c8, T={T}, N={N}, "
                    f"nframe={nframe}, bf16, greedy {args.new_tokens} tokens",
        "generate_ms_per_question": round(med(gen_q), 2),
        "session_first_question_ms": round(med(s_first), 2),
        "session_later_question_ms": round(med(s_later), 2),
        "later_over_generate": round(med(s_later) / med(gen_q), 3),
        "speedup_k_questions": round(med(gen_total) / med(s_total), 3),
        "raft_calls": {"generate": c_gen["raft"], "session": c_sess["raft"]},
        "vit_frames_encoded": {"generate": c_gen["vit_frames"], "session": c_sess["vit_frames"]},
        "ids_equal": bool(same),
        "reps": args.reps,
        "device": torch.cuda.get_device_name(0),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
