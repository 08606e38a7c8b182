#!/usr/bin/env python3
"""Reduce the kernel statistics of one leg of the C5 micro-batch to the families profiles/train_lm_bench.json records.
    rocprofv3 --kernel-trace --stats -d DIR -o leg --output-format csv -- python tools/train_bench.py 4 --train-lm {hf,own} --no-profile
    python tools/train_lm_trace.py DIR/.../leg_kernel_stats.csv [MICRO_BATCHES=12]      prints one JSON object
    python tools/train_lm_trace.py --record AB.json HF_kernel_stats.csv OWN_kernel_stats.csv OUT.json
        AB.json = what `tools/train_bench.py 4 --ab-train-lm 3 --json AB.json` wrote; OUT.json = the record profiles/train_lm_bench.json
(train_bench.py runs 4 warm-up and 8 timed micro-batches: 12 per process).  The language model's share is stated as a lower bound from the
kernels that can only be its own: under "own" the vtgb_gemm_train launches that read a bf16 weight (the frozen projections: the Q-Former's and
the adapters' weights are fp32) plus the kernels of train_llm.hip; under "hf" the hipBLASLt / rocBLAS kernels (the prefix graph calls none).
Adapter GEMMs and torch elementwise kernels come on top in both legs and are not attributed."""
import csv
import json
import re
import sys

FAMILIES = ("own training GEMM (tg_*)", "own LLM training kernels (train_llm.hip)", "own other training kernels",
            "own inference kernels (frozen ViT-g ...)", "hipBLASLt / rocBLAS (Cijk_*)", "torch: other")


def family(k: str) -> str:
    if any(x in k for x in ("tg_mfma_kernel", "tg_f32_kernel", "tg_split_reduce")):
        return FAMILIES[0]
    if any(x in k for x in ("rmsnorm_train", "rope_train", "swiglu_train", "attn_causal")):
        return FAMILIES[1]
    if any(x in k for x in ("attn_train", "ln_train", "gelu_fwd", "gelu_bwd", "col_sum", "ce_rows", "ce_reduce", "ce_backward", "concat_text_io")):
        return FAMILIES[2]
    if any(x in k for x in ("gemm_bf16", "attn_bf16", "layernorm_kernel", "gemm_skinny", "vit_", "pool_", "qformer")):
        return FAMILIES[3]
    if "Cijk_" in k:
        return FAMILIES[4]
    return FAMILIES[5]


def reduce(path: str, micro_batches: int = 12) -> dict:
    ms = dict.fromkeys(FAMILIES, 0.0)
    top, frozen = [], 0.0
    for r in csv.DictReader(open(path)):
        k, t = r["Name"], float(r["TotalDurationNs"]) / 1e6
        ms[family(k)] += t
        top.append((t, int(r["Calls"]), k[:120]))
        m = re.search(r"tg_mfma_kernel<(\w+), (\w+), (\w+), (\w+)>", k)      # <a k-major, a fp32, b k-major, b fp32>: b = the weight
        if m and m.group(2) == "true" and m.group(4) == "false":
            frozen += t
    tot = sum(ms.values())
    llm = frozen + ms[FAMILIES[1]] + ms[FAMILIES[4]]
    top.sort(reverse=True)
    return {"device_ms_per_micro_batch": round(tot / micro_batches, 1),
            "ms_per_micro_batch_by_family": {k: round(v / micro_batches, 1) for k, v in ms.items()},
            "share_by_family": {k: round(v / tot, 4) for k, v in ms.items()},
            "frozen_weight_gemm_ms_per_micro_batch": round(frozen / micro_batches, 1),
            "llm_share_at_least": round(llm / tot, 3),
            "top_kernels_ms_of_all_micro_batches": [dict(ms=round(t, 1), calls=c, name=n) for t, c, n in top[:14]]}


if __name__ == "__main__":
    if sys.argv[1] == "--record":
        rec = json.load(open(sys.argv[2]))
        rec["how"] = ("timings: tools/train_bench.py 4 --ab-train-lm 3 (both values of train_lm alternated for three rounds in one process, 8 micro-batches per "
                      "timing); kernel_trace: rocprofv3 --kernel-trace --stats of tools/train_bench.py 4 --train-lm LEG --no-profile, each leg in a run of "
                      "its own, reduced by tools/train_lm_trace.py")
        rec["kernel_trace"] = {"hf": reduce(sys.argv[3]), "own": reduce(sys.argv[4])}
        with open(sys.argv[5], "w") as f:
            json.dump(rec, f, indent=1)
        sys.exit(0)
    print(json.dumps(reduce(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 12), indent=1))
