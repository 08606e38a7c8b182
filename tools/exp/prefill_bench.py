"""f2 prefill at the bench's shapes (Vicuna-7B, B clips x P prefix+prompt tokens): libvtgb (vtgb_gemm + vtgb_attention /
vtgb_attention_tiled + vtgb_llm_*) against F.linear (hipBLASLt) + SDPA, same weights, both in one process with the pairs alternated.
Usage: python tools/exp/prefill_bench.py [B] [P] [N] [--json FILE]    (a P = 384 row -- past the single-pass attention kernel's 288
tokens -- is printed as well)"""
import json, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from videotgb_amd import llm
from videotgb_amd.decode import GreedyDecoder

argv = list(sys.argv[1:])
out_json = argv.pop(argv.index("--json") + 1) if "--json" in argv else None
argv = [a for a in argv if a != "--json"]
B = int(argv[0]) if len(argv) > 0 else 124
P = int(argv[1]) if len(argv) > 1 else 52
N = int(argv[2]) if len(argv) > 2 else 16
dev = "cuda:0"
lm = llm.build_llama("vicuna-7b", torch.bfloat16, dev, seed=0)
rows = []
for p in dict.fromkeys((P, 384)):
    emb = (torch.randn(B, p, lm.config.hidden_size, device=dev) * 0.02).bfloat16()
    for name, maxtok in (("libvtgb", GreedyDecoder.PREFILL_MAX_TOKENS), ("blas", 0)) * 2:
        dec = GreedyDecoder(lm)
        dec.PREFILL_MAX_TOKENS = maxtok
        assert dec._use_hip_prefill(emb, p) == (name == "libvtgb")
        dec.generate(emb, N)
        for n_new in (1, N):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                ids = dec.generate(emb, n_new)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / 3 * 1e3
            rows.append(dict(path=name, B=B, P=p, new=n_new, ms=round(ms, 2)))
            print(f"{name:8s} B={B} P={p} new={n_new}: {ms:.1f} ms", flush=True)
        del dec
if out_json:
    with open(out_json, "w") as f:
        json.dump(rows, f)
        f.write("\n")
