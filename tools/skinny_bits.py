#!/usr/bin/env python3
"""sha256 digests of ops.gemm_skinny's outputs on small shapes chosen for where the weight-streaming kernel can go wrong.

    python tools/skinny_bits.py [--out tests/golden/skinny_bits.json]

Uses only the public ops API, so the same file runs on any commit: tests/golden/skinny_bits.json was recorded with it at 2f95aae (two kernels,
bf16 and fp8) on an MI355X, and tests/test_gpu_skinny_bits.py asks every later kernel for the same bits.  Inputs: torch.randn from a CPU
generator, cast to bf16, weights scaled by K ** -0.5.  Per case and weight form (row-major bf16, SkinnyWeight, SkinnyWeightFp8): the fp32
output, the bf16 output and, where the case splits K, the fp32 fragments left in the workspace under defer_reduce=True.  Outputs go into a
padded buffer (row pitch = N rounded up to 8) wherever that is wider than N; its pad columns must keep their prefill value."""
import argparse
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import torch  # noqa: E402

# (M, N, K, n_splits)
CASES = [
    (1, 128, 64, 0),        # one k-tile: less than one ring group
    (16, 131, 640, 1),      # x row blocks 1 | 2; 10 k-tiles: past a bf16 ring group, inside an fp8 one, across the x ring's wrap; N % 4 != 0: the
    (17, 131, 640, 1),      # scalar tail store of the unsplit epilogue, into a padded out
    (33, 384, 1088, 0),     # 17 k-tiles: one past an fp8 ring group; 4 x row blocks
    (65, 200, 1088, 3),     # 8 x row blocks; uneven splits of 5 / 6 / 6 k-tiles, each shorter than the ring
    (128, 256, 128, 2),     # all 128 rows; splits of one k-tile
    (5, 100, 128, 5),       # n_splits above the k-tile count: clamped to 2
]
PAD = -7.0                  # prefill of the output buffers


def case_name(M, N, K, S):
    return f"M{M}_N{N}_K{K}_S{S}"


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def _padded_out(M, N, dtype, dev):
    ldo = (N + 7) // 8 * 8
    return torch.full((M, ldo), PAD, dtype=dtype, device=dev)


def digests(dev):
    """{case: {weight form: {"f32" | "bf16" | "parts": sha256}}}; raises AssertionError where a call writes outside out[:, :N]."""
    from videotgb_amd import ops
    res = {}
    for M, N, K, S in CASES:
        g = torch.Generator().manual_seed(1000 * M + N)
        x = torch.randn(M, K, generator=g).bfloat16().to(dev)
        w = (torch.randn(N, K, generator=g) * K ** -0.5).bfloat16().to(dev)
        need = ops.gemm_skinny_workspace_bytes(M, N, K, S)
        forms = {"rowmajor": w, "tiled": ops.SkinnyWeight(w), "fp8": ops.SkinnyWeightFp8(w)}
        res[case_name(M, N, K, S)] = per_case = {}
        for form, wf in forms.items():
            d = {}
            for key, dtype in (("f32", torch.float32), ("bf16", torch.bfloat16)):
                buf = _padded_out(M, N, dtype, dev)
                ops.gemm_skinny(x, wf, out=buf[:, :N], n_splits=S)
                assert bool((buf[:, N:] == PAD).all()), (M, N, K, S, form, key, "pad columns written")
                d[key] = _sha(buf[:, :N])
            if need:
                ws = torch.zeros(need, dtype=torch.uint8, device=dev)
                buf = _padded_out(M, N, torch.bfloat16, dev)
                _, splits, parts = ops.gemm_skinny(x, wf, out=buf[:, :N], n_splits=S, workspace=ws, defer_reduce=True)
                assert splits > 1 and parts is ws
                assert bool((buf == PAD).all()), (M, N, K, S, form, "deferred call wrote out")
                d["parts"] = _sha(ws)
            per_case[form] = d
    torch.cuda.synchronize()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="write the JSON here (default: stdout)")
    ap.add_argument("--commit", default=None, help="recorded in the file: the commit the digests were taken at")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("skinny_bits needs a GPU")
    dev = torch.device("cuda:0")
    doc = {"recorded_at": args.commit, "device": torch.cuda.get_device_name(0), "cases": digests(dev)}
    text = json.dumps(doc, indent=1) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
