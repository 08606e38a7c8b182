#!/usr/bin/env python3
"""sha256 digests of the split-KV decode attention's outputs and pass-1 workspaces, on small shapes chosen for where pass 1 can go wrong.

    python tools/decode_attention_bits.py [--out tests/golden/decode_attention_bits.json] [--commit HASH]

Uses only the public ops API (decode_attention(split=True), decode_attention_fp8, decode_attention_beam), so the same file runs on any
commit: tests/golden/decode_attention_bits.json was recorded with it at 08a9d4e (three copies of pass 1: bf16 / fp32 cache, fp8 cache, beam
gather) on an MI355X, and tests/test_gpu_decode_attention_bits.py asks every later kernel for the same bits.
Inputs: torch.randn from a CPU generator seeded by the geometry, cast, then moved to the device; fp8 codes and scales are
ops.quantize_fp8_kv of the bf16 draw.  Per case two digests: "out", and "ws", the workspace, allocated with torch.zeros and exactly
decode_attention_workspace_bytes -- pass 1 writes only the chunks it visits, so the digest pins m, l, O and their layout.  Before each call
every slot the contract calls unread holds NaN (fp8: the e4m3 NaN code and a NaN scale): the slots past pos, masked slots, the prompt cache
from n_prompt on, the generated cache behind the step (table entries there: 1 << 20).  The beam "pads" cases mask min(3 + 4 b, n_prompt - 1)
leading prompt keys of item b: none at n_prompt = 1, where they run the MASKED kernels under a key_valid of all ones and so repeat the digests
of the "plain" cases (36 of the 240 beam cases; the test asserts that equality)."""
import argparse
import functools
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import torch  # noqa: E402

HEADS = [(4, 4), (8, 2), (12, 1)]       # (nq, nkv); 12 / 1: one full block of 8 query heads and one partial block of 4
HDS = [64, 128]
B = 2
# split and fp8 entries: three chunks, the last one a single wave
TMAX = 576
POSITIONS = [0, 63, 64, 255, 256, 300, 575]
PADS = 5                                # leading pads of row 0 under a key_valid
CHUNK0_MASKED_AT = 300                  # at this pos row 1's key_valid also masks keys 0 .. 255: pass 2 skips a chunk with m = -inf
BLIND_AT = 300                          # the case with row 1 fully masked
# beam entry: (tmax_p, n_prompt, steps); 250: the generated keys cross the 256-key boundary between step 5 and step 6
BEAMS = 3
TMAX_G = 64
BEAM_CASES = [(64, 1, (0, 1, 63)), (256, 250, (0, 5, 6, 63)), (256, 256, (0, 1, 63))]
E4M3_NAN = 0x7F
NAN = float("nan")


def groups():
    """[(entry, dtype name, nq, nkv, hd)]: one input draw each"""
    res = []
    for nq, nkv in HEADS:
        for hd in HDS:
            res += [("split", "bf16", nq, nkv, hd), ("split", "f32", nq, nkv, hd), ("fp8", "bf16", nq, nkv, hd), ("beam", "bf16", nq, nkv, hd),
                    ("beam", "f32", nq, nkv, hd)]
    return res


def group_name(entry, dt, nq, nkv, hd):
    return f"{entry}_{dt}_nq{nq}_nkv{nkv}_hd{hd}"


def group_cases(entry):
    """the case suffixes of one group, in the order they run"""
    if entry == "beam":
        return [f"P{tp}_n{n}_s{s}_{m}" for tp, n, steps in BEAM_CASES for s in steps for m in ("plain", "pads")]
    return [f"pos{p}_{m}" for p in POSITIONS for m in ("plain", "pads")] + [f"pos{BLIND_AT}_blind"]


def case_names():
    return [f"{group_name(*g)}_{c}" for g in groups() for c in group_cases(g[0])]


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def _dtype(dt):
    return torch.bfloat16 if dt == "bf16" else torch.float32


@functools.lru_cache(maxsize=None)
def _draw(dt, nq, nkv, hd, rows, lens):
    """q [rows, nq * hd] and one [n, nkv, t, hd] tensor per (n, t) of ``lens``, on the CPU"""
    g = torch.Generator().manual_seed(100000 * nq + 1000 * nkv + hd + 7 * rows)
    return tuple(torch.randn(*shape, generator=g).to(_dtype(dt)) for shape in [(rows, nq * hd)] + [(n, nkv, t, hd) for n, t in lens])


def _call(fn, dev, rows, nq, hd, tmax):
    """out and the workspace digests of one call: fn(out=..., workspace=...)"""
    from videotgb_amd import ops
    ws = torch.zeros(ops.decode_attention_workspace_bytes(rows, nq, hd, tmax), dtype=torch.uint8, device=dev)
    out = fn(workspace=ws)
    return out, {"out": _sha(out), "ws": _sha(ws)}


def _key_valid(kind, pos, dev):
    if kind == "plain":
        return None
    kv = torch.ones(B, TMAX, dtype=torch.uint8, device=dev)
    kv[0, :PADS] = 0
    if kind == "blind":
        kv[1] = 0
    elif pos == CHUNK0_MASKED_AT:
        kv[1, :256] = 0
    return kv


def _split_group(entry, dt, nq, nkv, hd, dev):
    from videotgb_amd import ops
    q, k, v = (t.to(dev) for t in _draw("bf16" if entry == "fp8" else dt, nq, nkv, hd, B, ((B, TMAX), (B, TMAX))))
    if entry == "fp8":
        (k8, ks), (v8, vs) = ops.quantize_fp8_kv(k), ops.quantize_fp8_kv(v)
        k8, v8 = k8.view(torch.uint8).contiguous(), v8.view(torch.uint8).contiguous()
    res = {}
    for name in group_cases(entry):
        pos, kind = int(name.split("_")[0][3:]), name.split("_")[1]
        kv = _key_valid(kind, pos, dev)
        bad = torch.zeros(B, TMAX, dtype=torch.bool, device=dev)
        bad[:, pos + 1:] = True
        if kv is not None:
            bad |= kv == 0
        bad = bad[:, None, :].expand(B, nkv, TMAX)
        post = torch.tensor([pos], device=dev)
        if entry == "fp8":
            a, b, c, d = k8.clone(), v8.clone(), ks.clone(), vs.clone()
            a[bad], b[bad], c[bad], d[bad] = E4M3_NAN, E4M3_NAN, NAN, NAN
            fn = functools.partial(ops.decode_attention_fp8, q, a, b, c, d, post, float(hd) ** -0.5, key_valid=kv)
        else:
            a, b = k.clone(), v.clone()
            a[bad], b[bad] = NAN, NAN
            fn = functools.partial(ops.decode_attention, q, a, b, post, float(hd) ** -0.5, key_valid=kv, split=True)
        out, res[name] = _call(fn, dev, B, nq, hd, TMAX)
        assert bool(torch.isfinite(out).all()), (entry, dt, nq, nkv, hd, name, "an unread slot reached the output")
        if kind == "blind":
            assert not bool(out[1].any()) and bool(out[0].any()), (entry, dt, nq, nkv, hd, name, "a row without a visible key is a zero row")
    return res


def _beam_group(dt, nq, nkv, hd, dev):
    from videotgb_amd import ops
    R = B * BEAMS
    res = {}
    for tmax_p, n_prompt, steps in BEAM_CASES:
        q, kp, vp, kg, vg = (t.to(dev) for t in _draw(dt, nq, nkv, hd, R, ((B, tmax_p), (B, tmax_p), (R, TMAX_G), (R, TMAX_G))))
        g = torch.Generator().manual_seed(31 * tmax_p + n_prompt)
        perm = torch.stack([torch.stack([torch.randperm(BEAMS, generator=g) for _ in range(TMAX_G)], 1) for _ in range(B)])      # [B, K, tmax_g]
        src = (perm + (torch.arange(B) * BEAMS)[:, None, None]).reshape(R, TMAX_G).int().contiguous().to(dev)      # rows permuted inside an item, per slot
        for step in steps:
            for kind in ("plain", "pads"):
                kv = None
                if kind == "pads":      # leading pads, another count per item
                    kv = torch.ones(B, tmax_p, dtype=torch.uint8, device=dev)
                    for b in range(B):
                        kv[b, : min(3 + 4 * b, n_prompt - 1)] = 0
                kp2, vp2, kg2, vg2, src2 = kp.clone(), vp.clone(), kg.clone(), vg.clone(), src.clone()
                for t in (kp2, vp2):
                    t[:, :, n_prompt:] = NAN
                    if kv is not None:
                        t.masked_fill_((kv == 0)[:, None, :, None], NAN)
                for t in (kg2, vg2):
                    t[:, :, step + 1:] = NAN
                src2[:, step + 1:] = 1 << 20
                fn = functools.partial(ops.decode_attention_beam, q, kp2, vp2, kg2, vg2, src2, torch.tensor([n_prompt], device=dev),
                                       torch.tensor([n_prompt + step], device=dev), float(hd) ** -0.5, key_valid=kv)
                name = f"P{tmax_p}_n{n_prompt}_s{step}_{kind}"
                out, res[name] = _call(fn, dev, R, nq, hd, tmax_p + TMAX_G)
                assert bool(torch.isfinite(out).all()), ("beam", dt, nq, nkv, hd, name, "an unread slot reached the output")
    return res


def digests(dev):
    """{case: {"out" | "ws": sha256}}; raises AssertionError where an unread slot's NaN reaches an output."""
    res = {}
    for entry, dt, nq, nkv, hd in groups():
        per = _beam_group(dt, nq, nkv, hd, dev) if entry == "beam" else _split_group(entry, dt, nq, nkv, hd, dev)
        assert list(per) == group_cases(entry)
        res.update({f"{group_name(entry, dt, nq, nkv, hd)}_{c}": d for c, d in per.items()})
    torch.cuda.synchronize()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="write the JSON here (default: stdout)")
    ap.add_argument("--commit", default=None, help="recorded in the file: the commit the digests were taken at")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_attention_bits needs a GPU")
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
