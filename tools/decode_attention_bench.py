#!/usr/bin/env python3
"""Kernel-level A/B timing of the split-KV decode attention entries between two builds of libvtgb.so.

    python tools/decode_attention_bench.py --parent-lib PATH/libvtgb.so [--new-lib videotgb_amd/libvtgb.so] [--pairs 3] [--only PREFIX] [--out FILE]

Public ops API only (decode_attention(split=True), decode_attention_fp8, decode_attention_beam); the library is the one VTGB_LIB names.
The driver starts one fresh child process per leg, one at a time, each under its own ``timeout``, and stops at the first leg that fails.
Legs alternate parent, new, parent, new ...: --pairs of each, and every leg times every shape, so each shape has --pairs times per library
taken minutes apart.  Per shape a leg captures one graph of n >= 8 calls, each over K/V caches of its own, n large enough that the caches
total more than 1 GB (nothing is served from the last-level cache), replays it to warm up, and then times, between two device events, as
many replays as fill at least half a second.  Reported per leg: microseconds per call (pass 1 + pass 2).

Shapes, all bf16, hd 128: split and fp8 at nq / nkv 32 / 32 (Vicuna-7B) and 32 / 8, B in {1, 16}, tmax in {2112, 4096}, pos = tmax - 1;
beam at 4 items x 5 beams, 32 / 32 heads, (tmax_p, tmax_g) in {(64, 64), (2048, 64)} at the last step (prompt = tmax_p - 12 tokens; the
first is the shape of tools/beam_decode_bench.py).
Per shape the spread of the parent's legs, (max - min) / median, is the noise; the new library's median may exceed the parent's by no more
than that.  Writes the raw per-leg times and that comparison to --out (default profiles/decode_attention_pass1_ab.json)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

HD = 128
MIN_BYTES = 1 << 30          # the caches of one graph: more than this
MIN_LAUNCHES = 8
MIN_WINDOW_MS = 500.0
LEG_TIMEOUT_S = 240


def shapes(only=""):
    """[(name, entry, geometry)] of the shapes whose name starts with ``only``"""
    return [s for s in _all_shapes() if s[0].startswith(only)]


def _all_shapes():
    res = []
    for entry in ("split", "fp8"):
        for nq, nkv in ((32, 32), (32, 8)):
            for B in (1, 16):
                for tmax in (2112, 4096):
                    res.append((f"{entry}_nq{nq}_nkv{nkv}_B{B}_t{tmax}", entry, dict(nq=nq, nkv=nkv, B=B, tmax=tmax)))
    for tmax_p in (64, 2048):
        res.append((f"beam_nq32_nkv32_B4_K5_P{tmax_p}_G64", "beam", dict(nq=32, nkv=32, B=4, K=5, tmax_p=tmax_p, tmax_g=64)))
    return res


def _calls(entry, p, dev):
    """n closures, each one call of the entry over caches of its own"""
    import torch
    from videotgb_amd import ops
    bf = torch.bfloat16
    scale = HD ** -0.5
    nq, nkv, B = p["nq"], p["nkv"], p["B"]
    if entry == "beam":
        K, tp, tg = p["K"], p["tmax_p"], p["tmax_g"]
        R = B * K
        per = 2 * (B * tp + R * tg) * nkv * HD * 2
    else:
        R, tmax = B, p["tmax"]
        per = 2 * B * nkv * tmax * HD * (1 if entry == "fp8" else 2)
    n = max(MIN_LAUNCHES, MIN_BYTES // per + 1)
    q = torch.randn(R, nq * HD, device=dev).to(bf)
    out = torch.empty(R, nq * HD, dtype=bf, device=dev)
    ws = torch.empty(max(16, ops.decode_attention_workspace_bytes(R, nq, HD, tp + tg if entry == "beam" else tmax)), dtype=torch.uint8, device=dev)
    calls = []
    for _ in range(n):
        if entry == "split":
            kc, vc = (torch.randn(B, nkv, tmax, HD, device=dev, dtype=bf) for _ in range(2))
            pos = torch.tensor([tmax - 1], device=dev)
            calls.append(lambda kc=kc, vc=vc, pos=pos: ops.decode_attention(q, kc, vc, pos, scale, out=out, workspace=ws, split=True))
        elif entry == "fp8":
            kc8, vc8 = (torch.randint(0, 0x78, (B, nkv, tmax, HD), device=dev, dtype=torch.uint8) for _ in range(2))      # finite codes
            ks, vs = (torch.full((B, nkv, tmax), 2.0 ** -6, device=dev) for _ in range(2))
            pos = torch.tensor([tmax - 1], device=dev)
            calls.append(lambda kc8=kc8, vc8=vc8, ks=ks, vs=vs, pos=pos: ops.decode_attention_fp8(q, kc8, vc8, ks, vs, pos, scale, out=out, workspace=ws))
        else:
            kp, vp = (torch.randn(B, nkv, tp, HD, device=dev, dtype=bf) for _ in range(2))
            kg, vg = (torch.randn(R, nkv, tg, HD, device=dev, dtype=bf) for _ in range(2))
            perm = torch.stack([torch.stack([torch.randperm(K, device=dev) for _ in range(tg)], 1) for _ in range(B)])      # [B, K, tmax_g]
            src = (perm + (torch.arange(B, device=dev) * K)[:, None, None]).reshape(R, tg).int().contiguous()
            n_prompt = torch.tensor([tp - 12], device=dev)
            pos = torch.tensor([tp - 12 + tg - 1], device=dev)
            calls.append(lambda kp=kp, vp=vp, kg=kg, vg=vg, src=src, n_prompt=n_prompt, pos=pos:
                         ops.decode_attention_beam(q, kp, vp, kg, vg, src, n_prompt, pos, scale, out=out, workspace=ws))
    return calls


def leg(only):
    """every shape once, with the library VTGB_LIB names: prints one JSON line {shape: microseconds per call}"""
    import torch
    if not torch.cuda.is_available():
        sys.exit("decode_attention_bench needs a GPU")
    from videotgb_amd import _lib
    _lib.lib()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    res = {}
    for name, entry, p in shapes(only):
        calls = _calls(entry, p, dev)
        for c in calls[:2]:      # outside the capture first: errors surface here
            c()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for c in calls:
                c()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(3):
            graph.replay()
        reps, ms = 4, 0.0
        while ms < MIN_WINDOW_MS:      # (the first, short windows only size the timed one)
            reps = reps if ms == 0.0 else int(reps * MIN_WINDOW_MS * 1.2 / ms) + 1
            e0.record()
            for _ in range(reps):
                graph.replay()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
        res[name] = ms * 1e3 / (reps * len(calls))
        print(f"  {name}: {res[name]:.2f} us per call ({len(calls)} calls per graph, {reps} replays, {ms:.0f} ms)", file=sys.stderr, flush=True)
        del graph, calls
        torch.cuda.empty_cache()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "us_per_call": res}))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--leg", action="store_true", help="(what the driver starts) time every shape once in this process")
    ap.add_argument("--parent-lib", help="libvtgb.so built from the parent commit")
    ap.add_argument("--new-lib", default=os.path.join(REPO, "videotgb_amd", "libvtgb.so"))
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--only", default="", help="only the shapes whose name starts with this, e.g. split_ or fp8_nq32_nkv8")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "decode_attention_pass1_ab.json"))
    args = ap.parse_args()
    if args.leg:
        return leg(args.only)
    if not args.parent_lib:
        ap.error("--parent-lib is required")
    libs = {"parent": os.path.abspath(args.parent_lib), "new": os.path.abspath(args.new_lib)}
    legs = []
    for i in range(args.pairs):
        for which in ("parent", "new"):
            env = dict(os.environ, VTGB_LIB=libs[which])
            p = subprocess.run(["timeout", "-k", "10", str(LEG_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--leg", "--only", args.only],
                               env=env,
                               stdout=subprocess.PIPE, text=True)
            if p.returncode != 0:
                sys.exit(f"leg {len(legs)} ({which}) failed with status {p.returncode}: stopping")
            legs.append({"lib": which, "pair": i, **json.loads(p.stdout.strip().splitlines()[-1])})
            print(f"leg {len(legs)} ({which}) done", flush=True)
    doc = {"method": f"graph of >= {MIN_LAUNCHES} calls over distinct caches (> 1 GiB in all), >= {MIN_WINDOW_MS:.0f} ms of replays between device events; "
                     "us per call = pass 1 + pass 2", "legs": legs, "shapes": {}}
    over = []
    for name, _, _ in shapes(args.only):
        t = {w: [l["us_per_call"][name] for l in legs if l["lib"] == w] for w in libs}
        mp, mn = statistics.median(t["parent"]), statistics.median(t["new"])
        noise = (max(t["parent"]) - min(t["parent"])) / mp
        doc["shapes"][name] = {"parent_us": [round(v, 3) for v in t["parent"]], "new_us": [round(v, 3) for v in t["new"]],
                               "parent_median_us": round(mp, 3), "new_median_us": round(mn, 3), "parent_spread": round(noise, 5),
                               "new_over_parent": round(mn / mp - 1.0, 5), "within_parent_spread": bool(mn / mp - 1.0 <= noise)}
        if mn / mp - 1.0 > noise:
            over.append(name)
        print(f"{name}: parent {mp:.2f} us, new {mn:.2f} us ({(mn / mp - 1) * 100:+.2f} %), parent spread {noise * 100:.2f} %")
    doc["slower_than_the_parent_spread_allows"] = over
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print("slower than the parent's spread allows: " + (", ".join(over) if over else "none"))


if __name__ == "__main__":
    main()
