#!/usr/bin/env python3
"""What a window buys: wld_run_chunks over the whole linkage-block set at
BASELINE config 4's size (20,000 sites x 2,000 sequences, r2 > 0.05), without
a window and under max_sites K, warm, timed on the host around each call.

    python tools/window_bench.py run --sites K --cache FILE --out FILE   one K (0: no window); one JSON line
    python tools/window_bench.py summary FILE...                          the table, and the check

Each run is a process of its own (tools/window_bench.sh gives each its own
time limit); the first one builds the alignment and leaves it in --cache.
The summary prints per run ms/step, tiles, pairs, rows and ms per 1,000
tiles against the unwindowed run's, and fails unless every windowed step is
faster than the unwindowed one.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
L, N, THR, STEPS, WARMUP = 20000, 2000, 0.05, 20, 3


def run(args):
    import bench
    import weightedld_amd as W
    if args.cache and os.path.exists(args.cache):
        z = np.load(args.cache)
        buf, w = z["buf"], z["w"]
    else:
        buf = bench.ld_blocks(L, N)
        w = W.henikoff_weights(W.SiteSet.from_buffer(buf))
        if args.cache:
            np.savez(args.cache, buf=buf, w=w)
    ctx = W.Context(0)
    ctx.load(buf, w)
    ctx.set_window(max_sites=args.sites)
    for _ in range(WARMUP):
        rows = ctx.run_chunks(THR)
    t = []
    for _ in range(STEPS):
        t0 = time.perf_counter()
        n = ctx.run_chunks(THR)
        t.append((time.perf_counter() - t0) * 1e3)
        assert n == rows
    st = ctx.stats()
    rec = {"max_sites": args.sites, "ms_per_step": float(np.median(t)), "ms_min": min(t), "ms_max": max(t),
           "tiles": st["tiles"], "pairs": st["pairs"], "rows": st["rows"], "screened": st["screened"],
           "pair_kernel_ms": st["pair_kernel_ms"], "order_ms": st["order_ms"], "steps": STEPS}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


def summary(args):
    recs = [json.loads(open(p).read()) for p in args.files]
    base = next(r for r in recs if r["max_sites"] == 0)
    per_tile0 = base["ms_per_step"] / base["tiles"]
    print("%9s %10s %9s %13s %9s %14s %9s" % ("max_sites", "ms/step", "tiles", "pairs", "rows", "ms/1000 tiles", "x base"))
    ok = True
    for r in recs:
        per_tile = r["ms_per_step"] / r["tiles"]
        print("%9d %10.4f %9d %13d %9d %14.4f %9.2f" % (r["max_sites"], r["ms_per_step"], r["tiles"], r["pairs"],
                                                        r["rows"], 1e3 * per_tile, per_tile / per_tile0))
        if r["max_sites"] and not r["ms_per_step"] < base["ms_per_step"]:
            ok = False
            print("  ^ not faster than the unwindowed step (%.4f ms)" % base["ms_per_step"])
    return 0 if ok else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("run")
    a.add_argument("--sites", type=int, default=0)
    a.add_argument("--cache")
    a.add_argument("--out")
    b = sub.add_parser("summary")
    b.add_argument("files", nargs="+")
    ns = ap.parse_args()
    sys.exit(run(ns) if ns.cmd == "run" else summary(ns))
