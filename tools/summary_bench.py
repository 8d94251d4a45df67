#!/usr/bin/env python3
"""What the summary's reducing epilogue costs against the row path's
compaction: the summary launch (Context.run_summary's kernel_ms) against the
row path's every-tile reference-order launch (set_option("screen", 0), r2 >
0.05, stats()["pair_kernel_ms"] — bench.py's unscreened_pair_kernel_ms) on
bench.synth(20000, 2000) with Henikoff weights, warm; and end to end,
run_summary against run_host(-1.0) (every pair as a row, copied to the host)
on bench.ld_blocks(5000, 500).

    python tools/summary_bench.py run --what rows|summary|summary_bins|e2e_rows|e2e_summary
                                      [--tree DIR] --cache FILE --out FILE      one measurement; one JSON line
    python tools/summary_bench.py summary FILE...                  the table, and the check

Each run is a process of its own (tools/summary_bench.sh gives each its own
time limit and interleaves the two sides); --tree DIR imports weightedld_amd
(package and built library) from another checkout, so the baseline can be the
parent commit's build on the same device.  The
summary fails unless every summary launch is within 1.10 x the median row
launch.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
L, N, THR, STEPS, WARMUP = 20000, 2000, 0.05, 10, 3
L2, N2 = 5000, 500
BIN_WIDTH, N_BINS = 64, 256


def data(kind, n_sites, n_seqs, cache):
    import bench
    import weightedld_amd as W
    if cache and os.path.exists(cache):
        z = np.load(cache)
        return z["buf"], z["w"]
    buf = getattr(bench, kind)(n_sites, n_seqs)
    w = W.henikoff_weights(W.SiteSet.from_buffer(buf))
    if cache:
        np.savez(cache, buf=buf, w=w)
    return buf, w


def run(args):
    if args.tree:
        sys.path.insert(0, os.path.abspath(args.tree))
    import weightedld_amd as W
    e2e = args.what.startswith("e2e")
    buf, w = data("ld_blocks", L2, N2, args.cache) if e2e else data("synth", L, N, args.cache)
    ctx = W.Context(0)
    ctx.load(buf, w)
    rec = {"what": args.what, "lib": W.LIB_PATH, "sites": int(buf.shape[0]), "seqs": int(buf.shape[1])}
    if args.what == "rows":
        ctx.set_option("screen", 0)
        for _ in range(WARMUP):
            ctx.run_chunks(THR)
        ms = []
        for _ in range(STEPS):
            ctx.run_chunks(THR)
            ms.append(ctx.stats()["pair_kernel_ms"])
        st = ctx.stats()
        rec.update(tiles=st["tiles"], pairs=st["pairs"], rows=st["rows"], ref_sums=st["ref_sums"])
    elif args.what in ("summary", "summary_bins"):
        bins = (BIN_WIDTH, N_BINS) if args.what == "summary_bins" else (0, 0)
        for _ in range(WARMUP):
            ctx.run_summary(*bins)
        ms = []
        for _ in range(STEPS):
            s = ctx.run_summary(*bins)
            ms.append(s.kernel_ms)
        rec.update(pairs=s.pairs, counted_pairs=s.counted_pairs, r2_sum=s.r2_sum)
    else:
        steps = 3
        call = (lambda: ctx.run_host(-1.0)) if args.what == "e2e_rows" else (lambda: ctx.run_summary(BIN_WIDTH, N_BINS))
        call()
        ms = []
        for _ in range(steps):
            t0 = time.perf_counter()
            r = call()
            ms.append((time.perf_counter() - t0) * 1e3)
        rec.update(rows=len(r) if args.what == "e2e_rows" else 0)
    rec.update(ms=float(np.median(ms)), ms_min=float(min(ms)), ms_max=float(max(ms)), steps=len(ms))
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


def summary(args):
    recs = [json.loads(open(p).read()) for p in args.files]
    print("%-13s %10s %10s %10s  %s" % ("what", "ms", "min", "max", "library"))
    for r in recs:
        print("%-13s %10.3f %10.3f %10.3f  %s" % (r["what"], r["ms"], r["ms_min"], r["ms_max"], r["lib"]))
    rows = [r["ms"] for r in recs if r["what"] == "rows"]
    ok = True
    if rows:
        base = float(np.median(rows))
        print("row path's every-tile launch: median %.3f ms over %d runs; limit 1.10 x = %.3f ms" %
              (base, len(rows), 1.10 * base))
        for r in recs:
            if r["what"] in ("summary", "summary_bins"):
                good = r["ms"] <= 1.10 * base
                ok = ok and good
                print("  %-13s %.3f ms = %.3f x  %s" % (r["what"], r["ms"], r["ms"] / base, "ok" if good else "MISSED"))
    for a, b in (("e2e_rows", "e2e_summary"),):
        x = [r["ms"] for r in recs if r["what"] == a]
        y = [r["ms"] for r in recs if r["what"] == b]
        if x and y:
            print("end to end, %d sites: run_host(-1.0) %.1f ms, run_summary %.1f ms (%.0f x)" %
                  (L2, np.median(x), np.median(y), np.median(x) / np.median(y)))
    return 0 if ok else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("run")
    a.add_argument("--what", required=True, choices=["rows", "summary", "summary_bins", "e2e_rows", "e2e_summary"])
    a.add_argument("--tree", help="checkout whose weightedld_amd (and built library) to measure; default this one")
    a.add_argument("--cache")
    a.add_argument("--out")
    b = sub.add_parser("summary")
    b.add_argument("files", nargs="+")
    ns = ap.parse_args()
    sys.exit(run(ns) if ns.cmd == "run" else summary(ns))
