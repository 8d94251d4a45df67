#!/usr/bin/env python3
"""What the LD blocks cost: pass 1's launch (Context.run_block_breaks'
kernel_ms) against the summary launch (Context.run_summary's kernel_ms) on the
same load — both run every in-window tile through the same sums, and the
summary code is the yardstick other reductions were measured by — pass 2's
time and tile count, the whole run_blocks call, and the alternative the
feature replaces: every in-window row at threshold -1 copied to the host and
scanned in numpy.  bench.ld_blocks(20000, 2000) with Henikoff weights, once
without a window and once at max_sites 1,000; one process, the two launches
interleaved, warm.

    python tools/blocks_bench.py [--sites L] [--seqs N] [--strong-min T] [--steps K] [--warmup W]
                                 [--no-rows] [--out FILE]

Prints one JSON line per window and a table.  No gate: the ratio of pass 1 to
the summary launch is reported, not checked.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def rows_scan(ctx, W, n_sites, last, strong_min):
    """The alternative: all in-window rows to the host, break arrays in numpy,
    the partition by the library's host code."""
    r = ctx.run_host(-1.0)
    weak = np.isfinite(r.r2) & ~(r.r2 >= np.float32(strong_min))
    a, b = r.site_a[weak].astype(np.int64), r.site_b[weak].astype(np.int64)
    fwd = np.full(n_sites, n_sites, dtype=np.int64)
    np.minimum.at(fwd, a, b)
    bwd = np.full(n_sites, -1, dtype=np.int64)
    np.maximum.at(bwd, b, a)
    none = np.uint32(W.BLOCKS_NONE)
    brk = W.LdBlockBreaks(fwd_weak=np.where(fwd == n_sites, none, fwd).astype(np.uint32),
                          bwd_weak=np.where(bwd < 0, none, bwd).astype(np.uint32), last=last, stat="r2",
                          strong_min=float(np.float32(strong_min)), pairs=len(r), none_pairs=0, nonfinite_pairs=0,
                          strong_pairs=0, weak_pairs=int(weak.sum()), tiles=0, kernel_ms=0.0)
    return brk.partition("all"), len(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=20000)
    ap.add_argument("--seqs", type=int, default=2000)
    ap.add_argument("--strong-min", type=float, default=0.3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-sites", type=int, default=1000)
    ap.add_argument("--no-rows", action="store_true", help="skip the rows-to-host alternative")
    ap.add_argument("--out")
    ns = ap.parse_args()
    import bench
    import weightedld_amd as W
    buf = bench.ld_blocks(ns.sites, ns.seqs)
    w = W.henikoff_weights(W.SiteSet.from_buffer(buf))
    ctx = W.Context(0)
    ctx.load(buf, w)
    recs = []
    for K in (0, ns.max_sites):
        ctx.set_window(0, K)
        for _ in range(ns.warmup):
            ctx.run_summary()
            ctx.run_block_breaks(ns.strong_min)
        s_ms, p1_ms, p2_ms, call_ms = [], [], [], []
        for _ in range(ns.steps):  # interleaved
            s_ms.append(ctx.run_summary().kernel_ms)
            b = ctx.run_block_breaks(ns.strong_min)
            p1_ms.append(b.kernel_ms)
        for _ in range(ns.steps):
            t0 = time.perf_counter()
            r = ctx.run_blocks(ns.strong_min)
            call_ms.append((time.perf_counter() - t0) * 1e3)
            p2_ms.append(r.kernel_ms)
        rec = {"sites": ns.sites, "seqs": ns.seqs, "max_sites": K, "strong_min": ns.strong_min, "steps": ns.steps,
               "lib": os.path.relpath(W.LIB_PATH, REPO), "pairs": b.pairs, "weak_pairs": b.weak_pairs, "tiles": b.tiles,
               "summary_ms": float(np.median(s_ms)), "summary_min": min(s_ms), "summary_max": max(s_ms),
               "pass1_ms": float(np.median(p1_ms)), "pass1_min": min(p1_ms), "pass1_max": max(p1_ms),
               "pass2_ms": float(np.median(p2_ms)), "pass2_tiles": r.tiles, "blocks": r.n_blocks,
               "largest_block": int(r.sites.max()) if r.n_blocks else 0,
               "call_ms": float(np.median(call_ms)), "call_min": min(call_ms), "call_max": max(call_ms)}
        rec["ratio"] = rec["pass1_ms"] / rec["summary_ms"]
        if K and not ns.no_rows:
            ms = []
            for _ in range(3):
                t0 = time.perf_counter()
                p, n_rows = rows_scan(ctx, W, ns.sites, b.last, ns.strong_min)
                ms.append((time.perf_counter() - t0) * 1e3)
            same = np.array_equal(p.first, r.first) and np.array_equal(p.last, r.last)
            rec.update(rows=n_rows, rows_scan_ms=float(np.median(ms)), rows_scan_same_blocks=bool(same))
        recs.append(rec)
        print(json.dumps(rec))
    ctx.close()
    print("%-10s %10s %10s %7s %8s %10s %8s %10s %8s" % ("max_sites", "summary", "pass 1", "ratio", "tiles", "pass 2",
                                                         "tiles", "call", "blocks"))
    for r in recs:
        print("%-10d %10.3f %10.3f %7.3f %8d %10.3f %8d %10.3f %8d" % (
            r["max_sites"], r["summary_ms"], r["pass1_ms"], r["ratio"], r["tiles"], r["pass2_ms"], r["pass2_tiles"],
            r["call_ms"], r["blocks"]))
        if "rows_scan_ms" in r:
            print("           rows at -1 to the host + numpy scan: %.1f ms for %d rows (%.0f x the call); same blocks: %s"
                  % (r["rows_scan_ms"], r["rows"], r["rows_scan_ms"] / r["call_ms"], r["rows_scan_same_blocks"]))
    if ns.out:
        with open(ns.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
