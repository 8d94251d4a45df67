#!/usr/bin/env python3
"""What the best-partner run's selecting epilogue and merge cost against the
row path's every-tile launch: Context.run_partners' kernel_ms + merge_ms against
the row path's every-tile reference-order launch (set_option("screen", 0), r2 >
0.05, stats()["pair_kernel_ms"] — the baseline of tools/summary_bench.py,
targets_bench.py and heatmap_bench.py) on bench.synth(20000, 2000) and
bench.ld_blocks(20000, 2000) with Henikoff weights, warm; and end to end for
k = 8 at threshold 0.2, run_partners against the route a user had before it:
run_host(0.2) plus a numpy group-by of the rows.

    python tools/partners_bench.py run --data synth|ldb --what rows|k1|k8|k64|k8_t02|e2e_rows
                                       [--tree DIR] --cache FILE --out FILE     one measurement; one JSON line
    python tools/partners_bench.py summary FILE...                 the table, and the check

Each run is a process of its own (tools/partners_bench.sh gives each its own
time limit and interleaves the two sides); --tree DIR imports weightedld_amd
(package and built library) from another checkout, so the baseline can be the
parent commit's build on the same device.  k1, k8 and k64 run at threshold -1
(every pair with a statistic is a candidate: the epilogue's worst case).  The
summary fails unless every k8 run is within 1.10 x the median row launch of its
data set; k1, k64, k8_t02 and the end-to-end times are recorded without a gate.
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
WHATS = {"k1": (1, -1.0), "k8": (8, -1.0), "k64": (64, -1.0), "k8_t02": (8, 0.2)}
GATED = ("k8",)


def data(kind, cache):
    import bench
    import weightedld_amd as W
    if cache and os.path.exists(cache):
        z = np.load(cache)
        return z["buf"], z["w"]
    buf = getattr(bench, "ld_blocks" if kind == "ldb" else "synth")(L, N)
    w = W.henikoff_weights(W.SiteSet.from_buffer(buf))
    if cache:
        np.savez(cache, buf=buf, w=w)
    return buf, w


def group_rows(r, n_sites, k):
    """The numpy route from rows to lists: both directions of every row,
    sorted by (site, r2 descending, partner), the first k per site."""
    site = np.concatenate((r.site_a, r.site_b)).astype(np.int64)
    part = np.concatenate((r.site_b, r.site_a)).astype(np.int64)
    r2 = np.concatenate((r.r2, r.r2))
    order = np.lexsort((part, -r2.astype(np.float64), site))
    site, part = site[order], part[order]
    start = np.searchsorted(site, np.arange(n_sites))
    rank = np.arange(site.size) - start[site]
    keep = rank < k
    return int(keep.sum()), int(part[keep].sum())


def run(args):
    if args.tree:
        sys.path.insert(0, os.path.abspath(args.tree))
    import weightedld_amd as W
    buf, w = data(args.data, args.cache)
    ctx = W.Context(0)
    ctx.load(buf, w)
    rec = {"what": args.what, "data": args.data, "lib": W.LIB_PATH, "sites": int(buf.shape[0]), "seqs": int(buf.shape[1])}
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
    elif args.what == "e2e_rows":
        k, thr = WHATS["k8_t02"]
        group_rows(ctx.run_host(thr), L, k)
        ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            r = ctx.run_host(thr)
            listed, check = group_rows(r, L, k)
            ms.append((time.perf_counter() - t0) * 1e3)
        rec.update(rows=len(r), listed=listed, partner_sum=check)
    else:
        k, thr = WHATS[args.what]
        for _ in range(WARMUP):
            ctx.run_partners(k, thr)
        ms, kern, merge, wall = [], [], [], []
        for _ in range(STEPS):
            t0 = time.perf_counter()
            p = ctx.run_partners(k, thr)
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(p.kernel_ms + p.merge_ms)
            kern.append(p.kernel_ms)
            merge.append(p.merge_ms)
        filled = p.partner != 0xFFFFFFFF
        rec.update(k=k, thr=thr, tiles=p.tiles, pairs=p.pairs, passing_pairs=p.passing_pairs,
                   listed=int(p.count.sum()), partner_sum=int(p.partner[filled].astype(np.int64).sum()),
                   kernel_ms=float(np.median(kern)), merge_ms=float(np.median(merge)), call_ms=float(np.median(wall)))
    rec.update(ms=float(np.median(ms)), ms_min=float(min(ms)), ms_max=float(max(ms)), steps=len(ms))
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


def summary(args):
    recs = [json.loads(open(p).read()) for p in args.files]
    print("%-6s %-9s %10s %10s %10s %10s %10s %8s  %s" % ("data", "what", "ms", "min", "max", "kernel", "merge", "tiles",
                                                         "library"))
    for r in recs:
        print("%-6s %-9s %10.3f %10.3f %10.3f %10s %10s %8s  %s" %
              (r["data"], r["what"], r["ms"], r["ms_min"], r["ms_max"],
               "%.3f" % r["kernel_ms"] if "kernel_ms" in r else "", "%.3f" % r["merge_ms"] if "merge_ms" in r else "",
               r.get("tiles", ""), r["lib"]))
    ok = True
    for d in ("synth", "ldb"):
        rows = [r["ms"] for r in recs if r["what"] == "rows" and r["data"] == d]
        if not rows:
            continue
        base = float(np.median(rows))
        print("%s: row path's every-tile launch: median %.3f ms over %d runs; limit 1.10 x = %.3f ms" %
              (d, base, len(rows), 1.10 * base))
        for r in recs:
            if r["data"] != d or r["what"] not in WHATS:
                continue
            gated = r["what"] in GATED
            good = r["ms"] <= 1.10 * base
            ok = ok and (good or not gated)
            print("  %-7s kernel %.3f + merge %.3f = %.3f ms = %.3f x, call %.1f ms  %s" %
                  (r["what"], r["kernel_ms"], r["merge_ms"], r["ms"], r["ms"] / base, r["call_ms"],
                   ("ok" if good else "MISSED") if gated else "(no gate)"))
        x = [r for r in recs if r["what"] == "e2e_rows" and r["data"] == d]
        y = [r for r in recs if r["what"] == "k8_t02" and r["data"] == d]
        if x and y:
            print("  end to end, k 8 at r2 > 0.2: run_host + numpy group-by %.1f ms (%d rows, %d listed); "
                  "run_partners %.1f ms (%d listed; same lists: %s)" %
                  (x[0]["ms"], x[0]["rows"], x[0]["listed"], y[0]["call_ms"], y[0]["listed"],
                   x[0]["listed"] == y[0]["listed"] and x[0]["partner_sum"] == y[0]["partner_sum"]))
    return 0 if ok else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("run")
    a.add_argument("--what", required=True, choices=["rows", "e2e_rows", *WHATS])
    a.add_argument("--data", required=True, choices=["synth", "ldb"])
    a.add_argument("--tree", help="checkout whose weightedld_amd (and built library) to measure; default this one")
    a.add_argument("--cache")
    a.add_argument("--out")
    b = sub.add_parser("summary")
    b.add_argument("files", nargs="+")
    ns = ap.parse_args()
    sys.exit(run(ns) if ns.cmd == "run" else summary(ns))
