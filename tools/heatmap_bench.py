#!/usr/bin/env python3
"""What the heat map's reducing epilogue costs against the row path's
compaction: the heat-map launch (Context.run_heatmap's kernel_ms) against the
row path's every-tile reference-order launch (set_option("screen", 0), r2 >
0.05, stats()["pair_kernel_ms"] — the baseline of tools/summary_bench.py) on
bench.synth(20000, 2000) with Henikoff weights, warm; a region of it (sites
2,000..3,999, 100 cells: the tile filter); and end to end, run_heatmap against
run_host(-1.0) plus a numpy binning of the rows into 100 x 100 cells on
bench.ld_blocks(5000, 500).

    python tools/heatmap_bench.py run --what rows|heat256_r2|heat256_dprime|heat4096|region|e2e_rows|e2e_heat
                                      [--tree DIR] --cache FILE --out FILE      one measurement; one JSON line
    python tools/heatmap_bench.py summary FILE...                  the table, and the check

Each run is a process of its own (tools/heatmap_bench.sh gives each its own
time limit and interleaves the two sides); --tree DIR imports weightedld_amd
(package and built library) from another checkout, so the baseline can be the
parent commit's build on the same device.  The summary fails unless every
256-cell heat-map launch is within 1.10 x the median row launch; the
4,096-cell map, the region and the end-to-end times are recorded without a
gate.
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
L2, N2, CELLS2 = 5000, 500, 100
REGION = (2000, 4000, 100)  # sites [2000, 4000), 100 cells
GATED = ("heat256_r2", "heat256_dprime")
WHATS = ["rows", "heat256_r2", "heat256_dprime", "heat4096", "region", "e2e_rows", "e2e_heat"]


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


def equal_cells(n_sites, n_cells):
    per = (n_sites + n_cells - 1) // n_cells
    return (np.arange(n_sites) // per).astype(np.int32)


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
    elif not e2e:
        if args.what == "region":
            n_cells = REGION[2]
            cells = np.full(L, -1, dtype=np.int32)
            cells[REGION[0]:REGION[1]] = equal_cells(REGION[1] - REGION[0], n_cells)
        else:
            n_cells = 4096 if args.what == "heat4096" else 256
            cells = equal_cells(L, n_cells)
        stat = "dprime" if args.what.endswith("dprime") else "r2"
        steps = 3 if args.what == "heat4096" else STEPS  # (each copies 335 MB back)
        for _ in range(1 if args.what == "heat4096" else WARMUP):
            ctx.run_heatmap(cells, n_cells, stat)
        ms, wall = [], []
        for _ in range(steps):
            t0 = time.perf_counter()
            h = ctx.run_heatmap(cells, n_cells, stat)
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(h.kernel_ms)
        rec.update(tiles=h.tiles, pairs=h.pairs, counted_pairs=h.counted_pairs, n_cells=n_cells, stat=stat,
                   total=float(h.sum.sum()), call_ms=float(np.median(wall)))
    else:
        steps = 3
        cells = equal_cells(L2, CELLS2)

        def rows_binned():
            r = ctx.run_host(-1.0)
            k = cells[r.site_a].astype(np.int64) * CELLS2 + cells[r.site_b]
            fin = np.isfinite(r.r2)
            count = np.bincount(k[fin], minlength=CELLS2 * CELLS2)
            total = np.bincount(k[fin], weights=r.r2[fin].astype(np.float64), minlength=CELLS2 * CELLS2)
            mx = np.full(CELLS2 * CELLS2, -np.inf, dtype=np.float32)
            np.maximum.at(mx, k[fin], r.r2[fin])
            return len(r), int(count.sum()), float(total.sum())

        def heat():
            h = ctx.run_heatmap(cells, CELLS2)
            return 0, h.counted_pairs, float(h.sum.sum())

        call = rows_binned if args.what == "e2e_rows" else heat
        call()
        ms = []
        for _ in range(steps):
            t0 = time.perf_counter()
            rows, counted, total = call()
            ms.append((time.perf_counter() - t0) * 1e3)
        rec.update(rows=rows, counted_pairs=counted, total=total)
    rec.update(ms=float(np.median(ms)), ms_min=float(min(ms)), ms_max=float(max(ms)), steps=len(ms))
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


def summary(args):
    recs = [json.loads(open(p).read()) for p in args.files]
    print("%-15s %10s %10s %10s %8s  %s" % ("what", "ms", "min", "max", "tiles", "library"))
    for r in recs:
        print("%-15s %10.3f %10.3f %10.3f %8s  %s" % (r["what"], r["ms"], r["ms_min"], r["ms_max"], r.get("tiles", ""),
                                                     r["lib"]))
    rows = [r["ms"] for r in recs if r["what"] == "rows"]
    ok = True
    if rows:
        base = float(np.median(rows))
        print("row path's every-tile launch: median %.3f ms over %d runs; limit 1.10 x = %.3f ms" %
              (base, len(rows), 1.10 * base))
        for r in recs:
            if r["what"] in GATED:
                good = r["ms"] <= 1.10 * base
                ok = ok and good
                print("  %-15s %.3f ms = %.3f x  %s" % (r["what"], r["ms"], r["ms"] / base, "ok" if good else "MISSED"))
            elif r["what"] in ("heat4096", "region"):
                print("  %-15s %.3f ms = %.3f x  %d tiles, call %.1f ms (no gate)" %
                      (r["what"], r["ms"], r["ms"] / base, r["tiles"], r["call_ms"]))
    x = [r["ms"] for r in recs if r["what"] == "e2e_rows"]
    y = [r["ms"] for r in recs if r["what"] == "e2e_heat"]
    if x and y:
        print("end to end, %d sites, %d x %d cells: run_host(-1.0) + numpy binning %.1f ms, run_heatmap %.1f ms (%.0f x)" %
              (L2, CELLS2, CELLS2, np.median(x), np.median(y), np.median(x) / np.median(y)))
    return 0 if ok else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("run")
    a.add_argument("--what", required=True, choices=WHATS)
    a.add_argument("--tree", help="checkout whose weightedld_amd (and built library) to measure; default this one")
    a.add_argument("--cache")
    a.add_argument("--out")
    b = sub.add_parser("summary")
    b.add_argument("files", nargs="+")
    ns = ap.parse_args()
    sys.exit(run(ns) if ns.cmd == "run" else summary(ns))
