#!/usr/bin/env python3
"""What LD pruning costs on the device against the host route on the same
tree: Context.run_prune (rows stay on the device; CSR build, rounds, tags)
against Context.run_host at the same threshold (every row copied to the host)
plus a sequential greedy over the returned rows, at 20,000 sites x 2,000
sequences with Henikoff weights, warm:

    blocks       bench.ld_blocks, r2 > 0.2, no window
    blocks_win   the same with max_sites = 1000
    synth        bench.synth, r2 > 0.05: the edge-free case

    python tools/prune_bench.py run --case blocks|blocks_win|synth --route device|host
                                    --cache FILE --out FILE        one measurement; one JSON line
    python tools/prune_bench.py summary FILE...                    the table

Each run is a process of its own (tools/prune_bench.sh gives each its own
time limit).  The host route's greedy is numpy on a CSR of the rows (a Python
loop over the sites); its time is reported apart from the row run's, so the
device route can be compared with the rows' transfer alone.  The summary
fails if the two routes of a case disagree on the kept set.
"""
import argparse
import json
import os
import sys
import time
import zlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
L, N, STEPS, WARMUP = 20000, 2000, 5, 1
CASES = {"blocks": ("ld_blocks", 0.2, 0), "blocks_win": ("ld_blocks", 0.2, 1000), "synth": ("synth", 0.05, 0)}


def data(kind, cache):
    import bench
    import weightedld_amd as W
    if cache and os.path.exists(cache):
        z = np.load(cache)
        return z["buf"], z["w"]
    buf = getattr(bench, kind)(L, N)
    w = W.henikoff_weights(W.SiteSet.from_buffer(buf))
    if cache:
        np.savez(cache, buf=buf, w=w)
    return buf, w


def host_greedy(n, a, b):
    """Sequential greedy in index order on the rows (a < b): a site is kept iff
    none of its lower neighbours is kept."""
    order = np.argsort(b, kind="stable")
    lower = a[order]
    off = np.concatenate(([0], np.cumsum(np.bincount(b, minlength=n))))
    keep = np.zeros(n, dtype=bool)
    for v in range(n):
        keep[v] = not keep[lower[off[v]:off[v + 1]]].any()
    return keep


def run(args):
    import weightedld_amd as W
    kind, thr, max_sites = CASES[args.case]
    buf, w = data(kind, args.cache)
    ctx = W.Context(0)
    ctx.load(buf, w)
    ctx.set_window(0, max_sites)
    rec = {"case": args.case, "route": args.route, "sites": L, "seqs": N, "thr": thr, "max_sites": max_sites}
    runs = []
    for k in range(WARMUP + STEPS):
        t0 = time.perf_counter()
        if args.route == "device":
            p = ctx.run_prune(thr)
            wall = (time.perf_counter() - t0) * 1e3
            csr, rounds, tags = ctx.prune_times()
            r = {"wall_ms": wall, "pair_ms": p.pair_ms, "prune_ms": p.prune_ms, "csr_ms": csr, "rounds_ms": rounds,
                 "tags_ms": tags, "rounds": p.rounds}
            keep, edges = p.keep, p.edges
        else:
            rows = ctx.run_host(thr)
            t1 = time.perf_counter()
            keep = host_greedy(L, rows.site_a.astype(np.int64), rows.site_b.astype(np.int64))
            t2 = time.perf_counter()
            r = {"wall_ms": (t2 - t0) * 1e3, "rows_ms": (t1 - t0) * 1e3, "greedy_ms": (t2 - t1) * 1e3}
            edges = len(rows)
        if k >= WARMUP:
            runs.append(r)
    for f in runs[0]:
        v = [x[f] for x in runs]
        rec[f] = float(np.median(v))
        rec[f + "_min"], rec[f + "_max"] = float(min(v)), float(max(v))
    rec.update(edges=int(edges), n_kept=int(keep.sum()), keep_crc=zlib.crc32(np.packbits(keep).tobytes()), steps=len(runs))
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


def summary(args):
    recs = [json.loads(open(p).read()) for p in args.files]
    ok = True
    for case in CASES:
        dev = [r for r in recs if r["case"] == case and r["route"] == "device"]
        host = [r for r in recs if r["case"] == case and r["route"] == "host"]
        for d in dev:
            print("%-10s device: %d edges, %d kept; pair %.3f ms, prune %.3f ms (CSR %.3f, rounds %.3f in %d launches, "
                  "tags %.3f); wall %.2f ms [%.2f, %.2f]" %
                  (case, d["edges"], d["n_kept"], d["pair_ms"], d["prune_ms"], d["csr_ms"], d["rounds_ms"], d["rounds"],
                   d["tags_ms"], d["wall_ms"], d["wall_ms_min"], d["wall_ms_max"]))
        for h in host:
            print("%-10s host:   %d rows, %d kept; run_host %.2f ms + greedy %.2f ms = wall %.2f ms [%.2f, %.2f]" %
                  (case, h["edges"], h["n_kept"], h["rows_ms"], h["greedy_ms"], h["wall_ms"], h["wall_ms_min"],
                   h["wall_ms_max"]))
        for d in dev:
            for h in host:
                same = (d["edges"], d["n_kept"], d["keep_crc"]) == (h["edges"], h["n_kept"], h["keep_crc"])
                ok = ok and same
                print("%-10s device wall / run_host alone %.2f x, / host route %.2f x; kept sets %s" %
                      (case, h["rows_ms"] / d["wall_ms"], h["wall_ms"] / d["wall_ms"], "equal" if same else "DIFFER"))
    return 0 if ok else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("run")
    a.add_argument("--case", required=True, choices=sorted(CASES))
    a.add_argument("--route", required=True, choices=["device", "host"])
    a.add_argument("--cache")
    a.add_argument("--out")
    b = sub.add_parser("summary")
    b.add_argument("files", nargs="+")
    ns = ap.parse_args()
    sys.exit(run(ns) if ns.cmd == "run" else summary(ns))
