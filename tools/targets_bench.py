#!/usr/bin/env python3
"""Target-site LD (Context.run_targets) against the only routes the parent
commit has to the same answer, on bench.synth(20000, 2000) and
bench.ld_blocks(20000, 2000) with Henikoff weights, warm:

  targets     run_targets for Q in {1, 16, 256} evenly spaced targets at r2 >
              0.0 and 0.2: kernel_ms (the pair launches) and wall time;
  rows        the row path's every-tile reference-order launch
              (set_option("screen", 0), stats()["pair_kernel_ms"] — bench.py's
              unscreened_pair_kernel_ms): the kernel time of the triangle, the
              only route to a threshold-0 answer; no row is copied;
  e2e_rows    run_host(0.2) plus the numpy filter for the Q = 16 targets, end
              to end;
  hbm         the device's streaming read rate (a 1 GiB torch reduction), for
              the model.

    python tools/targets_bench.py run --what targets|rows|e2e_rows|hbm --data synth|ld_blocks
                                      [--tree DIR] --cache FILE --out FILE      one measurement; one JSON line
    python tools/targets_bench.py summary FILE...                  the tables

Each run is a process of its own (tools/targets_bench.sh gives each its own
time limit and interleaves the two sides); --tree DIR imports weightedld_amd
(package and built library) from another checkout, so the parent side can be
the parent commit's build on the same device.

The model of a launch is the larger of one read of the lane-class codes at the
measured HBM rate and 16 ceil(Q / 16) L pair sums at the pairs/s the rows
launch reaches on the same data.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
L, N, STEPS, WARMUP = 20000, 2000, 10, 3
QS, THRS = (1, 16, 256), (0.0, 0.2)


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


def targets_of(q):
    return (np.arange(q, dtype=np.int64) * L // q + L // (2 * q)).astype(np.uint32)


def med(x):
    return {"ms": float(np.median(x)), "ms_min": float(min(x)), "ms_max": float(max(x)), "steps": len(x)}


def run(args):
    if args.tree:
        sys.path.insert(0, os.path.abspath(args.tree))
    import weightedld_amd as W
    rec = {"what": args.what, "data": args.data, "lib": W.LIB_PATH, "sites": L, "seqs": N}
    if args.what == "hbm":
        import torch
        x = torch.ones(1 << 28, dtype=torch.float32, device="cuda")
        ms = []
        for k in range(WARMUP + STEPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            x.sum()
            b.record()
            torch.cuda.synchronize()
            if k >= WARMUP:
                ms.append(a.elapsed_time(b))
        rec.update(med(ms), bytes=int(x.numel() * 4), gb_per_s=float(x.numel() * 4 / np.median(ms) / 1e6))
    else:
        buf, w = data(args.data, args.cache)
        ctx = W.Context(0)
        ctx.load(buf, w)
        if args.what == "rows":
            ctx.set_option("screen", 0)
            for _ in range(WARMUP):
                ctx.run_chunks(0.05)
            ms = []
            for _ in range(STEPS):
                ctx.run_chunks(0.05)
                ms.append(ctx.stats()["pair_kernel_ms"])
            st = ctx.stats()
            rec.update(med(ms), pairs=st["pairs"], ref_sums=st["ref_sums"],
                       pairs_per_s=float(st["pairs"] / np.median(ms) * 1e3))
        elif args.what == "e2e_rows":
            t = targets_of(16)
            ms = []
            for k in range(1 + 3):
                t0 = time.perf_counter()
                rows = ctx.run_host(0.2)
                sel = np.isin(rows.site_a, t) | np.isin(rows.site_b, t)
                kept = int(sel.sum())
                if k:
                    ms.append((time.perf_counter() - t0) * 1e3)
            rec.update(med(ms), rows=len(rows), kept=kept)
        else:
            cases = []
            for q in QS:
                t = targets_of(q)
                for thr in THRS:
                    for _ in range(WARMUP):
                        ctx.run_targets(t, thr)
                    km, wm = [], []
                    for _ in range(STEPS):
                        t0 = time.perf_counter()
                        r = ctx.run_targets(t, thr)
                        wm.append((time.perf_counter() - t0) * 1e3)
                        km.append(r.kernel_ms)
                    cases.append({"q": q, "thr": thr, "rows": len(r), "items": r.items, "batches": r.batches,
                                  "kernel": med(km), "wall": med(wm)})
            rec.update(cases=cases)
        ctx.close()
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


def summary(args):
    recs = [json.loads(open(p).read()) for p in args.files]
    hbm = [r["gb_per_s"] for r in recs if r["what"] == "hbm"]
    hbm = float(np.median(hbm)) if hbm else None
    if hbm:
        print("HBM streaming read: %.0f GB/s" % hbm)
    npr = 8 * ((N // 8 + 63) // 64) * 64 + (64 if N % 8 else 0)
    code_bytes = (L + 63) // 64 * 64 * npr
    for kind in ("synth", "ld_blocks"):
        rows = [r for r in recs if r["what"] == "rows" and r["data"] == kind]
        e2e = [r for r in recs if r["what"] == "e2e_rows" and r["data"] == kind]
        tg = [r for r in recs if r["what"] == "targets" and r["data"] == kind]
        if not (rows or tg):
            continue
        print("== %s(%d, %d)" % (kind, L, N))
        rate = None
        if rows:
            ms = float(np.median([r["ms"] for r in rows]))
            rate = float(np.median([r["pairs_per_s"] for r in rows]))
            print("rows (every tile, reference order): %.3f ms over %d runs, %.3g pairs/s  [%s]" %
                  (ms, len(rows), rate, rows[0]["lib"]))
        if e2e:
            print("run_host(0.2) + filter for 16 targets, end to end: %.1f ms (%d rows, %d kept)" %
                  (np.median([r["ms"] for r in e2e]), e2e[0]["rows"], e2e[0]["kept"]))
        if not tg:
            continue
        print("%5s %5s %9s %8s %10s %10s %10s %8s %8s" %
              ("Q", "thr", "rows", "items", "kernel ms", "wall ms", "model ms", "of model", "vs rows"))
        for q in QS:
            for thr in THRS:
                c = [x for r in tg for x in r["cases"] if x["q"] == q and x["thr"] == thr]
                k = float(np.median([x["kernel"]["ms"] for x in c]))
                wl = float(np.median([x["wall"]["ms"] for x in c]))
                model = None
                if hbm and rate:
                    model = max(code_bytes / (hbm * 1e9), 16 * ((q + 15) // 16) * L / rate) * 1e3
                print("%5d %5.1f %9d %8d %10.4f %10.3f %10s %8s %8s" %
                      (q, thr, c[0]["rows"], c[0]["items"], k, wl, "%.4f" % model if model else "-",
                       "%.2f" % (model / k) if model and k > 0 else "-",
                       "%.0f x" % (np.median([r["ms"] for r in rows]) / k) if rows and k > 0 else "-"))
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("run")
    a.add_argument("--what", required=True, choices=["targets", "rows", "e2e_rows", "hbm"])
    a.add_argument("--data", default="synth", choices=["synth", "ld_blocks"])
    a.add_argument("--tree", help="checkout whose weightedld_amd (and built library) to measure; default this one")
    a.add_argument("--cache")
    a.add_argument("--out")
    b = sub.add_parser("summary")
    b.add_argument("files", nargs="+")
    ns = ap.parse_args()
    sys.exit(run(ns) if ns.cmd == "run" else summary(ns))
