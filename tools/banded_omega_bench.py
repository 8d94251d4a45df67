#!/usr/bin/env python3
"""What the sweep scan costs: HIP-event times, warm, medians,

  * scan20k — bench.synth(20000, 2000) with Henikoff weights, max_side 500
    (window max_sites 999, K = 999), r2 with zero_missing: the band fill
    (run_matrix_banded), the pair sums (banded_pairsum) and the scan
    (banded_omega) separately, for every split and for n_grid 1,000; the pair
    sums against their byte model (4 + 2 (8 + 8) bytes per band element at the
    streaming HBM rate), the scan in candidates per second and f64 divisions per
    second; and what a user did before: the band to the host, then
    banded_pairsum_host + banded_omega_host in numpy on the same inputs (the
    numpy scan on the first --host-splits splits of each list, scaled);
  * million — 1,000,000 x 200 synthetic sites, max_side 500, n_grid 10,000: the
    4 GB band, the 8 GB table and the scan.  No host arm at that size.

    python tools/banded_omega_bench.py run --what WHAT --cache FILE --out FILE    one measurement; one JSON line
    python tools/banded_omega_bench.py summary FILE...                            the tables
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from banded_bench import HBM_BYTES_PER_S, L, LM, N, NM, data, stats  # noqa: E402

WHATS = ["scan20k", "million"]
MAX_SIDE, MIN_SIDE, EPS = 500, 2, 1e-5


def candidates(split, lo, hi, min_side):
    c, l, h = (x.astype(np.int64) for x in (split, lo, hi))
    return int((np.maximum(0, c - min_side + 2 - l) * np.maximum(0, h - c - min_side + 1)).sum())


def run(args):
    import torch
    import weightedld_amd as W
    what = args.what
    big = what == "million"
    buf, w = data(LM, NM, None) if big else data(L, N, args.cache)
    n = int(buf.shape[0])
    steps, warmup = (3, 1) if big else (10, 3)
    ctx = W.Context(0)
    ctx.load(buf, w)
    ctx.set_window(0, 2 * MAX_SIDE - 1)
    K = ctx.matrix_banded_width()
    rec = {"what": what, "lib": os.path.relpath(W.LIB_PATH, REPO), "sites": n, "seqs": int(buf.shape[1]), "bandwidth": K,
           "max_side": MAX_SIDE, "min_side": MIN_SIDE, "eps": EPS, "band_bytes": n * (K + 1) * 4,
           "table_bytes": n * (K + 1) * 8}
    band = torch.empty((n, K + 1), dtype=torch.float32, device="cuda:0")
    ms = []
    for it in range(warmup + steps):
        _, info = ctx.run_matrix_banded(stat="r2", zero_missing=True, out=band)
        if it >= warmup:
            ms.append(info.kernel_ms)
    rec["fill"] = dict(stats(ms), pairs=info.pairs)
    M = torch.empty((n, K + 1), dtype=torch.float64, device="cuda:0")
    ms = []
    for it in range(warmup + steps):
        _, pinfo = ctx.banded_pairsum(band, out=M)
        if it >= warmup:
            ms.append(pinfo.kernel_ms)
    model = n * (K + 1) * (4 + 2 * (8 + 8)) / HBM_BYTES_PER_S * 1e3
    rec["pairsum"] = dict(stats(ms), nonfinite=pinfo.nonfinite, model_ms=model)
    rec["pairsum"]["fraction_of_model"] = model / rec["pairsum"]["ms"]
    rec["scans"] = []
    host_M = None
    for n_grid in ((10000,) if big else (0, 1000)):
        _, split, lo, hi = W.omega_splits(None, n, n_grid, MAX_SIDE)
        dev = [torch.from_numpy(x.view(np.int32)).cuda() for x in (split, lo, hi)]
        ms = []
        for it in range(warmup + steps):
            res = ctx.banded_omega(M, dev[0], dev[1], dev[2], MIN_SIDE, EPS)
            if it >= warmup:
                ms.append(res.kernel_ms)
        cand = candidates(split, lo, hi, MIN_SIDE)
        assert cand == res.evaluated + res.skipped
        r = dict(stats(ms), n_grid=n_grid, splits=len(split), candidates=cand, evaluated=res.evaluated, skipped=res.skipped,
                 omega_max=float(np.nanmax(res.omega)), zns_mean=float(res.zns.mean()))
        r["candidates_per_s"] = cand / (r["ms"] * 1e-3)
        r["f64_divisions_per_s"] = (res.evaluated * 3 + res.skipped * 2) / (r["ms"] * 1e-3)
        r["table_bytes_per_s"] = cand * 8 / (r["ms"] * 1e-3)  # (ST alone: one f64 per candidate)
        if not big:
            # the host arm: the band to the host, the numpy twins
            t0 = time.perf_counter()
            hb = band.cpu().numpy()
            t1 = time.perf_counter()
            if host_M is None:
                host_M = W.banded_pairsum_host(hb)
                rec["host_pairsum_s"] = time.perf_counter() - t1
                rec["host_copy_s"] = t1 - t0
                assert host_M.tobytes() == M.cpu().numpy().tobytes(), "the device table is the twin's"
            g = min(args.host_splits, len(split))
            t2 = time.perf_counter()
            want = W.banded_omega_host(host_M, split[:g], lo[:g], hi[:g], MIN_SIDE, EPS)
            host_s = time.perf_counter() - t2
            assert want.omega.tobytes() == res.omega[:g].tobytes() and np.array_equal(want.left, res.left[:g])
            sub = candidates(split[:g], lo[:g], hi[:g], MIN_SIDE)
            r["host"] = {"splits": g, "candidates": sub, "s": host_s, "s_scaled": host_s * cand / max(sub, 1)}
        rec["scans"].append(r)
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


def summary(args):
    for p in args.files:
        rec = json.loads(open(p).read())
        print("%s: %d sites, bandwidth %d, max_side %d; band %.2f GB, table %.2f GB" %
              (rec["what"], rec["sites"], rec["bandwidth"], rec["max_side"], rec["band_bytes"] / 1e9, rec["table_bytes"] / 1e9))
        f, s = rec["fill"], rec["pairsum"]
        print("  band fill %9.3f ms (min %.3f, max %.3f), %d pairs" % (f["ms"], f["ms_min"], f["ms_max"], f["pairs"]))
        print("  pair sums %9.3f ms (min %.3f, max %.3f); byte model %.3f ms: %.1f %% of it" %
              (s["ms"], s["ms_min"], s["ms_max"], s["model_ms"], 100 * s["fraction_of_model"]))
        if "host_pairsum_s" in rec:
            print("  host: band copy %.3f s, banded_pairsum_host %.3f s" % (rec["host_copy_s"], rec["host_pairsum_s"]))
        for r in rec["scans"]:
            print("  scan n_grid %-6d %9.3f ms (min %.3f, max %.3f): %d splits, %.3g candidates (%d skipped), %.3g candidates/s, "
                  "%.3g f64 divisions/s, %.3g table bytes/s" %
                  (r["n_grid"], r["ms"], r["ms_min"], r["ms_max"], r["splits"], r["candidates"], r["skipped"],
                   r["candidates_per_s"], r["f64_divisions_per_s"], r["table_bytes_per_s"]))
            if "host" in r:
                h = r["host"]
                print("    banded_omega_host on %d splits (%.3g candidates): %.2f s, scaled to the list %.1f s: %.0f x the device" %
                      (h["splits"], h["candidates"], h["s"], h["s_scaled"], h["s_scaled"] / (r["ms"] * 1e-3)))
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("run")
    a.add_argument("--what", required=True, choices=WHATS)
    a.add_argument("--cache")
    a.add_argument("--out")
    a.add_argument("--host-splits", type=int, default=200)
    b = sub.add_parser("summary")
    b.add_argument("files", nargs="+")
    ns = ap.parse_args()
    sys.exit(run(ns) if ns.cmd == "run" else summary(ns))
