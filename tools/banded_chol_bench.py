#!/usr/bin/env python3
"""What the banded Cholesky factorisation costs: HIP-event times, warm, medians,

  * factor20k — bench.synth(20000, 2000) with Henikoff weights under max_sites
    1,000 (K = 1,000), r with zero_missing, ridge 0.1: Context.banded_cholesky
    (kernel_ms) and Context.banded_solve with 1 and 64 columns, against
    torch.linalg.cholesky_ex + torch.cholesky_solve of the float64 dense matrix
    on the same device in the same run, the arms alternating; and against
    banded_cg_solve to 1e-8 for one column;
  * small — the same sites under max_sites 64 and 128: the launch count and
    the time per launch, where launch gaps are what is measured;
  * million — 1,000,000 x 200 synthetic sites under max_sites 1,000: the 8 GB
    factor and the solves.  No dense arm exists at that size.

Where ridge 0.1 leaves the band indefinite the ridge is doubled until the
factorisation succeeds, and the ridge used is reported.

    python tools/banded_chol_bench.py run --what WHAT --cache FILE --out FILE     one measurement; one JSON line
    python tools/banded_chol_bench.py summary FILE...                             the tables
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from banded_bench import L, LM, N, NM, data, stats  # noqa: E402

WHATS = ["factor20k", "small", "million"]
COLS = (1, 64)
RIDGE = 0.1


def launches(n, K):
    """banded_chol_plan.hpp's launches(): the fill, then per block row of 64 the
    diagonal block and, where a panel exists, the panel and the window."""
    count = 1
    for i0 in range(0, n, 64):
        count += 1 + (2 if min(i0 + 64 + K, n) > min(i0 + 64, n) else 0)
    return count


def events(torch, call, steps, warmup):
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def factor(ctx, band, out, steps, warmup):
    """(ridge used, kernel_ms list, info) of banded_cholesky, the ridge doubled while the band is indefinite."""
    ridge = RIDGE
    while True:
        _, info = ctx.banded_cholesky(band, ridge, out=out)
        if info.ok:
            break
        ridge *= 2.0
    for _ in range(warmup):
        ctx.banded_cholesky(band, ridge, out=out)
    ms = []
    for _ in range(steps):
        _, info = ctx.banded_cholesky(band, ridge, out=out)
        ms.append(info.kernel_ms)
    return ridge, ms, info


def solve_ms(ctx, torch, F, n, cols, steps, warmup, g):
    from weightedld_amd._lib import lib
    import ctypes
    out = {}
    for c in cols:
        b = torch.rand((n, c), generator=g, device="cuda:0", dtype=torch.float64) - 0.4
        x = torch.empty_like(b)
        ms = []
        for it in range(warmup + steps):
            x.copy_(b)
            torch.cuda.synchronize()
            t = ctypes.c_double(0.0)
            rc = lib().wld_banded_solve_device(ctx._h, ctypes.c_void_p(F.data_ptr()), F.stride(0), n, F.shape[1] - 1, 0,
                                               ctypes.c_void_p(x.data_ptr()), c, c, ctypes.byref(t))
            assert rc == 0
            if it >= warmup:
                ms.append(t.value)
        out[str(c)] = {"banded": stats(ms), "checksum": float(x.abs().sum())}
    return out


def run(args):
    import torch
    import weightedld_amd as W
    what = args.what
    buf, w = data(LM, NM, None) if what == "million" else data(L, N, args.cache)
    n = int(buf.shape[0])
    ctx = W.Context(0)
    ctx.load(buf, w)
    g = torch.Generator(device="cuda:0").manual_seed(7)
    rec = {"what": what, "lib": os.path.relpath(W.LIB_PATH, REPO), "sites": n, "seqs": int(buf.shape[1]), "runs": []}
    for win in ((64, 128) if what == "small" else (1000,)):
        ctx.set_window(0, win)
        K = ctx.matrix_banded_width()
        band = torch.empty((n, K + 1), dtype=torch.float32, device="cuda:0")
        ctx.run_matrix_banded(stat="r", zero_missing=True, out=band)
        F = torch.empty((n, K + 1), dtype=torch.float64, device="cuda:0")
        big = what == "million"
        ridge, ms, info = factor(ctx, band, F, 3 if big else 10, 1 if big else 3)
        r = {"bandwidth": K, "ridge": ridge, "factor": stats(ms), "min_pivot": info.min_pivot, "launches": launches(n, K),
             "factor_bytes": n * (K + 1) * 8, "logdet": W.banded_logdet(F),
             "solve": solve_ms(ctx, torch, F, n, COLS, 3 if big else 10, 1 if big else 3, g)}
        r["us_per_launch"] = 1e3 * r["factor"]["ms"] / r["launches"]
        if what == "factor20k":
            # the dense arm: the same matrix in float64, torch's factorisation and solves
            dense = torch.zeros((n, n), dtype=torch.float64, device="cuda:0")
            for k in range(K + 1):
                dense.diagonal(k).copy_(band[:n - k, k])
            dense = dense + dense.T - torch.diag(dense.diagonal().clone())
            dense.diagonal().add_(ridge)
            Lt = [None]

            def dense_factor():
                Lt[0], bad = torch.linalg.cholesky_ex(dense)
                return bad

            assert int(dense_factor()) == 0
            r["torch_factor"] = stats(events(torch, dense_factor, 3, 1))
            r["logdet_torch"] = 2.0 * float(Lt[0].diagonal().log().sum())
            for c in COLS:
                b = torch.rand((n, c), generator=torch.Generator(device="cuda:0").manual_seed(11), device="cuda:0",
                               dtype=torch.float64) - 0.4
                r["solve"][str(c)]["torch"] = stats(events(torch, lambda: torch.cholesky_solve(b, Lt[0]), 5, 2))
                x = ctx.banded_solve(F, b)
                ref = torch.cholesky_solve(b, Lt[0])
                r["solve"][str(c)]["rel_diff_vs_torch"] = float((x - ref).abs().max() / ref.abs().max())
            del Lt, dense
            b = torch.rand((n,), generator=g, device="cuda:0", dtype=torch.float64) - 0.4
            cg = []
            for _ in range(3):
                cg += events(torch, lambda: W.banded_cg_solve(ctx.banded_apply, band, b, ridge=ridge, tol=1e-8), 1, 0)
            x_cg, it, res, ok = W.banded_cg_solve(ctx.banded_apply, band, b, ridge=ridge, tol=1e-8)
            x = ctx.banded_solve(F, b)
            r["cg"] = dict(stats(cg), iterations=it, residual=res, converged=bool(ok),
                           rel_diff=float((x - x_cg).abs().max() / x.abs().max()))
        rec["runs"].append(r)
        del band, F
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


def summary(args):
    for p in args.files:
        rec = json.loads(open(p).read())
        for r in rec["runs"]:
            f = r["factor"]
            print("%s: %d sites, bandwidth %d, ridge %g, factor %.2f GB" %
                  (rec["what"], rec["sites"], r["bandwidth"], r["ridge"], r["factor_bytes"] / 1e9))
            print("  factor %9.3f ms (min %.3f, max %.3f), %d launches, %.2f us per launch, min pivot %.3g" %
                  (f["ms"], f["ms_min"], f["ms_max"], r["launches"], r["us_per_launch"], r["min_pivot"]))
            if "torch_factor" in r:
                t = r["torch_factor"]
                print("  torch.linalg.cholesky_ex (f64 dense) %9.3f ms (min %.3f, max %.3f): banded / torch = %.4f" %
                      (t["ms"], t["ms_min"], t["ms_max"], f["ms"] / t["ms"]))
            for c, s in r["solve"].items():
                line = "  solve n_cols %-3s %9.3f ms (min %.3f, max %.3f)" % (c, s["banded"]["ms"], s["banded"]["ms_min"],
                                                                             s["banded"]["ms_max"])
                if "torch" in s:
                    line += "; torch.cholesky_solve %.3f ms: banded / torch = %.3f; max |diff| / max |x| %.2e" % (
                        s["torch"]["ms"], s["banded"]["ms"] / s["torch"]["ms"], s["rel_diff_vs_torch"])
                print(line)
            if "cg" in r:
                c = r["cg"]
                print("  banded_cg_solve to 1e-8: %.3f ms, %d iterations, residual %.2e, converged %s; solve / cg = %.4f; "
                      "max |diff| / max |x| %.2e" % (c["ms"], c["iterations"], c["residual"], c["converged"],
                                                     r["solve"]["1"]["banded"]["ms"] / c["ms"], c["rel_diff"]))
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("run")
    a.add_argument("--what", required=True, choices=WHATS)
    a.add_argument("--cache")
    a.add_argument("--out")
    b = sub.add_parser("summary")
    b.add_argument("files", nargs="+")
    ns = ap.parse_args()
    sys.exit(run(ns) if ns.cmd == "run" else summary(ns))
