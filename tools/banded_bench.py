#!/usr/bin/env python3
"""What band storage costs and buys: on bench.synth(20000, 2000) with Henikoff
weights under max_sites 1,000, warm, medians of 10,

  * the band fill — Context.run_matrix_banded into a [20000, 1001] float32
    device tensor (kernel_ms: fill + pair launch) — against run_matrix of the
    same tree under the same window into the 20,000-site square (the same
    tiles, twenty times the bytes);
  * the band product — Context.banded_apply of that band with n_cols = 1, 16,
    64 float32 columns (host clock around the call, which ends in a stream
    synchronise) — against torch's matmul of the dense run_matrix tensor
    (float32, and float64 as the band product accumulates), the two
    alternating in one process, and against its byte model (the band twice,
    X once, Y once) at the HBM rate a streaming kernel reaches;
  * one size the dense call cannot do: 1,000,000 x 200 synthetic sites under
    max_sites 1,000: the band fill, the product and the device memory in use.

    python tools/banded_bench.py run --what WHAT --cache FILE --out FILE     one measurement; one JSON line
    python tools/banded_bench.py summary FILE...                             the tables

Each run is a process of its own (tools/banded_bench.sh gives each its own
time limit and interleaves the dense and the band fill)."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
L, N, STEPS, WARMUP = 20000, 2000, 10, 3
LM, NM = 1000000, 200
WIN = 1000
COLS = (1, 16, 64)
HBM_BYTES_PER_S = 6.3e12  # what a streaming kernel reaches on MI355X (8 TB/s nominal)
WHATS = ["win_dense", "win_banded", "apply", "million"]


def data(n_sites, n_seqs, cache):
    import bench
    import weightedld_amd as W
    if cache and os.path.exists(cache):
        z = np.load(cache)
        return z["buf"], z["w"]
    buf = bench.synth(n_sites, n_seqs)
    w = W.henikoff_weights(W.SiteSet.from_buffer(buf))
    if cache:
        np.savez(cache, buf=buf, w=w)
    return buf, w


def timed(call, sync, steps=STEPS, warmup=WARMUP):
    for _ in range(warmup):
        call()
    sync()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        call()
        sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def stats(ms):
    return {"ms": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)), "steps": len(ms)}


def model_ms(n, K, band_bytes_per, c, x_bytes_per):
    return (2.0 * n * (K + 1) * band_bytes_per + n * c * x_bytes_per + n * c * 8) / HBM_BYTES_PER_S * 1e3


def run(args):
    import torch
    import weightedld_amd as W
    what = args.what
    big = what == "million"
    buf, w = data(LM, NM, None) if big else data(L, N, args.cache)
    n = int(buf.shape[0])
    ctx = W.Context(0)
    ctx.load(buf, w)
    ctx.set_window(0, WIN)
    K = ctx.matrix_banded_width()
    rec = {"what": what, "lib": W.LIB_PATH, "sites": n, "seqs": int(buf.shape[1]), "bandwidth": K}
    sync = lambda: torch.cuda.synchronize()  # noqa: E731
    if what in ("win_dense", "win_banded"):
        shape = (n, n) if what == "win_dense" else (n, K + 1)
        out = torch.empty(shape, dtype=torch.float32, device="cuda:0")
        call = (lambda: ctx.run_matrix(stat="r", out=out)[1]) if what == "win_dense" else \
            (lambda: ctx.run_matrix_banded(stat="r", out=out)[1])
        for _ in range(WARMUP):
            call()
        ms = []
        for _ in range(STEPS):
            s = call()
            ms.append(s.kernel_ms)
        rec.update(stats(ms), pairs=s.pairs, tiles=s.tiles, bytes=int(out.numel()) * 4,
                   checksum=float(torch.nan_to_num(out).abs().sum(dtype=torch.float64)))
    elif what == "apply":
        band = torch.empty((n, K + 1), dtype=torch.float32, device="cuda:0")
        dense = torch.empty((n, n), dtype=torch.float32, device="cuda:0")
        ctx.run_matrix_banded(stat="r", zero_missing=True, out=band)
        ctx.run_matrix(stat="r", zero_missing=True, out=dense)
        dense64 = dense.double()
        band16 = band.half()
        g = torch.Generator(device="cuda:0").manual_seed(7)
        rec["cols"] = {}
        for c in COLS:
            X = torch.rand((n, c), generator=g, device="cuda:0", dtype=torch.float32) - 0.4
            X64 = X.double()
            Y = torch.empty((n, c), dtype=torch.float64, device="cuda:0")
            arms = {"banded_f32": lambda: ctx.banded_apply(band, X, out=Y),
                    "banded_f16": lambda: ctx.banded_apply(band16, X, out=Y),
                    "banded_x64": lambda: ctx.banded_apply(band, X64, out=Y),
                    "torch_f32": lambda: torch.matmul(dense, X),
                    "torch_f64": lambda: torch.matmul(dense64, X64)}
            ms = {k: [] for k in arms}
            for k in arms:  # warm
                timed(arms[k], sync, steps=1)
            for _ in range(STEPS):  # interleaved
                for k in arms:
                    ms[k] += timed(arms[k], sync, steps=1, warmup=0)
            ref = torch.matmul(dense64, X64)
            err = float((ctx.banded_apply(band, X) - ref).abs().max() / ref.abs().max())
            rec["cols"][str(c)] = {"arms": {k: stats(v) for k, v in ms.items()}, "rel_diff_vs_torch_f64": err,
                                   "model_ms_f32": model_ms(n, K, 4, c, 4), "model_ms_f16": model_ms(n, K, 2, c, 4),
                                   "model_ms_x64": model_ms(n, K, 4, c, 8)}
        rec.update(ms=0.0, ms_min=0.0, ms_max=0.0, steps=STEPS, band_bytes=n * (K + 1) * 4, dense_bytes=n * n * 4)
    else:
        free0, total = torch.cuda.mem_get_info()
        band = torch.empty((n, K + 1), dtype=torch.float32, device="cuda:0")
        fill = []
        for _ in range(3):
            _, s = ctx.run_matrix_banded(stat="r", zero_missing=True, out=band)
            fill.append(s.kernel_ms)
        free1, _ = torch.cuda.mem_get_info()
        rec.update(stats(fill), pairs=s.pairs, tiles=s.tiles, band_bytes=n * (K + 1) * 4,
                   device_bytes_in_use=int(total - free1), device_bytes_before_band=int(total - free0), cols={})
        g = torch.Generator(device="cuda:0").manual_seed(7)
        for c in (1, 16):
            X = torch.rand((n, c), generator=g, device="cuda:0", dtype=torch.float32) - 0.4
            Y = torch.empty((n, c), dtype=torch.float64, device="cuda:0")
            ms = timed(lambda: ctx.banded_apply(band, X, out=Y), sync, steps=5, warmup=2)
            rec["cols"][str(c)] = {"arms": {"banded_f32": stats(ms)}, "model_ms_f32": model_ms(n, K, 4, c, 4),
                                   "checksum": float(Y.abs().sum())}
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


def summary(args):
    recs = [json.loads(open(p).read()) for p in args.files]

    def of(what):
        return [r for r in recs if r["what"] == what]

    print("%-12s %10s %10s %10s %14s" % ("fill", "ms", "min", "max", "bytes"))
    for r in of("win_dense") + of("win_banded"):
        print("%-12s %10.3f %10.3f %10.3f %14d" % (r["what"], r["ms"], r["ms_min"], r["ms_max"], r["bytes"]))
    d, b = [r["ms"] for r in of("win_dense")], [r["ms"] for r in of("win_banded")]
    if d and b:
        spread = max(d) - min(d)
        verdict = "not slower" if np.median(b) <= np.median(d) + spread else "SLOWER beyond the dense call's spread"
        print("max_sites %d: dense %.3f ms (spread of its runs %.3f), banded %.3f ms = %.3f x: %s" %
              (WIN, np.median(d), spread, np.median(b), np.median(b) / np.median(d), verdict))
    for r in of("apply") + of("million"):
        print("%s: %d sites, bandwidth %d, band %.2f GB" % (r["what"], r["sites"], r["bandwidth"], r["band_bytes"] / 1e9))
        if r["what"] == "million":
            print("  fill %.1f ms (min %.1f, max %.1f), %d tiles; device memory in use %.2f GB (%.2f GB before the band)" %
                  (r["ms"], r["ms_min"], r["ms_max"], r["tiles"], r["device_bytes_in_use"] / 1e9,
                   r["device_bytes_before_band"] / 1e9))
        for c, x in r["cols"].items():
            for k, v in x["arms"].items():
                model = x.get({"banded_f32": "model_ms_f32", "banded_f16": "model_ms_f16", "banded_x64": "model_ms_x64"}.get(k, ""))
                print("  n_cols %-3s %-11s %9.3f ms (min %.3f, max %.3f)%s" %
                      (c, k, v["ms"], v["ms_min"], v["ms_max"],
                       "  byte model %.3f ms: %.0f %% of it" % (model, 100.0 * model / v["ms"]) if model else ""))
            a = x["arms"]
            if "torch_f32" in a:
                print("  n_cols %-3s banded_f32 / torch_f32 = %.3f, / torch_f64 = %.3f; max |diff| / max |Y| vs torch f64 %.2e" %
                      (c, a["banded_f32"]["ms"] / a["torch_f32"]["ms"], a["banded_f32"]["ms"] / a["torch_f64"]["ms"],
                       x["rel_diff_vs_torch_f64"]))
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
