#!/usr/bin/env python3
"""What the LD matrix's epilogue (a 64x64 tile staged in LDS and stored twice,
2 x 4 bytes per pair) costs against the summary's: the launches of
Context.run_matrix into a device tensor (kernel_ms: fill + pair launch) for
the full square in float32 and float16, under a window (max_sites 1,000), for
a block of the square the window leaves empty (the fill alone) and for a
2,000-site square region, against the summary launch (Context.run_summary's
kernel_ms, no bins) on bench.synth(20000, 2000) with Henikoff weights, warm,
medians of 10; and end to end on bench.ld_blocks(5000, 500): run_host(-1.0)
plus the host's scatter of the rows into a symmetric dense r matrix, and
wld_dense, against run_matrix into a device tensor and to the host.

    python tools/matrix_bench.py run --what WHAT [--tree DIR] --cache FILE --out FILE     one measurement; one JSON line
    python tools/matrix_bench.py summary FILE...                    the table, and the 1.10 x statement

Each run is a process of its own (tools/matrix_bench.sh gives each its own
time limit and interleaves the two sides); --tree DIR imports weightedld_amd
(package and built library) from another checkout, so the baseline can be the
parent commit's build on the same device.  The summary states whether the
float32 launch is within 1.10 x the median summary launch (a finding either
way: its exit status is 0), the store rate the launches imply and the fill's.
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
L2, N2 = 5000, 500
WIN = 1000
WHATS = ["summary", "matrix_f32", "matrix_f16", "win_summary", "win_matrix_f32", "win_fill", "region_f32",
         "e2e_rows", "e2e_dense", "e2e_torch", "e2e_host"]


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
    what = args.what
    e2e = what.startswith("e2e")
    buf, w = data("ld_blocks", L2, N2, args.cache) if e2e else data("synth", L, N, args.cache)
    ctx = W.Context(0)
    ctx.load(buf, w)
    if what.startswith("win_"):
        ctx.set_window(0, WIN)
    rec = {"what": what, "lib": W.LIB_PATH, "sites": int(buf.shape[0]), "seqs": int(buf.shape[1])}
    if what in ("summary", "win_summary"):
        for _ in range(WARMUP):
            ctx.run_summary()
        ms = []
        for _ in range(STEPS):
            s = ctx.run_summary()
            ms.append(s.kernel_ms)
        rec.update(pairs=s.pairs, counted_pairs=s.counted_pairs)
    elif not e2e:
        import torch
        rows, cols = {"win_fill": ((0, 8000), (12000, 20000)), "region_f32": ((9000, 11000), (9000, 11000))}.get(
            what, ((0, L), (0, L)))
        dtype = "float16" if what.endswith("f16") else "float32"
        out = torch.empty((rows[1] - rows[0], cols[1] - cols[0]), dtype=getattr(torch, dtype), device="cuda:0")
        for _ in range(WARMUP):
            ctx.run_matrix(rows, cols, "r", dtype, out=out)
        ms = []
        for _ in range(STEPS):
            _, s = ctx.run_matrix(rows, cols, "r", dtype, out=out)
            ms.append(s.kernel_ms)
        rec.update(pairs=s.pairs, counted_pairs=s.counted_pairs, tiles=s.tiles,
                   bytes=int(out.numel()) * int(out.element_size()), checksum=float(torch.nan_to_num(out.float()).abs().sum()))
    else:
        n = buf.shape[0]

        def rows_then_numpy():
            r = ctx.run_host(-1.0)
            s = np.sqrt(r.r2)
            x = np.zeros((n, n), dtype=np.float32)
            x[r.site_a, r.site_b] = np.where(r.d > 0, -s, s)
            x[r.site_b, r.site_a] = x[r.site_a, r.site_b]
            x[np.arange(n), np.arange(n)] = 1.0
            return x

        def to_torch():
            import torch
            out = torch.empty((n, n), dtype=torch.float32, device="cuda:0")
            ctx.run_matrix(stat="r", out=out)
            return out

        call = {"e2e_rows": rows_then_numpy, "e2e_dense": lambda: ctx.dense(n)[2], "e2e_torch": to_torch,
                "e2e_host": lambda: ctx.run_matrix(stat="r")[0]}[what]
        call()
        ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            m = call()
            ms.append((time.perf_counter() - t0) * 1e3)
        if what == "e2e_torch":
            m = m.cpu().numpy()
        rec.update(checksum=float(np.nan_to_num(np.abs(m.astype(np.float64))).sum()))
    rec.update(ms=float(np.median(ms)), ms_min=float(min(ms)), ms_max=float(max(ms)), steps=len(ms))
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


def summary(args):
    recs = [json.loads(open(p).read()) for p in args.files]
    print("%-15s %10s %10s %10s  %s" % ("what", "ms", "min", "max", "library"))
    for r in recs:
        print("%-15s %10.3f %10.3f %10.3f  %s" % (r["what"], r["ms"], r["ms_min"], r["ms_max"], r["lib"]))

    def med(what):
        x = [r["ms"] for r in recs if r["what"] == what]
        return float(np.median(x)) if x else None

    def nbytes(what):
        x = [r["bytes"] for r in recs if r["what"] == what]
        return x[0] if x else 0

    base, wbase = med("summary"), med("win_summary")
    if base:
        print("summary launch: median %.3f ms over the runs; 1.10 x = %.3f ms" % (base, 1.10 * base))
        for k in ("matrix_f32", "matrix_f16"):
            if med(k):
                print("  %-14s %.3f ms = %.3f x%s; %.3f ms over the summary: %.0f GB/s of stores" %
                      (k, med(k), med(k) / base, ("  (within 1.10 x)" if med(k) <= 1.10 * base else "  (EXCEEDS 1.10 x)")
                       if k == "matrix_f32" else "", med(k) - base, nbytes(k) / max(med(k) - base, 1e-9) / 1e6))
    if wbase and med("win_matrix_f32"):
        k = "win_matrix_f32"
        print("max_sites %d: summary %.3f ms, matrix %.3f ms (%.3f x; the whole square is written: %.0f GB/s overall)" %
              (WIN, wbase, med(k), med(k) / wbase, nbytes(k) / med(k) / 1e6))
    if med("win_fill"):
        print("fill alone (8,000 x 8,000 out of the window): %.3f ms, %.0f GB/s" %
              (med("win_fill"), nbytes("win_fill") / med("win_fill") / 1e6))
    if med("region_f32"):
        print("2,000-site square region: %.3f ms" % med("region_f32"))
    e = {k: med(k) for k in ("e2e_rows", "e2e_dense", "e2e_torch", "e2e_host")}
    if all(e.values()):
        print("end to end, %d sites: run_host(-1.0) + numpy %.1f ms, wld_dense %.1f ms, run_matrix -> device tensor "
              "%.2f ms (%.0f x), run_matrix -> host %.1f ms (%.1f x)" %
              (L2, e["e2e_rows"], e["e2e_dense"], e["e2e_torch"], e["e2e_rows"] / e["e2e_torch"], e["e2e_host"],
               e["e2e_rows"] / e["e2e_host"]))
    return 0


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
