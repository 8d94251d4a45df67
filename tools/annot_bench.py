#!/usr/bin/env python3
"""What the partitioned LD scores' epilogue (two f64 matrix products and up to
128 C f64 atomics per tile) costs against the summary's: the launch of
Context.run_annot_scores (kernel_ms) for dense random annotations of C = 1,
16, 64 and 128 columns and for a 64-column one-hot matrix (the zero-chunk skip
path), against the summary launch (Context.run_summary's kernel_ms, no bins)
on bench.synth(20000, 2000) with Henikoff weights, warm, medians of 10; and
end to end on bench.ld_blocks(5000, 500) with C = 64, run_annot_scores against
run_host(-1.0) (every pair as a row, copied to the host) plus the host's
scatter of the rows into a dense matrix and its product with the annotations.

    python tools/annot_bench.py run --what summary|annot1|annot16|annot64|annot128|onehot64|e2e_rows|e2e_annot
                                    [--tree DIR] --cache FILE --out FILE      one measurement; one JSON line
    python tools/annot_bench.py summary FILE...                    the table, and the check

Each run is a process of its own (tools/annot_bench.sh gives each its own time
limit and interleaves the two sides); --tree DIR imports weightedld_amd
(package and built library) from another checkout, so the baseline can be the
parent commit's build on the same device.  The summary fails unless every
C = 1 launch is within 1.10 x the median summary launch; the larger C are
reported with the cost per column they imply.
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
L2, N2, C2 = 5000, 500, 64
WHATS = ["summary", "annot1", "annot16", "annot64", "annot128", "onehot64", "e2e_rows", "e2e_annot"]


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


def annotations(what, n_sites):
    if what == "onehot64":  # 64 runs of consecutive sites: a tile's sites lie in one or two columns
        a = np.zeros((n_sites, 64), dtype=np.float32)
        a[np.arange(n_sites), np.arange(n_sites) * 64 // n_sites] = 1.0
        return a
    c = C2 if what.startswith("e2e") else int(what[len("annot"):])
    return np.random.default_rng(0xA0 + c).standard_normal((n_sites, c)).astype(np.float32)


def run(args):
    if args.tree:
        sys.path.insert(0, os.path.abspath(args.tree))
    import weightedld_amd as W
    e2e = args.what.startswith("e2e")
    buf, w = data("ld_blocks", L2, N2, args.cache) if e2e else data("synth", L, N, args.cache)
    ctx = W.Context(0)
    ctx.load(buf, w)
    rec = {"what": args.what, "lib": W.LIB_PATH, "sites": int(buf.shape[0]), "seqs": int(buf.shape[1])}
    if args.what == "summary":
        for _ in range(WARMUP):
            ctx.run_summary()
        ms = []
        for _ in range(STEPS):
            s = ctx.run_summary()
            ms.append(s.kernel_ms)
        rec.update(pairs=s.pairs, counted_pairs=s.counted_pairs)
    elif not e2e:
        a = annotations(args.what, buf.shape[0])
        for _ in range(WARMUP):
            ctx.run_annot_scores(a)
        ms = []
        for _ in range(STEPS):
            s = ctx.run_annot_scores(a)
            ms.append(s.kernel_ms)
        rec.update(pairs=s.pairs, counted_pairs=s.counted_pairs, columns=int(a.shape[1]), tiles=s.tiles)
    else:
        a = annotations(args.what, buf.shape[0])

        def rows_then_numpy():
            r = ctx.run_host(-1.0)
            keep = np.isfinite(r.r2)
            x = np.zeros((buf.shape[0], buf.shape[0]))
            x[r.site_a[keep], r.site_b[keep]] = r.r2[keep]
            x[r.site_b[keep], r.site_a[keep]] = r.r2[keep]
            return x @ a.astype(np.float64)

        call = rows_then_numpy if args.what == "e2e_rows" else (lambda: ctx.run_annot_scores(a).score)
        call()
        ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            score = call()
            ms.append((time.perf_counter() - t0) * 1e3)
        rec.update(columns=C2, checksum=float(np.abs(score).sum()))
    rec.update(ms=float(np.median(ms)), ms_min=float(min(ms)), ms_max=float(max(ms)), steps=len(ms))
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


def summary(args):
    recs = [json.loads(open(p).read()) for p in args.files]
    print("%-10s %10s %10s %10s  %s" % ("what", "ms", "min", "max", "library"))
    for r in recs:
        print("%-10s %10.3f %10.3f %10.3f  %s" % (r["what"], r["ms"], r["ms_min"], r["ms_max"], r["lib"]))
    base = [r["ms"] for r in recs if r["what"] == "summary"]
    ok = True
    if base:
        base = float(np.median(base))
        print("summary launch: median %.3f ms over the runs; limit for C = 1: 1.10 x = %.3f ms" % (base, 1.10 * base))
        med = {}
        for r in recs:
            if r["what"].startswith("annot") or r["what"] == "onehot64":
                med.setdefault(r["what"], []).append(r["ms"])
                if r["what"] == "annot1":
                    good = r["ms"] <= 1.10 * base
                    ok = ok and good
                    print("  annot1     %.3f ms = %.3f x  %s" % (r["ms"], r["ms"] / base, "ok" if good else "MISSED"))
        med = {k: float(np.median(v)) for k, v in med.items()}
        for k in ("annot16", "annot64", "annot128", "onehot64"):
            if k in med:
                cols = 64 if k == "onehot64" else int(k[len("annot"):])
                print("  %-10s %.3f ms = %.3f x; %.4f ms per column over the summary" %
                      (k, med[k], med[k] / base, (med[k] - base) / cols))
    x = [r["ms"] for r in recs if r["what"] == "e2e_rows"]
    y = [r["ms"] for r in recs if r["what"] == "e2e_annot"]
    if x and y:
        print("end to end, %d sites, %d columns: run_host(-1.0) + numpy %.1f ms, run_annot_scores %.1f ms (%.0f x)" %
              (L2, C2, np.median(x), np.median(y), np.median(x) / np.median(y)))
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
