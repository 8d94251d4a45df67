#!/usr/bin/env python3
"""C4 passes (default options; WLD_AB_OPTS as tools/ab_builds.py) on the library of WLD_LIB_PATH, for a rocprofv3 --pmc run of their own; prints the last pass's stats.
    python tools/fp6_c4_passes.py [passes]"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402,F401

import bench  # noqa: E402
import weightedld_amd as W  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4
N, L, thr, _ = bench.CONFIGS["c4"]
buf = bench.synth(L, N)
w = W.henikoff_weights(W.SiteSet.from_buffer(buf))
ctx = W.Context(0, W.KERNEL_MFMA)
for kv in filter(None, os.environ.get("WLD_AB_OPTS", "").split(";")):
    ctx.set_option(kv.split("=", 1)[0], int(kv.split("=", 1)[1]))
ctx.load(buf, w)
for _ in range(n):
    rows = ctx.run(thr)
st = ctx.stats()
print(json.dumps({"lib": os.environ.get("WLD_LIB_PATH"), "rows": rows,
                  **{k: st[k] for k in ("screen_ms", "pair_kernel_ms", "screen_fp6", "fp6_three", "fp6_quick",
                                        "fp6_quick_full", "fp6_rechecked", "fp6_shared", "candidate_tiles", "tiles")}}))
ctx.close()
