#!/usr/bin/env python3
"""In-kernel clock of the tile-pair fp6 screen from a -DWLD_EXP_CLOCK build
(tools/build_variant.sh): wave 0 of each workgroup stamps s_memtime (shader
cycles) and s_memrealtime (100 MHz) around the stage loop.  Runs the bench
config back to back for SECONDS (default 2), then reports, over the last
launch's workgroups, the median clock (GHz) and the loop's cycles and
microseconds; screen_ms / pair_kernel_ms are the last run's event times.
    python tools/fp6_clock.py LIB [config] [seconds]"""
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402,F401

import weightedld_amd._lib as _L  # noqa: E402
_L.LIB_PATH = os.path.abspath(sys.argv[1])
import bench  # noqa: E402
import weightedld_amd as W  # noqa: E402

cfg = sys.argv[2] if len(sys.argv) > 2 else "c4"
secs = float(sys.argv[3]) if len(sys.argv) > 3 else 2.0
N, L, thr, _ = bench.CONFIGS[cfg]
buf = bench.synth(L, N)
w = W.henikoff_weights(W.SiteSet.from_buffer(buf))
ctx = W.Context(0, W.KERNEL_MFMA)
ctx.set_option("screen_fp6", 2)  # forced: the pass completes on fp6 whatever the candidate count
for kv in filter(None, os.environ.get("WLD_AB_OPTS", "").split(";")):  # opt=v;opt=v, as tools/ab_builds.py
    ctx.set_option(kv.split("=", 1)[0], int(kv.split("=", 1)[1]))
ctx.load(buf, w)
t0, runs = time.time(), 0
while time.time() - t0 < secs or runs < 3:
    ctx.run(thr)
    runs += 1
st = ctx.stats()
K = 8192
arr = (ctypes.c_ulonglong * (2 * K))()
fn = W.lib().wld_debug_f6_clock
fn.argtypes = [ctypes.POINTER(ctypes.c_ulonglong)]
assert fn(arr) == 0
a = np.frombuffer(arr, dtype=np.uint64).reshape(K, 2).astype(np.float64)
a = a[a[:, 1] > 0]
ghz = a[:, 0] / a[:, 1] * 0.1
print(json.dumps({"lib": sys.argv[1], "config": cfg, "runs": runs, "slots": int(len(a)),
                  "clock_ghz_med": float(np.median(ghz)), "clock_ghz_p10": float(np.percentile(ghz, 10)),
                  "clock_ghz_p90": float(np.percentile(ghz, 90)), "loop_cycles_med": float(np.median(a[:, 0])),
                  "loop_us_med": float(np.median(a[:, 1]) / 100.0), "screen_ms": st["screen_ms"],
                  "pair_kernel_ms": st["pair_kernel_ms"], "candidate_tiles": st["candidate_tiles"],
                  "tiles": st["tiles"], "screen_fp6": st["screen_fp6"], "fp6_three": st["fp6_three"],
                  "fp6_rechecked": st["fp6_rechecked"]}))
