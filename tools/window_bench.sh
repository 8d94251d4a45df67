#!/bin/bash
# What a window buys (tools/window_bench.py): the unwindowed step and
# max_sites 256, 1000, 4000 on the linkage-block set at BASELINE config 4's
# size, each run a process under its own time limit, then the table.
#   tools/window_bench.sh [OUTDIR]   (default window_bench_out)
out=${1:-window_bench_out}; mkdir -p "$out"
cache=$(mktemp -d)/ldb_c4.npz
step() { timeout -k 10 300 python3 tools/window_bench.py run --sites "$1" --cache "$cache" --out "$out/k$1.json"; }
step 0 && step 256 && step 1000 && step 4000 &&
    python3 tools/window_bench.py summary "$out"/k0.json "$out"/k256.json "$out"/k1000.json "$out"/k4000.json | tee "$out/summary.txt"
rc=${PIPESTATUS[0]}
rm -rf "$(dirname "$cache")"
exit $rc
