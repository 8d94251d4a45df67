#!/bin/bash
# The best-partner run against the row path's every-tile launch
# (tools/partners_bench.py) on both data sets, the two sides interleaved, each
# run a process under its own time limit, then the table and the 1.10 x check
# of k = 8 at threshold -1.
#   tools/partners_bench.sh [OUTDIR] [BASELINE_TREE]
# BASELINE_TREE: the checkout whose built weightedld_amd the row-path runs
# import (the parent commit's; default: this tree).
out=${1:-partners_bench_out}; mkdir -p "$out"
base=${2:-}
tmp=$(mktemp -d)
step() {  # data what run [tree]
    timeout -k 10 300 python3 tools/partners_bench.py run --data "$1" --what "$2" ${4:+--tree "$4"} \
        --cache "$tmp/$1.npz" --out "$out/$1_$2_$3.json"
}
side() {  # data
    step "$1" rows 1 "$base" && step "$1" k8 1 && step "$1" rows 2 "$base" && step "$1" k8 2 &&
        step "$1" k1 1 && step "$1" k64 1 && step "$1" k8_t02 1 && step "$1" e2e_rows 1 "$base"
}
side synth && side ldb && python3 tools/partners_bench.py summary "$out"/*.json | tee "$out/summary.txt"
rc=${PIPESTATUS[0]}
rm -rf "$tmp"
exit $rc
