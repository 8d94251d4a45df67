#!/bin/bash
# The heat-map launch against the row path's every-tile launch
# (tools/heatmap_bench.py), the two sides interleaved, each run a process under
# its own time limit, then the table and the 1.10 x check.
#   tools/heatmap_bench.sh [OUTDIR] [BASELINE_TREE]
# BASELINE_TREE: the checkout whose built weightedld_amd the row-path runs
# import (the parent commit's; default: this tree).
out=${1:-heatmap_bench_out}; mkdir -p "$out"
base=${2:-}
tmp=$(mktemp -d)
step() {  # name what [tree]
    case $2 in e2e*) c=ldb ;; *) c=c4 ;; esac
    timeout -k 10 300 python3 tools/heatmap_bench.py run --what "$2" ${3:+--tree "$3"} \
        --cache "$tmp/$c.npz" --out "$out/$1.json"
}
step rows1 rows "$base" && step r2_1 heat256_r2 && step rows2 rows "$base" && step dp_1 heat256_dprime &&
    step rows3 rows "$base" && step r2_2 heat256_r2 && step dp_2 heat256_dprime &&
    step region region && step fine heat4096 &&
    step e2e_rows e2e_rows "$base" && step e2e_heat e2e_heat &&
    python3 tools/heatmap_bench.py summary "$out"/*.json | tee "$out/summary.txt"
rc=${PIPESTATUS[0]}
rm -rf "$tmp"
exit $rc
