#!/bin/bash
# The summary launch against the row path's every-tile launch
# (tools/summary_bench.py), the two sides interleaved, each run a process under
# its own time limit, then the table and the 1.10 x check.
#   tools/summary_bench.sh [OUTDIR] [BASELINE_TREE]
# BASELINE_TREE: the checkout whose built weightedld_amd the row-path runs
# import (the parent commit's; default: this tree).
out=${1:-summary_bench_out}; mkdir -p "$out"
base=${2:-}
tmp=$(mktemp -d)
step() {  # name what [tree]
    case $2 in e2e*) c=ldb ;; *) c=c4 ;; esac
    timeout -k 10 300 python3 tools/summary_bench.py run --what "$2" ${3:+--tree "$3"} \
        --cache "$tmp/$c.npz" --out "$out/$1.json"
}
step rows1 rows "$base" && step sum1 summary && step rows2 rows "$base" && step bins1 summary_bins &&
    step rows3 rows "$base" && step sum2 summary && step bins2 summary_bins &&
    step e2e_rows e2e_rows "$base" && step e2e_sum e2e_summary &&
    python3 tools/summary_bench.py summary "$out"/*.json | tee "$out/summary.txt"
rc=${PIPESTATUS[0]}
rm -rf "$tmp"
exit $rc
