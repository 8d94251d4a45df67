#!/bin/bash
# The partitioned-score launch against the summary launch (tools/annot_bench.py),
# the two sides interleaved, each run a process under its own time limit, then
# the table and the 1.10 x check of C = 1.
#   tools/annot_bench.sh [OUTDIR] [BASELINE_TREE]
# BASELINE_TREE: the checkout whose built weightedld_amd the summary and the
# end-to-end row runs import (the parent commit's; default: this tree).
out=${1:-annot_bench_out}; mkdir -p "$out"
base=${2:-}
tmp=$(mktemp -d)
step() {  # name what [tree]
    case $2 in e2e*) c=ldb ;; *) c=c4 ;; esac
    timeout -k 10 300 python3 tools/annot_bench.py run --what "$2" ${3:+--tree "$3"} \
        --cache "$tmp/$c.npz" --out "$out/$1.json"
}
step sum1 summary "$base" && step a1_1 annot1 && step sum2 summary "$base" && step a16 annot16 &&
    step a1_2 annot1 && step a64 annot64 && step sum3 summary "$base" && step a128 annot128 &&
    step hot64 onehot64 && step a1_3 annot1 &&
    step e2e_rows e2e_rows "$base" && step e2e_annot e2e_annot &&
    python3 tools/annot_bench.py summary "$out"/*.json | tee "$out/summary.txt"
rc=${PIPESTATUS[0]}
rm -rf "$tmp"
exit $rc
