#!/bin/bash
# The LD matrix launch against the summary launch (tools/matrix_bench.py), the
# two sides interleaved, each run a process under its own time limit, then the
# table and the 1.10 x statement.
#   tools/matrix_bench.sh [OUTDIR] [BASELINE_TREE]
# BASELINE_TREE: the checkout whose built weightedld_amd the summary, the
# end-to-end row runs and wld_dense import (the parent commit's; default: this
# tree).
out=${1:-matrix_bench_out}; mkdir -p "$out"
base=${2:-}
tmp=$(mktemp -d)
step() {  # name what [tree]
    case $2 in e2e*) c=ldb ;; *) c=c4 ;; esac
    timeout -k 10 300 python3 tools/matrix_bench.py run --what "$2" ${3:+--tree "$3"} \
        --cache "$tmp/$c.npz" --out "$out/$1.json"
}
step sum1 summary "$base" && step m32_1 matrix_f32 && step sum2 summary "$base" && step m16_1 matrix_f16 &&
    step m32_2 matrix_f32 && step sum3 summary "$base" && step m16_2 matrix_f16 && step m32_3 matrix_f32 &&
    step wsum win_summary "$base" && step wm32 win_matrix_f32 && step wfill win_fill && step reg region_f32 &&
    step e2e_rows e2e_rows "$base" && step e2e_dense e2e_dense "$base" && step e2e_torch e2e_torch &&
    step e2e_host e2e_host &&
    python3 tools/matrix_bench.py summary "$out"/*.json | tee "$out/summary.txt"
rc=${PIPESTATUS[0]}
rm -rf "$tmp"
exit $rc
