#!/bin/bash
# Target-site LD against the row path's routes to the same answer
# (tools/targets_bench.py), the two sides interleaved, each run a process under
# its own time limit, then the tables.
#   tools/targets_bench.sh [OUTDIR] [BASELINE_TREE]
# BASELINE_TREE: the checkout whose built weightedld_amd the row-path runs
# import (the parent commit's; default: this tree).
out=${1:-targets_bench_out}; mkdir -p "$out"
base=${2:-}
tmp=$(mktemp -d)
step() {  # name what data [tree]
    timeout -k 10 240 python3 tools/targets_bench.py run --what "$2" --data "$3" ${4:+--tree "$4"} \
        --cache "$tmp/$3.npz" --out "$out/$1.json"
}
step hbm hbm synth &&
    step s_rows1 rows synth "$base" && step s_tg1 targets synth && step s_rows2 rows synth "$base" &&
    step s_tg2 targets synth && step s_e2e e2e_rows synth "$base" &&
    step l_rows1 rows ld_blocks "$base" && step l_tg1 targets ld_blocks && step l_rows2 rows ld_blocks "$base" &&
    step l_tg2 targets ld_blocks && step l_e2e e2e_rows ld_blocks "$base" &&
    python3 tools/targets_bench.py summary "$out"/*.json | tee "$out/summary.txt"
rc=${PIPESTATUS[0]}
rm -rf "$tmp"
exit $rc
