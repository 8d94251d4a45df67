#!/bin/bash
# LD pruning on the device against the host route (tools/prune_bench.py): per
# case the two routes, each run a process under its own time limit, then the
# table and the check that both routes kept the same sites.
#   tools/prune_bench.sh [OUTDIR]
out=${1:-prune_bench_out}; mkdir -p "$out"
tmp=$(mktemp -d)
step() {  # case route
    case $1 in synth) c=synth ;; *) c=blocks ;; esac
    timeout -k 10 300 python3 tools/prune_bench.py run --case "$1" --route "$2" \
        --cache "$tmp/$c.npz" --out "$out/$1_$2.json"
}
step blocks device && step blocks host && step blocks_win device && step blocks_win host &&
    step synth device && step synth host &&
    python3 tools/prune_bench.py summary "$out"/*.json | tee "$out/summary.txt"
rc=${PIPESTATUS[0]}
rm -rf "$tmp"
exit $rc
