#!/bin/bash
# The banded LD matrix's fill against the dense fill under the same window (the
# two interleaved), the band product against torch's matmul of the dense
# matrix and its byte model, and the million-site band
# (tools/banded_bench.py); each run a process under its own time limit, then
# the tables (of whatever ran: the first failing step ends the GPU work).
#   tools/banded_bench.sh [OUTDIR]
out=${1:-banded_bench_out}; mkdir -p "$out"
tmp=$(mktemp -d)
step() {  # name what [seconds]
    timeout -k 10 "${3:-300}" python3 tools/banded_bench.py run --what "$2" --cache "$tmp/c4.npz" --out "$out/$1.json"
}
step dense1 win_dense && step band1 win_banded && step dense2 win_dense && step band2 win_banded &&
    step dense3 win_dense && step band3 win_banded && step apply apply && step million million 600
rc=$?
rm -rf "$tmp"
python3 tools/banded_bench.py summary "$out"/*.json | tee "$out/summary.txt"
exit $rc
