#!/bin/bash
# GPU box: the full bench line (every leg of --full), then the sharded path at N = 1 (rehearsal), logs under $OUT.
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
TAG=${1:-r04}
timeout -k 10 400 python3 bench.py --full --steps 20 --warmup 5 > "$OUT/bench_${TAG}.json" 2> "$OUT/bench_${TAG}.err" || exit $?
tail -3 "$OUT/bench_${TAG}.err"
timeout -k 10 400 python3 -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 \
    --master-port 29533 bench.py --gpus 1 --sharded --full --steps 20 --warmup 5 --cpu-baseline off \
    > "$OUT/bench_${TAG}_sharded.json" 2> "$OUT/bench_${TAG}_sharded.err"
rc=$?
tail -3 "$OUT/bench_${TAG}_sharded.err"
exit $rc
