#!/bin/bash
# A/B of prover scheduling knobs on one box (bench.py --full, 2^22 proof); results in $OUT_DIR/ab/
set -e
O=${OUT_DIR:-bench_out}/ab
mkdir -p $O
run() { name=$1; shift; env "$@" timeout -k 10 120 python bench.py --full --cpu-baseline 0 --steps 8 --warmup 2 > $O/$name.log 2>&1; }
for cfg in "$@"; do
  name=${cfg%%:*}; vars=${cfg#*:}
  run "$name" $vars
done
