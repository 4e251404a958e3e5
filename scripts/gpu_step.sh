#!/bin/bash
TAG=${1:-step}
O=${OUT_DIR:-bench_outputs}; mkdir -p $O
timeout 420 python bench.py --full --steps 20 --warmup 8 --no-cpu-baseline --kernels new > $O/${TAG}_new.json 2> $O/${TAG}_new.err; cut -c1-220 $O/${TAG}_new.json
