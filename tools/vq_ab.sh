#!/bin/bash
# Vert QP work aid: bit-identity hashes + config4v throughput in one GPU call.  usage: bash tools/vq_ab.sh <tag>
set -e
tag=${1:-x}
OUT_DIR=${OUT_DIR:-out}
mkdir -p $OUT_DIR/vq
python tools/state_hash.py --batch 512 --steps 60 vertbox vertbox4 config4v > $OUT_DIR/vq/hash_$tag.txt 2>&1
cat $OUT_DIR/vq/hash_$tag.txt
python bench.py --full --workload config4v --no-continuous --no-cpu-baseline --min-seconds 3 > $OUT_DIR/vq/bench_$tag.json 2> $OUT_DIR/vq/bench_$tag.err
python -c "
import json; d=json.load(open('$OUT_DIR/vq/bench_$tag.json')); print('config4v', d['value'], d['roofline']['resident_instances_per_cu'])"
