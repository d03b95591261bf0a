set -e
OUT_DIR=${OUT_DIR:-out}
mkdir -p $OUT_DIR
timeout -k 10 900 python -m pytest tests -m gpu -q > $OUT_DIR/gputest.log 2>&1 || true
tail -8 $OUT_DIR/gputest.log
for B in 256 512 1024 2048 2816 4096; do
  timeout -k 10 100 python bench.py --full --min-seconds 6 --batch $B --split 1 --steps 50 --warmup 10 --no-cpu-baseline > $OUT_DIR/lat_$B.json 2> $OUT_DIR/lat_$B.err
  python3 -c "import json;r=json.load(open('$OUT_DIR/lat_$B.json'));print($B, r['value'], r['ms_per_step'], r['roofline']['kernel_ms'], r['roofline']['resident_instances_per_cu'])"
done
