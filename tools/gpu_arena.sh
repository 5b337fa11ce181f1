set -o pipefail
cd "$(dirname "$0")/.."; OUT=${OUT:-bench_outputs}
mkdir -p $OUT
fault() { case "$1" in 124|134|137|139) return 0;; *) return 1;; esac; }
timeout -k 10 600 python -m pytest tests -m gpu -q -x > $OUT/pytest_gpu.log 2>&1; rc=$?
tail -15 $OUT/pytest_gpu.log; fault $rc && exit $rc
for c in metric resnet18 vit_bf16 hier gossip; do
  timeout -k 10 400 python bench.py --full --config $c --steps 10 --warmup 3 --no-cpu-baseline > $OUT/arena_$c.json 2> $OUT/arena_$c.err; rc=$?
  echo "== $c rc=$rc $(python -c "import json;d=json.load(open('$OUT/arena_$c.json'));print(d['value'], d['ms_per_step'], d['roofline']['achieved'], d['roofline']['frac'], d['parity'])")"
  fault $rc && exit $rc
done
for v in 0 4 6 7 8; do
  timeout -k 10 300 python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --variant $v > $OUT/arena_v$v.json 2>>$OUT/arena_sweep.err; rc=$?
  echo "variant $v: $(python -c "import json;d=json.load(open('$OUT/arena_v$v.json'));print(d['value'], d['roofline']['kernel_avg_ms'], d['parity'])")"
  fault $rc && exit $rc
done
