# Interleaved A/B of the weighted-sum kernel variants on the default (tiled) metric.
set -o pipefail
cd "$(dirname "$0")/.."; OUT=${OUT:-bench_outputs}; mkdir -p $OUT
for rep in 1 2; do for v in 0 1 2 4 5 7 8; do
  timeout -k 10 300 python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --check-samples 4096 --variant $v > $OUT/v.json 2>>$OUT/v.err || exit 1
  python -c "import json;d=json.load(open('$OUT/v.json'));print('variant', $v, d['value'], d['roofline']['kernel_avg_ms'], d['parity'][:9])"
done; done
