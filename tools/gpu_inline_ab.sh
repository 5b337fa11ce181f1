# Inline (kernel-argument) vs staged descriptor tables: GPU tests, then A/B on the metric, cfg2 and
# one N = 8 rank's chunked step (tools/host_overhead.py), interleaved.
set -o pipefail
cd "$(dirname "$0")/.."; OUT=${OUT:-bench_outputs}
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest tests -m gpu -q -x --timeout 120 --timeout-method thread > $OUT/pytest_gpu.log 2>&1 || { tail -30 $OUT/pytest_gpu.log; exit 1; }
tail -2 $OUT/pytest_gpu.log
for rep in 1 2; do
  for f in 1 0; do
    for c in metric resnet18; do
      FA_INLINE_DESC=$f timeout -k 10 300 python bench.py --full --config $c --steps 20 --warmup 3 --no-cpu-baseline > $OUT/ab_${c}_$f.json 2> $OUT/ab_${c}_$f.err || { tail -5 $OUT/ab_${c}_$f.err; exit 1; }
      python -c "import json;d=json.load(open('$OUT/ab_${c}_$f.json'));print('rep $rep inline=$f $c',d['value'],d['ms_per_step'],d['roofline'].get('kernel_avg_ms'),d.get('parity'))"
    done
  done
done
for f in 1 0; do
  FA_INLINE_DESC=$f timeout -k 10 300 python tools/host_overhead.py > $OUT/ho_$f.json 2> $OUT/ho_$f.err || { tail -5 $OUT/ho_$f.err; exit 1; }
  echo "host_overhead inline=$f"; tail -12 $OUT/ho_$f.json
done
