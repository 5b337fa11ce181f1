# One GPU session: parity tests, HBM probe, kernel-variant sweep, rocprofv3 evidence.
set -o pipefail
cd "$(dirname "$0")/.."; OUT=${OUT:-bench_outputs}
mkdir -p $OUT
fault() { case "$1" in 124|134|137|139) return 0;; *) return 1;; esac; }
timeout -k 10 600 python -m pytest tests -m gpu -q > $OUT/pytest_gpu.log 2>&1; rc=$?
tail -6 $OUT/pytest_gpu.log; fault $rc && exit $rc
timeout -k 10 200 python tools/hbm_probe.py 16 > $OUT/hbm_probe.json 2>$OUT/hbm_probe.err; rc=$?
cat $OUT/hbm_probe.json; fault $rc && exit $rc
for v in ${VARIANTS:-0 1 2 3 4 5 6 7 8}; do
  timeout -k 10 300 python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --variant $v > $OUT/bench_v$v.json 2>>$OUT/bench_sweep.err; rc=$?
  echo "variant $v: $(python -c "import json;d=json.load(open('$OUT/bench_v$v.json'));print(d['value'], d['roofline']['kernel_avg_ms'], d['parity'])")"
  fault $rc && exit $rc
done
[ -n "$NOPROF" ] || bash tools/profile.sh ${TAG:-r01}
