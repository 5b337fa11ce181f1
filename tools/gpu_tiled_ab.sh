# Tiled-arena parity tests, then interleaved A/B of the metric (client-major vs tiled arena) + hier/cfg2/cfg3.
set -o pipefail
cd "$(dirname "$0")/.."; OUT=${OUT:-bench_outputs}; mkdir -p $OUT
timeout -k 10 600 python -u -m pytest tests/test_gpu_tiled.py tests/test_gpu_parity.py -x -q --timeout 120 --timeout-method thread > $OUT/pytest_tiled.log 2>&1 || { tail -40 $OUT/pytest_tiled.log; exit 1; }
tail -2 $OUT/pytest_tiled.log
run() { timeout -k 10 300 python bench.py --full "$@" --no-cpu-baseline > $OUT/ab.json 2>>$OUT/ab.err || { tail -20 $OUT/ab.err; exit 1; }
        python -c "import json,sys;d=json.load(open('$OUT/ab.json'));print(sys.argv[1:], d['value'], d['roofline']['kernel_avg_ms'], d['parity'])" "$@"; }
for r in 1 2 3; do run --layout arena; run --layout tiled; done
run --config hier --layout arena; run --config hier --layout tiled
run --config resnet18 --layout arena; run --config resnet18 --layout tiled
run --config vit_bf16 --layout arena; run --config vit_bf16 --layout tiled
