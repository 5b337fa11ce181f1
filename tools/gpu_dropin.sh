# GPU tests (drop-in path) + state_dict-path benches (cfg2/cfg3 tensors, fragmented metric).
set -o pipefail
cd "$(dirname "$0")/.."; OUT=${OUT:-bench_outputs}; mkdir -p $OUT
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/pytest_gpu.log 2>&1 || { tail -40 $OUT/pytest_gpu.log; exit 1; }
tail -2 $OUT/pytest_gpu.log
run() { timeout -k 10 300 python bench.py --full "$@" --no-cpu-baseline > $OUT/ab.json 2>>$OUT/ab.err || { tail -20 $OUT/ab.err; exit 1; }
        python -c "import json,sys;d=json.load(open('$OUT/ab.json'));print(sys.argv[1:], d['value'], d['ms_per_step'], d['roofline']['kernel_avg_ms'], d['parity'])" "$@"; }
run --config resnet18 --layout tensors
run --config resnet18 --layout tiled
run --config vit_bf16 --layout tensors
run --config fragmented
