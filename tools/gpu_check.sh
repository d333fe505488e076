# GPU check after a change: the whole -m gpu suite, then short bench lines for the given configs.
#   bash tools/gpu_check.sh TAG [CONFIG...]
set -o pipefail
export OUT=${OUT:-bench_out}  # where the outputs go
mkdir -p $OUT
tag=$1; shift
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 600 --timeout-method thread > $OUT/gpu_tests_$tag.txt 2>&1 || { tail -30 $OUT/gpu_tests_$tag.txt; exit 1; }
tail -1 $OUT/gpu_tests_$tag.txt
for cfg in "$@"; do
  timeout -k 10 300 python bench.py --full --config $cfg --steps 10 --warmup 2 --no-cpu-baseline > $OUT/bench_${tag}_$cfg.json 2> $OUT/bench_${tag}_$cfg.err || { tail -5 $OUT/bench_${tag}_$cfg.err; exit 1; }
  python3 -c "import json,sys;d=json.load(open(sys.argv[1]));print(sys.argv[2], round(d['ms_per_step'],3), 'build', round(d['build']['insert_ms'],3), {k[:22]: round(x,3) for k,x in list(d['kernels_ms'].items())[:6]})" $OUT/bench_${tag}_$cfg.json $cfg
done
