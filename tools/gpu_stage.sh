#!/bin/bash
# development GPU run: usage: bash tools/gpu_stage.sh <tag> [tests] [bench] [benchmain] [pmc] [traffic] [prof]
tag=$1; shift
root=$(pwd); out=$(realpath -m "${OUT_DIR:-results}")   # results under $OUT_DIR (default: results/ of the tree)
mkdir -p "$out"
for what in "$@"; do
  case $what in
    tests)     timeout ${TESTS_LIMIT:-420} python -m pytest tests -m gpu -q -x > $out/${tag}_tests.log 2>&1; echo "tests rc=$?"; tail -4 $out/${tag}_tests.log ;;
    bench)     timeout ${BENCH_LIMIT:-700} python bench.py --full > $out/${tag}_bench.json 2> $out/${tag}_bench.err; echo "bench rc=$?"; tail -c 400 $out/${tag}_bench.err; head -c 600 $out/${tag}_bench.json; echo ;;
    benchmain) timeout 300 python bench.py --only-main --steps 3 > $out/${tag}_benchmain.json 2> $out/${tag}_benchmain.err; echo "benchmain rc=$?"; tail -c 300 $out/${tag}_benchmain.err; python - <<PY
import json
try:
    d = json.load(open("$out/${tag}_benchmain.json")); print(d["value"], {k: v["avg_us"] for k, v in d["kernels"].items()})
except Exception as e: print("no line", e)
PY
 ;;
    single)    timeout 200 python bench.py --batch 1 --only-main --steps 3 > $out/${tag}_single.json 2> $out/${tag}_single.err; echo "single rc=$?"; python -c "
import json; d=json.load(open('$out/${tag}_single.json')); print(d['ms_per_step'], {k: v['avg_us'] for k, v in d['kernels'].items()})" ;;
    pmc)       bash tools/prof_parse_pmc.sh $tag --batch 512 > $out/${tag}_pmc.txt 2>&1; grep -E "k_parse|k_recon|pass" $out/${tag}_pmc.txt | cut -c1-420 ;;
    traffic)   bash tools/prof_hbm_traffic.sh 2>&1 | tail -3 ;;
    prof)      ( cd /tmp && export TMPDIR=/tmp
                 HIPDEC_SYNC_UPLOAD=1 timeout 240 rocprofv3 --kernel-trace --stats --output-format csv -d $out/${tag}_prof -o p -- \
                   python $root/bench.py --only-main --steps 2 --warmup 1 > $out/${tag}_prof_bench.json 2> $out/${tag}_prof.err
                 echo "prof rc=$?"; f=$(find $out/${tag}_prof -name '*kernel_stats.csv' | head -1); [ -n "$f" ] && head -12 $f ) ;;
  esac
done
