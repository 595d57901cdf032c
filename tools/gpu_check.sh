export TMPDIR=/tmp
OUT=${OUT:-gpu_check_out}
mkdir -p "$OUT"
timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > "$OUT/gpu_tests.log" 2>&1 || { echo TESTFAIL; tail -30 "$OUT/gpu_tests.log"; exit 1; }
tail -2 "$OUT/gpu_tests.log"
timeout -k 10 300 python -u bench.py --full > "$OUT/bench.log" 2>&1 || { echo BENCHFAIL; tail -20 "$OUT/bench.log"; exit 1; }
grep '^{' "$OUT/bench.log"
timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof" -o run -- python3 bench.py --full --no-cpu-baseline > "$OUT/bench_prof.log" 2>&1 || { echo PROFFAIL; exit 1; }
python3 tools/summarize_stats.py $(ls "$OUT"/prof/*/run_kernel_stats.csv "$OUT"/prof/run_kernel_stats.csv 2>/dev/null | head -1) 10
