#!/bin/bash
# One GPU-box session: parity tests, smoke, bench, rocprof.  Everything lands in $OUT (default session_out/).
set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
OUT="${OUT:-session_out}"
mkdir -p "$OUT"
export TMPDIR=/tmp
WHAT="${1:-all}"
echo "== $(date) host: $(nproc) cpus; $(rocminfo 2>/dev/null | grep -m1 'Marketing Name.*MI' || true)" | tee $OUT/session.log
if [[ "$WHAT" == all || "$WHAT" == tests ]]; then
  timeout 1500 python -m pytest tests -m gpu -q --no-header -rfE -p no:cacheprovider ${PYTEST_K:+-k "$PYTEST_K"} > $OUT/pytest_gpu.log 2>&1
  echo "pytest exit $?" | tee -a $OUT/session.log
  tail -n 60 $OUT/pytest_gpu.log
fi
if [[ "$WHAT" == all || "$WHAT" == smoke ]]; then
  timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1; echo "smoke exit $?" | tee -a $OUT/session.log
  tail -n 5 $OUT/smoke.log
fi
if [[ "$WHAT" == all || "$WHAT" == bench ]]; then
  timeout 600 python bench.py --full --steps 50 --warmup 10 > $OUT/bench.json 2> $OUT/bench.err; echo "bench exit $?" | tee -a $OUT/session.log
  cat $OUT/bench.json; tail -n 5 $OUT/bench.err
  timeout 300 python bench.py --steps 30 --warmup 5 --no-graph --full --no-cpu-baseline > $OUT/bench_eager.json 2> $OUT/bench_eager.err; cat $OUT/bench_eager.json
  timeout 300 python bench.py --steps 20 --warmup 5 --batch 16 --full --no-cpu-baseline > $OUT/bench_b16.json 2> $OUT/bench_b16.err; cat $OUT/bench_b16.json
  timeout 300 python bench.py --steps 10 --warmup 3 --batch 128 --full --no-cpu-baseline > $OUT/bench_b128.json 2> $OUT/bench_b128.err; cat $OUT/bench_b128.json
fi
if [[ "$WHAT" == all || "$WHAT" == prof ]]; then
  (cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats -d "$OLDPWD/$OUT/prof" -o r --output-format csv -- python "$OLDPWD/bench.py" --steps 20 --warmup 5 --no-graph --full --no-cpu-baseline > "$OLDPWD/$OUT/prof_bench.json" 2> "$OLDPWD/$OUT/prof.err"); echo "rocprof exit $?" | tee -a $OUT/session.log
  find $OUT/prof -name "*kernel_stats.csv" | head -1 | xargs -r head -n 25
fi
ls -la "$OUT" | tail -n 20
