#!/bin/bash
# One GPU-box pass: gpu tests, smoke, 1-GPU bench (--full record), kernel-trace stats of the bench.
# Every GPU step has its own time limit; the chain stops at the first failure.
# Logs go to $OUT_DIR (default: build/gpu_round under the repository root).
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
ROOT=$PWD
OUT=$(realpath -m "${OUT_DIR:-$ROOT/build/gpu_round}")   # absolute: the profiler step runs from /tmp
mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread \
    > "$OUT/gpu_tests.log" 2>&1 \
&& timeout -k 10 180 python -u -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1 \
&& timeout -k 10 300 python -u bench.py --full > "$OUT/bench.log" 2>&1 \
&& if [ "${PROFILE:-1}" = 1 ]; then
     (cd /tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_bench" \
        -o bench -- python3 "$ROOT/bench.py" --steps 5 --warmup 2) > "$OUT/prof_bench.log" 2>&1
   fi
rc=$?
tail -3 "$OUT/gpu_tests.log"; tail -2 "$OUT/smoke.log" 2>/dev/null; tail -2 "$OUT/bench.log" 2>/dev/null
exit $rc
