#!/bin/bash
# One GPU session: parity tests, the full bench line, a rocprofv3 kernel
# summary of the headline config and the PMC passes bench.py's roofline reads.
# Every GPU step has its own time limit; a crash / timeout stops the session.
#   tools/round_all.sh <tag>      -> $OUT_DIR (default: out/ in the repository)
R="${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}"
TAG="${1:-r02}"
OUT="${OUT_DIR:-$R/out}"
cd "$R" && mkdir -p "$OUT"
PYTHONUNBUFFERED=1 timeout -k 10 400 python -u -m pytest tests -m gpu -x -q -rf --timeout 120 --timeout-method thread \
    > "$OUT/pytest_gpu_$TAG.txt" 2>&1
rc=$?; tail -3 "$OUT/pytest_gpu_$TAG.txt"; echo "pytest rc=$rc"
[ $rc -eq 0 ] || exit $rc
timeout -k 10 400 python bench.py --full > "$OUT/bench_$TAG.json" 2> "$OUT/bench_$TAG.err"
rc=$?; cut -c1-600 "$OUT/bench_$TAG.json"; echo "bench rc=$rc"
[ $rc -eq 0 ] || { tail -20 "$OUT/bench_$TAG.err"; exit $rc; }
[ -n "$NO_PROF" ] && exit 0
PROF_TIMEOUT=300 bash tools/profile.sh > "$OUT/profile_$TAG.txt" 2>&1
rc=$?; tail -8 "$OUT/profile_$TAG.txt"; [ $rc -eq 0 ] || exit $rc
bash tools/pmc_round.sh $TAG
