set -o pipefail
cd $GRAFT_REPO_ROOT
# the full record: GPU suite, smoke, the 500-step benchmark with its AUC parity (bench.py --full)
# usage: tools/gpu_full.sh [LOG_DIR=build/gpu_full]
OUT=${1:-build/gpu_full}
mkdir -p "$OUT"
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > "$OUT/gpu_tests.log" 2>&1 || { tail -40 "$OUT/gpu_tests.log"; exit 1; }
tail -3 "$OUT/gpu_tests.log"
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1 || { tail -20 "$OUT/smoke.log"; exit 1; }
timeout -k 10 600 python -u bench.py --steps 500 --warmup 20 --full > "$OUT/bench500.log" 2>&1 || { tail -20 "$OUT/bench500.log"; exit 1; }
tail -1 "$OUT/bench500.log"
