# Round evidence: parity tests -> smoke -> bench --full -> rocprofv3 kernel-trace stats -> PMC traffic passes.
# Run from anywhere on a machine with one MI355X; logs and profiles go under $OUT_DIR (default: out/).
set -u
R="$(cd "$(dirname "$0")/.." && pwd)"
cd "$R"
O="${OUT_DIR:-out}"
TAG="${TAG:-run}"
mkdir -p "$O/prof" "$O/pmc"
rc=0
if [ -z "${SKIP_TESTS:-}" ]; then
timeout -k 10 900 python -u -m pytest tests -m gpu -q -rf --timeout 600 --timeout-method thread ${PYTEST_ARGS:-} > "$O/pytest_gpu.log" 2>&1
rc=$?
fi
echo "pytest rc=$rc" >> "$O/pytest_gpu.log"
[ $rc -eq 0 ] || [ $rc -eq 1 ] || exit $rc
if [ -z "${SKIP_TESTS:-}" ]; then
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$O/smoke.log" 2>&1 || exit $?
# every leg of the bench (timed-output check, rooflines, ResNet, CPU baseline)
timeout -k 10 600 python bench.py --full ${BENCH_ARGS:-} > "$O/bench.log" 2>&1 || exit $?
fi
export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$R/$O/prof" -o $TAG --output-format csv -- python3 "$R/bench.py" --streams 1 --steps 3 --warmup 1 > "$O/prof.log" 2>&1 || exit $?
find "$O/prof" -name "*kernel_trace*" -delete
for c in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 300 rocprofv3 --pmc $c --kernel-include-regex "^(k_|void k_)" -d "$R/$O/pmc/$c" -o pmc --output-format csv -- python3 "$R/bench.py" --streams 1 --steps 1 --warmup 0 --batch 8 > "$O/pmc/$c.log" 2>&1 || exit $?
done
# 8 HMults in the run (one mhe_hmult_batch call, the bench's default launch shape)
python3 scripts/traffic.py "$O/pmc" 8 "$O/pmc/traffic.json" > "$O/pmc/traffic.log" 2>&1
find "$O/pmc" -name "*.csv" -delete
exit $rc
