# GPU check of an IPM change (tube): tube / tube-time / SBPLX-QCQP / config-3
# tests, the 400-seed status agreement, and the C3, time-qcqp (FD) and
# time-qcqp (LN_SBPLX) bench lines with their CPU baselines (--full).
# Outputs under $MTG_OUT/ipm/ (default measure_out/ipm/).
set -e -o pipefail
OUT=${MTG_OUT:-measure_out}/ipm
mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 900 python -u -m pytest -x -q --timeout 600 --timeout-method thread \
  tests/test_tube_gpu.py tests/test_tube_time_gpu.py tests/test_tube_time_sbplx_gpu.py \
  tests/test_configs_gpu.py tests/test_cpp_api.py -k "tube or config3 or cpp" > "$OUT/tests.log" 2>&1
timeout -k 10 300 python tools/tube_status_agreement.py ipm > "$OUT/agreement.txt" 2>&1
timeout -k 10 300 python bench.py --full --workload tube --steps 20 --warmup 3 > "$OUT/bench_tube.json" 2> "$OUT/bench_tube.err"
timeout -k 10 300 python bench.py --full --workload time-qcqp --steps 5 --warmup 2 > "$OUT/bench_time_qcqp.json" 2> "$OUT/bench_time_qcqp.err"
timeout -k 10 600 python bench.py --full --workload time-qcqp --optimizer sbplx --steps 3 --warmup 1 > "$OUT/bench_time_qcqp_sbplx.json" 2> "$OUT/bench_time_qcqp_sbplx.err"
