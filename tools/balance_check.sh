# round-5 measured batch layout: full GPU suite, then the 1-GPU bench and the 8-engine rehearsal
#   tools/balance_check.sh OUTPUT_DIR
set -e
OUT=${1:?output directory}
mkdir -p "$OUT"
export PYTHONPATH=$PWD:$PWD/tests
timeout -k 10 900 python -u -m pytest -x -q --timeout 300 --timeout-method thread -m gpu tests > "$OUT/bal5_gputests.log" 2>&1
timeout -k 10 400 python -u bench.py --full > "$OUT/bal5_bench.json" 2> "$OUT/bal5_bench.err"
timeout -k 10 400 python -u bench.py --full --no-directed --opt devices=8 > "$OUT/bal5_dev8.json" 2> "$OUT/bal5_dev8.err"
