# kernel trace of BASELINE config 5's fit (skinning backward of the full mesh: split form + chunk reduction)
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mktemp -d)
timeout 600 rocprofv3 --kernel-trace --stats -d "$OUT" -o t -- python3 "$ROOT/bench.py" --config c5 --value-only --steps 1 --warmup 0 --iters 100 > /dev/null 2>&1
python3 "$ROOT/tools/rocpd_summary.py" "$OUT/t_results.db" /dev/null | sed -n 4,12p | cut -c1-100
