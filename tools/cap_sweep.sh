out=$(mktemp -d); trap 'rm -rf "$out"' EXIT
for cap in 25165824 8388608 5242880; do
  GSPLAT_BENCH_PAIR_CAP=$cap python bench.py --full --no-cpu-baseline --steps 40 > "$out/cap_$cap.json" 2>/dev/null
  python - $cap "$out/cap_$cap.json" <<'PY'
import json,sys
d=json.load(open(sys.argv[2]))
print(sys.argv[1], "views/s", d["value"], {k: v["ms"] for k, v in d["stages"].items()}, d["config"].get("workload_stats", d.get("workload_stats")))
PY
done
