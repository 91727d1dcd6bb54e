#!/bin/bash
# usage: tools/sweep.sh "<residency list>"  -- runs bench.py per setting and prints value / fwd / stage times
out=$(mktemp -d); trap 'rm -rf "$out"' EXIT
for r in $1; do
  python bench.py --full --no-cpu-baseline --steps 40 --residency $r > "$out/sw_$r.json" 2>/dev/null
  python - "$r" "$out/sw_$r.json" <<'PY'
import json,sys
r=sys.argv[1]
d=json.load(open(sys.argv[2]))
print(r, "views/s", d["value"], "fwd_ms", d["fwd_ms"], {k: v["ms"] for k, v in d["stages"].items()}, d.get("depth_cuts"), d["workload_stats"]["M_pairs"])
PY
done
