#!/bin/bash
# the bench lines of every configuration (--full: with the per-call roofline pass and the CPU baseline where the config has one)
# -> <dir>/<cfg>.json, <dir> = the second argument (default: a new temporary directory)
TAG=${1:-r04}
cd ${GRAFT_REPO_ROOT:-/root/repo}
LINES=${2:-$(mktemp -d -t lines_$TAG.XXXXXX)}
mkdir -p $LINES
python bench.py --full --steps 50 --warmup 5 2>/dev/null | tail -1 > $LINES/cfg2.json
for c in cfg4 cfg5 cfg3 cfg1; do python bench.py --full --config $c --steps 30 --warmup 5 2>/dev/null | tail -1 > $LINES/$c.json; done
python - <<PY
import json
for c in ("cfg2","cfg4","cfg5","cfg3","cfg1"):
    d=json.load(open("$LINES/%s.json"%c)); r=d["roofline"]
    print(c, round(d["value"]), round(d["ms_per_step"],4), r.get("kernel"), r.get("bound"), r.get("frac"), r.get("traffic"), r.get("traffic_stale"), (d.get("cpu_baseline") or {}).get("value"))
PY
