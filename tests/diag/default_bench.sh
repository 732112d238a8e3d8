# the driver-form run with every --full leg, and its wall time: bash tests/diag/default_bench.sh <out dir>
O=$1; mkdir -p $O
t0=$(date +%s)
python bench.py --full > $O/bench.json 2> $O/bench.err
echo "wall seconds: $(( $(date +%s) - t0 ))" | tee $O/bench_wall.txt
python - <<PY
import json
d = json.loads(open("$O/bench.json").read().strip().splitlines()[-1])
print(d["value"], d["ms_per_step"], d["roofline"]["frac"], d["roofline"]["traffic"], d["graph_captures_in_timed_region"], d["graph_setup_steps"], d["cpu_baseline"]["value"])
for k, v in d["extras"].items():
    if isinstance(v, dict):
        print(k, v.get("value"), (v.get("roofline") or {}).get("frac"), (v.get("roofline") or {}).get("traffic"))
PY
