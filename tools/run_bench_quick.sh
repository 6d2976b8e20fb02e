#!/bin/bash
O=${BENCH_OUT:-bench_out}      # output directory (relative to the repository root)
mkdir -p $O
timeout -k 5 900 python bench.py --full --steps 10 --warmup 3 > $O/bench_quick.json 2> $O/bench_quick.err; tail -3 $O/bench_quick.err
python - "$O" <<'PY'
import json, sys
d=json.loads(open(sys.argv[1] + "/bench_quick.json").read().strip().splitlines()[-1])
print("value", d["value"], "ms", d["ms_per_step"])
print("roofline", d["roofline"]["kernel"], d["roofline"]["frac"])
print("warmup_stage", d.get("warmup_stage"))
print("micro", {k: d["microbench"][k] for k in d["microbench"] if "us" in k})
print("breakdown", {k: round(v, 3) for k, v in d["breakdown_ms_per_step"].items()})
PY
