#!/bin/bash
# round-end sequence on one box: GPU suite, smoke(), the full bench line (-> runs/<tag>/, or the directory given as $2)
TAG=${1:-full}; OUT=${2:-runs/$TAG}; mkdir -p $OUT
( time timeout 1800 python -m pytest tests -m gpu -q -x ) > $OUT/pytest.log 2>&1; echo "pytest rc $?" >> $OUT/pytest.log
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/smoke.log 2>&1
( time python bench.py --full > $OUT/bench.json 2> $OUT/bench.err ) 2> $OUT/bench.time
tail -4 $OUT/pytest.log; tail -1 $OUT/smoke.log; cat $OUT/bench.time | tail -3
python - <<PY
import json
j=json.loads(open("$OUT/bench.json").read().strip().splitlines()[-1])
print("value", j["value"], "ms", j["ms_per_step"], "roofline", j["roofline"]["frac"], "traffic", j["roofline"]["traffic"], "fk", j["roofline_fk_jac"]["frac"])
for k in ("tol_1e-08","tol_1e-06","batch_invariant"): print(k, {kk: vv for kk, vv in (j.get(k) or {}).items() if kk != "note"})
print("pcie", j["pcie_inclusive"]["solves_per_s"], "pop", j["quality"].get("population_vs_host_port",{}).get("misses_1e-6"), j["quality"].get("population_vs_host_port",{}).get("misses_1e-9"))
print("lat", j["latency_b1_ms"], j["latency_b1024_ms"], "cpu", j["cpu_baseline"]["value"], j["cpu_baseline"]["cores"])
for k,v in j["configs"].items():
    if isinstance(v, dict):
        rf=v.get("roofline") or {}; cb=v.get("cpu_baseline") or {}
        print(k, v.get("device_ms"), v.get("converged_frac"), "| rf", rf.get("kernel"), rf.get("achieved"), rf.get("frac"), "| cpu", cb.get("value"), cb.get("cores"), cb.get("gpu_vs_port_objective_rel_max"), cb.get("error"))
PY
