"""What the A/B tools of the kernel families share (tools/gpu_qp_ab_dump.py, tools/gpu_pm_ab_dump.py): the timing loop of one point, the compiler's
resource-usage remarks as a table, and the report that holds the new library's median against the parent's maximum."""
import json
import os
import re

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
REPEATS, WARMUP = 7, 2


def timed(solve, ms, iters=lambda res: res.iters, status=lambda res: res.status):
    for _ in range(WARMUP):
        solve()
    times = []
    for _ in range(REPEATS):
        res = solve()
        times.append(float(ms()))
    return {"ms": times, "iters_sum": int(iters(res).sum()), "iters_max": int(iters(res).max()), "converged": float((status(res) == 0).mean())}


def write_times(path, pts):
    with open(path, "w") as f:
        json.dump({"library": os.environ.get("OPTAS_HIP_LIBRARY", "in-tree"), "points": pts}, f, indent=1)


def resource_usage(path, kernels):
    """{kernel: {vgprs, sgprs, scratch_bytes, occupancy}} of the kernels ({piece of the mangled name: name}) in one file of resource-usage remarks"""
    table, name = {}, None
    fields = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes", "Occupancy [waves/SIMD]": "occupancy"}
    for line in open(path):
        hit = re.search(r"remark: +([A-Za-z \[\]/]+): (\S+) \[-Rpass-analysis", line)
        if not hit:
            continue
        if hit.group(1) == "Function Name":
            name = next((pretty for mangled, pretty in kernels.items() if mangled in hit.group(2)), None)
        elif name and hit.group(1) in fields:
            table.setdefault(name, {})[fields[hit.group(1)]] = int(hit.group(2))
    return table


def report(files, kernels, source, out_name, check_occupancy=False):
    """files: the json files of `time`, told apart by their "library" entry (several per library are pooled), and *.remarks files, the parent's with
    "parent" in the file name.  Writes profiles/<out_name>; 0 if every point holds and no kernel gained scratch (check_occupancy: nor lost occupancy)."""
    runs, usage = {"parent": {}, "new": {}}, {"parent": {}, "new": {}}
    for path in files:
        if path.endswith(".remarks"):
            usage["parent" if "parent" in os.path.basename(path) else "new"].update(resource_usage(path, kernels))
            continue
        rec = json.load(open(path))
        side = "new" if rec["library"] == "in-tree" else "parent"
        for k, v in rec["points"].items():
            e = runs[side].setdefault(k, dict(v, ms=[]))
            assert (e["iters_sum"], e["iters_max"], e["path"]) == (v["iters_sum"], v["iters_max"], v["path"]), (path, k)
            e["ms"].extend(v["ms"])
    points = {}
    for k, nw in runs["new"].items():
        pa = runs["parent"][k]
        assert (pa["iters_sum"], pa["iters_max"]) == (nw["iters_sum"], nw["iters_max"]), (k, pa, nw)  # the same iteration on both sides
        points[k] = {"path": nw["path"], "parent_ms": pa["ms"], "new_ms": nw["ms"], "parent_max_ms": max(pa["ms"]), "new_median_ms": float(np.median(nw["ms"])),
                     "holds": bool(np.median(nw["ms"]) <= max(pa["ms"])), "iters_sum": nw["iters_sum"], "iters_max": nw["iters_max"],
                     "converged": (pa["converged"], nw["converged"])}
    scratch_gained = [k for k, v in usage["new"].items() if v["scratch_bytes"] > usage["parent"][k]["scratch_bytes"]]
    occupancy_lost = [k for k, v in usage["new"].items() if v["occupancy"] < usage["parent"][k]["occupancy"]] if check_occupancy else []
    res = {"source": source, "timer": "oh_get_timing out[4] (HIP events around the solve's launches); per process %d solves after %d warm-ups" % (REPEATS, WARMUP),
           "speed_criterion": "per point, the new library's median over its runs <= the parent's maximum over its runs; processes of the two libraries alternated",
           "points": points, "resource_usage_new": usage["new"], "resource_usage_parent": usage["parent"], "scratch_gained": scratch_gained}
    if check_occupancy:
        res["occupancy_lost"] = occupancy_lost
    with open(os.path.join(ROOT, "profiles", out_name), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: (v["parent_max_ms"], v["new_median_ms"], v["holds"]) for k, v in points.items()}, indent=1))
    return 0 if all(v["holds"] for v in points.values()) and not scratch_gained and not occupancy_lost else 1
