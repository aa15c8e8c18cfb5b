#!/usr/bin/env python3
"""The A/B table of profiles/ndt_one_map/timing_ab.txt from a file of '## run R <parent|branch> <mode>' lines, each followed by
the JSON line of that run of tools/localiser_timing.py --localiser ndt <mode> (mode 'bench': of bench.py).  Per figure: each
run's median, the median of the three on each side, and the rule that the branch's may exceed the parent's by at most the
parent's own spread (max - min of its three)."""
import json
import statistics as st
import sys

runs, cur = {}, None
for line in open(sys.argv[1]):
    line = line.strip()
    if line.startswith("## run"):
        _, _, r, side, *mode = line.split()
        cur = (side, " ".join(mode))
    elif line.startswith("{"):
        runs.setdefault(cur, []).append(json.loads(line))
figures = [("--update-map", "update_alone_ms", True), ("--update-map", "submit_integrate_ms", True), ("--update-map", "submit_ms", False),
           ("--update-map", "dynamic_build_ms", False),
           ("--carve", "carve_alone_ms", True), ("--carve", "update_alone_ms", False), ("--carve", "submit_integrate_carve_ms", True),
           ("--resolutions 2,1,0.5 --integrate --carve", "submit_ms", False),
           ("--resolutions 2,1,0.5 --integrate --carve", "update_fused_ms", True),
           ("--resolutions 2,1,0.5 --integrate --carve", "carve_fused_ms", True),
           ("--resolutions 2,1,0.5 --integrate --carve", "submit_online_ms", True),
           ("--resolutions 2,1,0.5 --integrate --carve", "update_chained_ms", False),
           ("--resolutions 2,1,0.5 --integrate --carve", "carve_chained_ms", False),
           ("bench", "ms_per_step", True)]
print("# medians of each run in ms (bench: ms per step), parent and branch alternating in one session, profiler off")
print("# condition (gated rows): median of the branch's three <= median of the parent's three + (max - min of the parent's three)")
print(f"{'mode':44s} {'figure':26s} {'parent 1':>9s} {'parent 2':>9s} {'parent 3':>9s} {'branch 1':>9s} {'branch 2':>9s} {'branch 3':>9s} "
      f"{'p median':>9s} {'p spread':>9s} {'b median':>9s} {'b - p':>9s}  verdict")
ok = True
for mode, key, gated in figures:
    vals = {}
    for side in ("parent", "branch"):
        rs = runs.get((side, mode), [])
        if not rs or key not in rs[0]:
            break
        vals[side] = [r[key]["median"] if isinstance(r[key], dict) else r[key] for r in rs]
    else:
        p, b = vals["parent"], vals["branch"]
        pm, bm, sp = st.median(p), st.median(b), max(p) - min(p)
        holds = bm <= pm + sp
        verdict = ("holds" if holds else "EXCEEDS") if gated else "recorded, not gated"
        ok &= holds or not gated
        print(f"{mode:44s} {key:26s} " + " ".join(f"{v:9.4f}" for v in p + b) + f" {pm:9.4f} {sp:9.4f} {bm:9.4f} {bm - pm:+9.4f}  {verdict}")
        continue
    print(f"{mode:44s} {key:26s} (not in the output)")
print("# every gated figure holds" if ok else "# a gated figure does not hold")
