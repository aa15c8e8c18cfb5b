#!/usr/bin/env python3
"""The A/B table of a refactor's timing_ab.txt (profiles/ndt_one_map, profiles/ndt_one_scan) from a file of
'## run R <parent|branch> <mode>' lines, each followed by the JSON line of that run of tools/localiser_timing.py --localiser ndt
<mode> (mode 'bench': of bench.py).  Per figure: each run's median, the median of the three on each side, and the rule that the
branch's may exceed the parent's by at most the parent's own spread (max - min of its three).

    python tools/ndt_one_map_timing.py runs.txt [fold]

fold: which table of FIGURES below names the figures (default one_map).  A figure is a path into the run's JSON, its parts
joined by dots; a dict with a 'median' stands for that median."""
import json
import statistics as st
import sys

PYR = "--resolutions 2,1,0.5 --integrate --carve"
D2D_PYR = ("--source cells --resolutions 2,1,0.5 --source-resolutions 2,1,0.5 --iterations 90 --level-iterations 30,30,30 "
           "--source-min-points 6")
# fold -> (mode, figure, gated)
FIGURES = {
    "one_map": [("--update-map", "update_alone_ms", True), ("--update-map", "submit_integrate_ms", True),
                ("--update-map", "submit_ms", False), ("--update-map", "dynamic_build_ms", False),
                ("--carve", "carve_alone_ms", True), ("--carve", "update_alone_ms", False),
                ("--carve", "submit_integrate_carve_ms", True),
                (PYR, "submit_ms", False), (PYR, "update_fused_ms", True), (PYR, "carve_fused_ms", True),
                (PYR, "submit_online_ms", True), (PYR, "update_chained_ms", False), (PYR, "carve_chained_ms", False),
                ("bench", "ms_per_step", True)],
    "one_scan": [("", "ndt.ms", True), ("", "icp.ms", False),
                 ("--hypotheses 8", "batch_ms", True), ("--hypotheses 8", "k_single_ms", False),
                 ("--hypotheses 8", "one_submit_ms", False),
                 ("--search 4096", "score_poses_ms", True), ("--search 4096", "batch0_ms", False),
                 ("--resolutions 2,1,0.5", "usual.pyramid.ms", True), ("--resolutions 2,1,0.5", "lag_0.5m.pyramid.ms", True),
                 ("--resolutions 2,1,0.5", "usual.single.ms", False),
                 ("--source cells", "cells.ms", True), ("--source cells", "source_build_ms", True),
                 ("--source cells", "points.ms", False),
                 ("--source cells --d2d --hypotheses 8", "submit_batch_K8.cells", True),
                 ("--source cells --d2d --hypotheses 8", "submit_batch_K8.points", False),
                 ("--source cells --d2d --search 4096", "score_poses_P4096.cells", True),
                 ("--source cells --d2d --search 4096", "relocalise_P4096_keep8.cells", True),
                 ("--source cells --d2d --search 4096", "score_poses_P4096.points", False),
                 (D2D_PYR, "cells_pyramid.ms", True), (D2D_PYR, "source_build_ms.one_call", True),
                 (D2D_PYR, "source_build_ms.single_builds", True), (D2D_PYR, "points_pyramid.ms", False),
                 (D2D_PYR, "cells.ms", False),
                 ("bench", "ms_per_step", True)],
}


def figure(run, path):
    """the figure at ``path`` of a run's JSON, None where the run has none (a key may itself hold a dot: "lag_0.5m")"""
    while path:
        key = next((k for k in sorted(run, key=len, reverse=True) if path == k or path.startswith(k + ".")), None) \
            if isinstance(run, dict) else None
        if key is None:
            return None
        run, path = run[key], path[len(key) + 1:]
    return run["median"] if isinstance(run, dict) else run


runs, cur = {}, None
for line in open(sys.argv[1]):
    line = line.strip()
    if line.startswith("## run"):
        _, _, r, side, *mode = line.split()
        cur = (side, " ".join(mode))
    elif line.startswith("{"):
        runs.setdefault(cur, []).append(json.loads(line))
print("# medians of each run in ms (bench: ms per step), parent and branch alternating in one session, profiler off")
print("# condition (gated rows): median of the branch's three <= median of the parent's three + (max - min of the parent's three)")
print(f"{'mode':44s} {'figure':30s} {'parent 1':>9s} {'parent 2':>9s} {'parent 3':>9s} {'branch 1':>9s} {'branch 2':>9s} {'branch 3':>9s} "
      f"{'p median':>9s} {'p spread':>9s} {'b median':>9s} {'b - p':>9s}  verdict")
ok = True
for mode, key, gated in FIGURES[sys.argv[2] if len(sys.argv) > 2 else "one_map"]:
    name = (mode or "(plain)")[:44]
    vals = {side: [figure(r, key) for r in runs.get((side, mode), [])] for side in ("parent", "branch")}
    if not vals["parent"] or not vals["branch"] or None in vals["parent"] + vals["branch"]:
        print(f"{name:44s} {key:30s} (not in the output)")
        ok &= not gated
        continue
    p, b = vals["parent"], vals["branch"]
    pm, bm, sp = st.median(p), st.median(b), max(p) - min(p)
    holds = bm <= pm + sp
    verdict = ("holds" if holds else "EXCEEDS") if gated else "recorded, not gated"
    ok &= holds or not gated
    print(f"{name:44s} {key:30s} " + " ".join(f"{v:9.4f}" for v in p + b) + f" {pm:9.4f} {sp:9.4f} {bm:9.4f} {bm - pm:+9.4f}  {verdict}")
print("# every gated figure holds" if ok else "# a gated figure does not hold")
