#!/usr/bin/env python3
"""Kernel by kernel, the gfx950 device assembly of two builds of the library (profiles/ndt_one_map/asm_compare.txt): the former
k_ndt_pyr_upd_* / k_ndt_pyr_carve_* of the first against k_ndt_upd_* / k_ndt_carve_* of the second, every other kernel against
itself, and the resource lines of the update / carve kernels.  Needs no GPU.  Per side, in sps_amd/csrc:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -Rpass-analysis=kernel-resource-usage \
        -o side.s sps_hip.hip 2> side_res.txt
    python tools/ndt_one_map_asm.py parent.s branch.s parent_res.txt branch_res.txt

Compared per kernel: every line from its label to the end of its descriptor, comments dropped, basic-block labels renumbered
per function, and the renamed kernels' own mangled names made equal.  Exit status 1 if anything differs."""
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = body
                name = None
                continue
            t = line.split(";")[0].rstrip()
            if not t.strip():
                continue
            t = re.sub(r"\.LBB\d+_", ".LBB_", t)
            t = re.sub(r"\d+k_ndt_(?:pyr_)?(upd|carve)_", r"k_ndt_\1_", t)   # the renamed kernels' own mangled names
            body.append(t)
    return out


def short(mangled):
    m = re.search(r"(k_[a-z0-9_]+)", mangled)
    # the mangled name carries the length: _ZN12_GLOBAL__N_116k_ndt_upd_lookupE...
    m2 = re.search(r"_GLOBAL__N_1(\d+)(k_\w+)", mangled)
    if m2:
        return m2.group(2)[:int(m2.group(1))]
    return m.group(1) if m else mangled


def resources(path):
    res, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = short(m.group(1))
            res[cur] = {}
            continue
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur:
            res[cur][m.group(1).split(" ")[0]] = int(m.group(2))
    return res


pa, br = kernels(sys.argv[1]), kernels(sys.argv[2])
pa = {short(k): v for k, v in pa.items() if "k_" in k}
br = {short(k): v for k, v in br.items() if "k_" in k}
rp, rb = resources(sys.argv[3]), resources(sys.argv[4])
stems = ["upd_lookup", "upd_found", "upd_resolve", "upd_offsets", "upd_fill", "upd_stats", "upd_merge", "carve_begin", "carve_rays",
         "carve_decide"]
print("# former k_ndt_pyr_<x> of the parent against k_ndt_<x> of the branch: instructions, equal?")
ok = True
for s in stems:
    a, b = pa["k_ndt_pyr_" + s], br["k_ndt_" + s]
    same = a == b
    ok &= same
    print(f"k_ndt_pyr_{s:12s} -> k_ndt_{s:12s} {len(a):5d} {len(b):5d}  {'identical' if same else 'DIFFERENT'}")
print("# kernels present on both sides under one name (every kernel of the library but the ten above)")
diff = []
n = 0
for k in sorted(set(pa) & set(br)):
    if k.startswith("k_ndt_upd_") or k.startswith("k_ndt_carve_"):
        continue
    n += 1
    if pa[k] != br[k]:
        diff.append(k)
for k in ("k_ndt_src_lookup", "k_ndt_src_found", "k_ndt_src_resolve", "k_ndt_src_offsets", "k_ndt_src_fill", "k_ndt_src_stats", "k_ndt_src_records",
          "k_ndt_assoc", "k_ndt_pyr_assoc", "k_ndt_pyr_solve", "k_ndt_assoc_batch", "k_ndt_solve_batch", "k_ndt_pyr_assoc_batch",
          "k_ndt_pyr_solve_batch", "k_ndt_select", "k_ndt_cells", "k_ndt_cells_get", "k_loc_solve"):
    if k in pa and k in br:
        print(f"{k:28s} {len(pa[k]):5d} {len(br[k]):5d}  {'identical' if pa[k] == br[k] else 'DIFFERENT'}")
    else:
        print(f"{k:28s} (no such kernel: parent {k in pa}, branch {k in br})")
print(f"# {n} kernels compared, different: {diff if diff else 'none'}")
print(f"# only in the parent: {sorted(set(pa) - set(br))}")
print(f"# only in the branch: {sorted(set(br) - set(pa))}")
print("# resources of the surviving update/carve kernels (branch; the parent's k_ndt_pyr_<x> in brackets; the parent's by-value k_ndt_<x> last)")
print(f"{'kernel':22s} {'VGPRs':>12s} {'SGPRs':>12s} {'LDS':>14s} {'scratch':>10s} {'occupancy':>10s}   by-value parent (VGPRs SGPRs LDS scratch occ)")
for s in stems:
    b, p, v = rb["k_ndt_" + s], rp["k_ndt_pyr_" + s], rp["k_ndt_" + s]
    cols = ("VGPRs", "TotalSGPRs", "LDS", "ScratchSize", "Occupancy")
    print(f"k_ndt_{s:16s} " + " ".join(f"{b[c]:6d} [{p[c]:5d}]" for c in cols) + "   " + " ".join(str(v[c]) for c in cols))
sys.exit(0 if ok and not diff else 1)
