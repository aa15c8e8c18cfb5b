#!/usr/bin/env python3
"""Kernel by kernel, the gfx950 device assembly of two builds of the library, for a refactor that folds kernels: each kernel
the first build has and the second has not against the kernel that replaces it, every other kernel against itself, and the
resource lines of the replaced ones.  Needs no GPU.  Per side, in sps_amd/csrc:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -Rpass-analysis=kernel-resource-usage \
        -o side.s sps_hip.hip 2> side_res.txt
    python tools/ndt_one_map_asm.py parent.s branch.s parent_res.txt branch_res.txt [fold]

fold: which table of FOLDS below pairs the kernels (default one_map: profiles/ndt_one_map/asm_compare.txt; one_scan:
profiles/ndt_one_scan/asm_compare.txt).  A template instantiation is written k_name<Type>.

Compared per kernel: every line from its label to the end of its descriptor, comments dropped, basic-block labels renumbered
per function, and the kernel's own mangled name replaced by a placeholder, so that a kernel can be paired with one of another
name or with a template's instantiation.  Exit status 1 if anything differs."""
import re
import sys

UPD = ["upd_lookup", "upd_found", "upd_resolve", "upd_offsets", "upd_fill", "upd_stats", "upd_merge", "carve_begin", "carve_rays",
       "carve_decide"]
SCAN = ["k_ndt_assoc_batch", "k_ndt_pyr_assoc", "k_ndt_pyr_solve", "k_ndt_score"]
# fold -> (pairs (parent's kernel, branch's kernel), by-value kernels of the parent whose names the branch's second kernels took)
FOLDS = {
    "one_map": ([(f"k_ndt_pyr_{s}", f"k_ndt_{s}") for s in UPD], [f"k_ndt_{s}" for s in UPD]),
    "one_scan": ([(k, f"{k}<NdtPoints>") for k in SCAN] + [(k.replace("k_ndt_", "k_ndt_d2d_"), f"{k}<NdtCells>") for k in SCAN], []),
}


def short(mangled):
    """k_name, or k_name<Type> for an instantiation over one type: _ZN12_GLOBAL__N_111k_ndt_assocINS_9NdtPointsEEEvPKd..."""
    m = re.search(r"_GLOBAL__N_1(\d+)(k_\w+)", mangled)
    if not m:
        m = re.search(r"(k_[a-z0-9_]+)", mangled)
        return m.group(1) if m else mangled
    n = int(m.group(1))
    name, rest = m.group(2)[:n], m.group(2)[n:]
    t = re.match(r"INS_(\d+)(\w+)", rest)
    if t:
        return f"{name}<{t.group(2)[:int(t.group(1))]}>"
    return mangled if rest.startswith("I") else name    # other instantiations (the convolutions') keep their mangled names


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                if "k_" in name:
                    out[short(name)] = body
                name = None
                continue
            t = line.split(";")[0].rstrip()
            if not t.strip():
                continue
            t = re.sub(r"\.LBB\d+_", ".LBB_", t)
            body.append(t.replace(name, "@self"))
    return out


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


COLS = ("VGPRs", "TotalSGPRs", "LDS", "ScratchSize", "Occupancy")


def row(r):
    return " / ".join(str(r[c]) for c in COLS)


pa, br = kernels(sys.argv[1]), kernels(sys.argv[2])
rp, rb = resources(sys.argv[3]), resources(sys.argv[4])
pairs, by_value = FOLDS[sys.argv[5] if len(sys.argv) > 5 else "one_map"]
print(f"# {len(pa)} kernels in the parent, {len(br)} in the branch")
print("# a kernel of the parent against the kernel of the branch that replaces it: lines, equal?  Resources where they differ:")
print("# VGPRs / SGPRs / LDS bytes / scratch bytes per lane / waves per SIMD")
ok = True
for a, b in pairs:
    same = pa[a] == br[b]
    ok &= same
    print(f"{a:24s} -> {b:30s} {len(pa[a]):5d} {len(br[b]):5d}  {'identical' if same else 'DIFFERENT'}")
    if not same:
        print(f"    parent {row(rp[a])}    branch {row(rb[b])}")
paired_a, paired_b = {a for a, _ in pairs}, {b for _, b in pairs}
both = sorted((set(pa) & set(br)) - paired_a - paired_b)
diff = [k for k in both if pa[k] != br[k]]
print(f"# kernels present on both sides under one name and in no pair above: {len(both)} compared, different: {diff if diff else 'none'}")
print(f"# only in the parent, unpaired: {sorted(set(pa) - set(br) - paired_a)}")
print(f"# only in the branch, unpaired: {sorted(set(br) - set(pa) - paired_b)}")
if by_value:
    print("# the parent's by-value kernels, deleted, beside the level-in-grid kernels that took their names (branch; the parent's twin in brackets)")
    print(f"{'kernel':22s} {'branch':>28s} {'[parent twin]':>28s} {'parent by value':>28s}")
    for (a, b), v in zip([p for p in pairs if p[1] in by_value], by_value):
        print(f"{b:22s} {row(rb[b]):>28s} {'[' + row(rp[a]) + ']':>28s} {row(rp[v]):>28s}")
sys.exit(0 if ok and not diff else 1)
