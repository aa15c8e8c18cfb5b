"""GPU tests of the global search at the edges of its kernels (sps_amd/csrc/bbs_kernels.inc.h), through the raw ABI
(sps_bbs_map_build / sps_bbs_map_level / sps_bbs_search) against the numpy restatement in tests/bbs_reference.py.  The
cases are those of tests/bbs_edge_inputs.py, and tests/test_bbs_cpu.py proves from the restatement alone that each sits
where it claims:

  chunk_*     k_bbs_score with 1, 2 and 3 chunks of 1024 offsets: counts of 1023 .. 3073 rows, the partial last int4,
              void words on both sides of a chunk edge, cap == n == 1025 (rows of the offsets that are not aligned)
  seg_*       k_bbs_threshold with 1, 1, 2, 5 and 65 scores per thread (cap 3 .. 65536), cut scores 1, 2 and 3 on the first
              and the last score of a segment, min_score 0, 1, 2; a score equal to cap (the last histogram bin)
  far_*       grids of 16377 x 1 and 1 x 16377 cells with three pooled levels and of 16384 x 1 with none: offsets of
              +-16376, +-16375, +-16383 (legal, out of reach) and +-16384 (void) in dx and in dy, with 0 and -1 on the other
              axis; pad_l7: 130 x 130 cells with seven levels, hits through the negative pad
  count_*     a device count beyond cap and a negative one
  frontier_*  the frontier limits 1 and 65536 on one scratch

Every comparison is exact: scores are integer sums, poses float64 with every operation fixed by the restatement.  The
cases that cut the frontier across several workgroups of k_bbs_count / k_bbs_write and pick 64 results out of 1500 tied
leaves go through the wrapper (cut_* of tests/bbs_inputs.py) and are compared in tests/test_hip_bbs.py."""
import numpy as np
import pytest
import torch

from tests import bbs_edge_inputs as BE
from tests import bbs_reference as BR

pytestmark = pytest.mark.gpu


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_CTX = {}


def context(grid):
    """a context of this module's own, holding the pyramid of ``grid`` (a key of BE.GRIDS): the localisers that
    tests/test_hip_bbs.py caches keep theirs"""
    from sps_amd import _native
    if "ctx" not in _CTX:
        _CTX["ctx"], _CTX["grid"] = _native.Context(torch.cuda.current_device()), None
    if _CTX["grid"] != grid:
        g = BE.GRIDS[grid]
        H, W = g["G0"].shape
        _CTX["grid"] = None
        _CTX["ctx"].bbs_map_build(dev(g["G0"]).data_ptr(), W, H, g["L"], stream())
        _CTX["grid"] = grid
    return _CTX["ctx"]


def scratch_for(cap, A, F):
    from sps_amd import _native
    return torch.empty(_native.lib.sps_bbs_search_scratch(cap, A, F), dtype=torch.uint8, device="cuda")


def raw_search(name, trace=True, scratch=None):
    """one call of sps_bbs_search for a case of BE.RAW -> GlobalSearchResult, the fields the wrapper's result has"""
    from sps_amd import _native
    from sps_amd.localiser import GlobalSearchResult
    c = BE.RAW[name]
    g = BE.GRIDS[c["grid"]]
    ctx = context(c["grid"])
    kw = c["kw"]
    K, A, F, L, cap = kw.get("keep", 8), c["A"], kw.get("frontier", 16384), g["L"], c["cap"]
    rows = np.zeros((max(cap, len(c["pts"]), 1), 3))                        # the device may read cap rows
    rows[:len(c["pts"])] = c["pts"]
    p_dev, n_dev = dev(rows), torch.full((1,), c["n_dev"], dtype=torch.int32, device="cuda")
    cs = dev(BR.yaw_table(A))
    top, score = torch.zeros(K, dtype=torch.int32, device="cuda"), torch.zeros(K, dtype=torch.int32, device="cuda")
    T_top, n_top = torch.zeros((K, 16), dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    info = torch.zeros(_native.BBS_INFO_WORDS, dtype=torch.int32, device="cuda")
    tr = torch.full(((L + 1), 5 * F), -1, dtype=torch.int32, device="cuda") if trace else None
    scratch = scratch_for(cap, A, F) if scratch is None else scratch
    assert scratch.numel() >= _native.lib.sps_bbs_search_scratch(cap, A, F) > 0
    T_up, z = kw.get("T_up", np.eye(4)), kw["scan_z"]
    ctx.bbs_search(p_dev.data_ptr(), n_dev.data_ptr(), cap, T_up, BE.R, g["i0"], g["j0"], z[0], z[1], cs.data_ptr(), A, F,
                   kw.get("min_score", 1), K, top.data_ptr(), score.data_ptr(), T_top.data_ptr(), n_top.data_ptr(),
                   info.data_ptr(), tr.data_ptr() if trace else None, scratch.data_ptr(), stream())
    i = info.cpu().numpy().astype(np.int64)
    per_level = i[4:4 + 2 * (L + 1)].reshape(L + 1, 2)
    cl = kl = None
    if trace:
        t = tr.cpu().numpy().astype(np.int64)
        cl = [t[l, :4 * F][t[l, :4 * F] >= 0] for l in range(L + 1)]
        kl = [t[l, 4 * F:][t[l, 4 * F:] >= 0] for l in range(L + 1)]
    out = GlobalSearchResult(top.cpu().numpy().astype(np.int64), score.cpu().numpy().astype(np.int64),
                             T_top.cpu().numpy().reshape(K, 4, 4), int(n_top.cpu()[0]), int(i[0]), int(i[1]), int(i[2]),
                             per_level[:, 0].copy(), per_level[:, 1].copy(), int(i[3]), len(BE.counted(c)), cl, kl)
    ctx.check_errors(stream())
    return out


def same_search(a, b):
    for f in ("index", "score", "poses", "candidates", "kept"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    for f in ("n_found", "certified", "dropped_bound", "n_dropped", "n_slice", "n_points"):
        assert getattr(a, f) == getattr(b, f), f


def equals_the_restatement(name, r):
    """everything tests/test_hip_bbs.py compares for a wrapper case, exactly; r: a result with its trace"""
    c, ref = BE.RAW[name], BE.reference(name)
    L = BE.GRIDS[c["grid"]]["L"]
    assert r.n_slice == ref["n_slice"]
    assert r.candidates.tolist() == ref["candidates"].tolist() and r.kept.tolist() == ref["kept"].tolist()
    for l in range(L, -1, -1):                                              # as ordered lists
        assert np.array_equal(r.candidate_lists[l], ref["candidate_lists"][l]), l
        assert np.array_equal(r.kept_lists[l], ref["kept_lists"][l]), l
    assert (r.dropped_bound, r.n_dropped, r.certified, r.n_found) == (ref["dropped_bound"], ref["n_dropped"], ref["certified"],
                                                                     ref["n_found"])
    assert r.index.tolist() == ref["index"].tolist() and r.score.tolist() == ref["score"].tolist()
    assert r.poses.tobytes() == ref["poses"].tobytes()
    K = len(r.index)
    if r.certified == K:                                                    # then the result is the exhaustive ranking
        ids, sc = BR.exhaustive_ranking(BE.exhaustive(name), K, c["kw"].get("min_score", 1))
        assert r.index.tolist() == ids.tolist() and r.score.tolist() == sc.tolist()


def check(name, scratch=None):
    r = raw_search(name, True, scratch)
    equals_the_restatement(name, r)
    same_search(raw_search(name, False, scratch), r)                        # the trace changes nothing
    return r


ONE_BY_ONE = sorted(n for n in BE.RAW if n.startswith(("chunk_", "far_", "pad_", "count_")))


@pytest.mark.parametrize("name", ONE_BY_ONE)
def test_the_raw_search_equals_the_restatement(name):
    check(name)


def test_a_count_outside_the_capacity_is_clamped():
    same_search(raw_search("count_beyond_cap"), raw_search("count_at_cap"))
    same_search(raw_search("count_negative"), raw_search("count_zero"))
    assert raw_search("count_negative").n_found == 0 and raw_search("count_beyond_cap").n_slice == 256


@pytest.mark.parametrize("cap", BE.SEG_CAPS)
def test_the_threshold_with_every_segment_length_and_cut_score(cap):
    """all frontiers and min_scores of one cap on one scratch, with the trace; then again in the opposite order without it:
    every search follows another one and must still equal its own first run (the threshold leaves the histogram at zero)"""
    names = [f"seg_cap{cap}_f{F}_ms{ms}" for F in BE.SEG_FRONTIERS for ms in BE.SEG_MIN_SCORES]
    scratch = scratch_for(cap, 16, max(BE.SEG_FRONTIERS))
    first = {}
    for n in names:
        first[n] = raw_search(n, True, scratch)
        equals_the_restatement(n, first[n])
    for n in reversed(names):
        same_search(raw_search(n, False, scratch), first[n])


def test_a_score_equal_to_the_capacity_is_counted_in_the_last_bin():
    scratch = scratch_for(1024, 1, 64)
    a, b = check("seg_last_bin", scratch), check("seg_last_bin_f32", scratch)
    assert a.score.tolist() == [1024] * 8 and b.dropped_bound == 1024 and b.kept.tolist() == [32, 25, 9]
    same_search(raw_search("seg_last_bin", False, scratch), a)              # after a cut in the last bin
    same_search(raw_search("seg_last_bin_f32", False, scratch), b)


def test_the_frontier_limits_on_one_scratch():
    scratch = scratch_for(512, 16, 65536)                                   # sized for the larger
    big = check("frontier_65536", scratch)
    one = check("frontier_1", scratch)
    kept = check("frontier_1_min_score_0", scratch)
    assert one.kept[3] == 1 and one.n_found == 0 and kept.n_found == 1 and big.kept[0] > 12 * BE.SCAN_BLOCK
    same_search(raw_search("frontier_65536", False, scratch), big)


@pytest.mark.parametrize("grid", ["far_w_l3", "far_h_l3", "far_w_l0", "pad_l7", "ones_9x9"])
def test_the_pooled_levels_at_the_storage_limit_equal_the_restatement(grid):
    g = BE.GRIDS[grid]
    ctx = context(grid)
    H, W = g["G0"].shape
    pad = (1 << g["L"]) - 1
    for l in range(g["L"] + 1):
        out = torch.zeros((H + pad, W + pad), dtype=torch.uint8, device="cuda")
        ctx.bbs_map_level(l, out.data_ptr())
        assert np.array_equal(out.cpu().numpy(), BR.stored(g["G0"], g["L"], l)), l
    ctx.check_errors(stream())

