"""GPU tests of the global search (sps_amd.localiser.NDTLocaliser.global_search / localise_global; C ABI: the "NDT
localiser, global search" section of include/sps_hip.h) against the numpy restatement in tests/bbs_reference.py.  Every
quantity is an integer or a pose whose operations the restatement fixes, so every comparison is exact.

The cases (tests/bbs_inputs.py) go through the wrapper: a grid of 37 x 21 cells with three pooled levels (no multiple of
8 on either axis, so children fall outside the grid and pooled cells reach into the negative pad), a grid of one cell and
an all-zero one; 1, 3, 7 and 16 yaws; 0, 1, 255, 256 and 257 points in the scan slice (the edges of the 256 threads of the
offsets kernel; all within one chunk of the 1024 offsets that the score kernel stages at a time) and 2544 points (three
chunks, the last one partial); points exactly on cell edges, off the grid on all four sides, rows that are not finite; a
slice that excludes every point; a frontier below the survivors of the first level with equal scores on both sides of the
cut, within one workgroup of the compaction (160 and 240 slots) and, in the cut_* cases, across four to six workgroups
(3344 to 6000 slots of a grid with one pooled level, frontiers 900, 901, 984 and 1500: ties kept in several workgroups and
dropped in the quota's own and in later ones, void slots in front of the cut, a frontier that the scores above the cut
fill exactly) with 64 results picked from 1500 leaves that tie at two or three scores; a frontier so small that the
certificate fails; more results asked for than leaves found; a min_score that prunes everything.  tests/test_bbs_cpu.py
asserts from the restatement alone that each case sits where it is said to.  Capacities other than 4096, exact row counts
on the chunk edges, the threshold kernel's segment lengths, offsets near the 16-bit limit and counts or frontiers on
their limits need the raw ABI: tests/test_hip_bbs_edges.py."""
import numpy as np
import pytest
import torch

from tests import bbs_inputs as BI
from tests import bbs_reference as BR

pytestmark = pytest.mark.gpu


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_LOCS = {}


def localiser(name):
    """one localiser per (map, grid) of the cases, built once"""
    from sps_amd.localiser import NDTLocaliser
    c = BI.CASES[name]
    key = (id(c["map"]), tuple(sorted((k, str(v)) for k, v in c["grid"].items())))
    if key not in _LOCS:
        _LOCS[key] = NDTLocaliser(c["map"], resolution=1.0, leaf=BI.LEAF, capacity=4096, global_grid=c["grid"])
    return _LOCS[key]


def run(name, rows=None, **over):
    c = BI.CASES[name]
    rows = dev(c["rows"]) if rows is None else rows
    kw = dict(c["kw"], **over)
    return localiser(name).global_search(rows, len(c["rows"]), c["A"], **kw)


def same_search(a, b):
    for f in ("index", "score", "poses", "candidates", "kept"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    for f in ("n_found", "certified", "dropped_bound", "n_dropped", "n_slice", "n_points"):
        assert getattr(a, f) == getattr(b, f), f


@pytest.mark.parametrize("name", ["main", "one_cell", "zero_map"])
def test_the_pooled_levels_equal_the_restatement(name):
    loc, c = localiser(name), BI.CASES[name]
    G0, i0, j0 = BR.grid(c["map"], BI.R, c["grid"]["map_z"])
    g = loc._global
    assert (g["i0"], g["j0"], g["W"], g["H"]) == (i0, j0, G0.shape[1], G0.shape[0]) and np.array_equal(g["G0"], G0)
    for l in range(c["grid"]["levels"] + 1):
        assert np.array_equal(loc.global_level(l), BR.stored(G0, c["grid"]["levels"], l)), l
    loc.ctx.check_errors(stream())


@pytest.mark.parametrize("name", sorted(BI.CASES))
def test_the_search_equals_the_restatement(name):
    c, ref = BI.CASES[name], BI.reference(name)
    r = run(name, trace=True).result()
    L = c["grid"]["levels"]
    assert r.n_slice == ref["n_slice"] == c["n"]
    assert r.candidates.tolist() == ref["candidates"].tolist() and r.kept.tolist() == ref["kept"].tolist()
    for l in range(L, -1, -1):                                              # as ordered lists
        assert r.candidate_lists[l].tolist() == ref["candidate_lists"][l].tolist(), l
        assert r.kept_lists[l].tolist() == ref["kept_lists"][l].tolist(), l
    assert (r.dropped_bound, r.n_dropped, r.certified, r.n_found) == (ref["dropped_bound"], ref["n_dropped"], ref["certified"],
                                                                     ref["n_found"])
    assert r.index.tolist() == ref["index"].tolist() and r.score.tolist() == ref["score"].tolist()
    assert r.poses.tobytes() == ref["poses"].tobytes()
    K = len(r.index)
    if r.certified == K:                                                    # then the result is the exhaustive ranking
        ids, sc = BR.exhaustive_ranking(BI.exhaustive(name), K, c["kw"].get("min_score", 1))
        assert r.index.tolist() == ids.tolist() and r.score.tolist() == sc.tolist()
    plain = run(name).result()                                              # the trace changes nothing
    same_search(plain, r)
    localiser(name).ctx.check_errors(stream())


def test_two_calls_give_the_same_bits_and_scratch_is_reused_across_shapes():
    a = run("main").result()
    run("uncertified").result()                                             # another frontier on the same scratch
    run("a7_n255").result()                                                 # another yaw count
    b = run("main").result()
    same_search(a, b)


def test_a_call_behind_a_kernel_on_the_callers_stream_sees_its_data():
    c = BI.CASES["main"]
    first = run("main").result()
    scan = dev(c["rows"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rows = torch.zeros_like(scan)
        a = torch.randn((2048, 2048), device="cuda")
        for _ in range(8):
            a = (a @ a).clamp_(-1.0, 1.0)                                   # work in front of the copy
        rows.copy_(scan + a[0, 0] * 0.0)                                    # the rows exist only once the stream gets here
        count = torch.full((1,), len(scan), dtype=torch.int32, device="cuda")
        p = localiser("main").global_search(rows, count, c["A"], **c["kw"])
    r = p.result()
    torch.cuda.current_stream().wait_stream(side)
    same_search(r, first)


def test_rows_that_are_not_finite_and_points_the_kernel_must_skip():
    """NaN and infinite rows never pass the thinning; given to the search directly, points that are not finite, or whose
    cell quotient exceeds 2^20, score nothing and the rest scores as without them"""
    c, ref = BI.CASES["a7_n255"], BI.reference("a7_n255")
    rows = np.concatenate([c["rows"], np.array([[np.nan, 0, 0.5, 0], [np.inf, 1, 0.5, 0], [0, -np.inf, 0.5, 0]], np.float32)])
    r = localiser("a7_n255").global_search(dev(rows), len(rows), c["A"], **c["kw"]).result()
    assert r.index.tolist() == ref["index"].tolist() and r.score.tolist() == ref["score"].tolist() and r.n_slice == ref["n_slice"]
    from sps_amd import _native
    loc = localiser("a7_n255")
    pts = BI.thinned(c["rows"])
    bad = np.array([[np.nan, 0.0, 0.5], [np.inf, 0.0, 0.5], [0.0, -np.inf, 0.5], [0.0, 0.0, np.nan], [6.0e5, 0.0, 0.5],
                    [0.0, -6.0e5, 0.5], [1.7e308, -1.7e308, 0.5]])             # the last: u overflows at 2 pi / 7
    both = np.concatenate([bad[:3], pts, bad[3:]])
    with np.errstate(invalid="ignore", over="ignore"):
        want = BR.search(ref["G0"], 3, BI.R, ref["i0"], ref["j0"], both, c["A"], **c["kw"])
    assert want["n_slice"] == ref["n_slice"] + 3 and want["index"].tolist() == ref["index"].tolist()
    K, A, F = 8, c["A"], 16384
    p_dev, n_dev = dev(both), torch.full((1,), len(both), dtype=torch.int32, device="cuda")
    cs = dev(BR.yaw_table(A))
    top, score = torch.zeros(K, dtype=torch.int32, device="cuda"), torch.zeros(K, dtype=torch.int32, device="cuda")
    T_top, n_top = torch.zeros((K, 16), dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    info = torch.zeros(_native.BBS_INFO_WORDS, dtype=torch.int32, device="cuda")
    scratch = torch.empty(_native.lib.sps_bbs_search_scratch(len(both), A, F), dtype=torch.uint8, device="cuda")
    loc.ctx.bbs_search(p_dev.data_ptr(), n_dev.data_ptr(), len(both), np.eye(4), BI.R, ref["i0"], ref["j0"], *BI.SCAN_Z,
                       cs.data_ptr(), A, F, 1, K, top.data_ptr(), score.data_ptr(), T_top.data_ptr(), n_top.data_ptr(),
                       info.data_ptr(), None, scratch.data_ptr(), stream())
    assert top.cpu().tolist() == want["index"].tolist() and score.cpu().tolist() == want["score"].tolist()
    assert info.cpu()[:4].tolist() == [want["certified"], want["dropped_bound"], want["n_dropped"], want["n_slice"]]
    assert T_top.cpu().numpy().reshape(K, 4, 4).tobytes() == want["poses"].tobytes()
    loc.ctx.check_errors(stream())


def test_the_entry_points_refuse_what_the_header_says():
    from sps_amd import _native
    loc = localiser("main")
    with pytest.raises(_native.SpsError):
        loc.ctx.bbs_map_level(4, torch.zeros(1, dtype=torch.uint8, device="cuda").data_ptr())
    with pytest.raises(_native.SpsError, match="levels"):
        loc.ctx.bbs_map_build(torch.zeros(4, dtype=torch.uint8, device="cuda").data_ptr(), 2, 2, 8, stream())
    from sps_amd.localiser import NDTLocaliser
    plain = NDTLocaliser(BI.MAP, resolution=1.0, leaf=BI.LEAF, capacity=1024)
    with pytest.raises(ValueError, match="global_grid"):
        plain.global_search(dev(BI.CASES["main"]["rows"]), 10, 16)
    same_search(run("main").result(), run("main").result())                 # the failed build left the pyramid alone


# ---- search plus registration, on the synthetic corridor ---------------------------------------------------------------
@pytest.fixture(scope="module")
def corridor():
    from sps_amd.localiser import NDTLocaliser
    from tests.test_bbs_cpu import CORRIDOR, corridor_scene
    s = corridor_scene()
    loc = NDTLocaliser(s["map_xyz"], resolution=1.0, leaf=0.2, iterations=8, global_grid=CORRIDOR["grid"])
    return loc, s


def test_localise_global_equals_the_search_followed_by_submit_batch(corridor):
    from tests.test_bbs_cpu import CORRIDOR
    loc, s = corridor
    scan = dev(s["scan"])
    kw = dict(keep=4, scan_z=CORRIDOR["scan_z"])
    both = loc.localise_global(scan, len(scan), CORRIDOR["yaw_steps"], with_normal=True, **kw).result()
    search = loc.global_search(scan, len(scan), CORRIDOR["yaw_steps"], **kw).result()
    batch = loc.submit_batch(scan, len(scan), search.poses, with_normal=True).result()
    same_search(both.search, search)
    assert search.n_found == 4 and search.certified == 4
    assert both.batch.best == batch.best and both.pose.tobytes() == batch.pose.tobytes()
    assert both.batch.scores.tobytes() == batch.scores.tobytes() and both.batch.counts.tobytes() == batch.counts.tobytes()
    for x, y in zip(both.batch.results, batch.results):
        assert x.pose.tobytes() == y.pose.tobytes() and (x.status, x.iterations, x.n_corr) == (y.status, y.iterations, y.n_corr)
        assert x.trace.tobytes() == y.trace.tobytes() and x.normal.tobytes() == y.normal.tobytes()
    assert both.ok and both.index == int(search.index[both.batch.best])
    again = loc.localise_global(scan, len(scan), CORRIDOR["yaw_steps"], with_normal=True, **kw).result()
    assert again.pose.tobytes() == both.pose.tobytes() and again.search.index.tolist() == both.search.index.tolist()
    loc.ctx.check_errors(stream())
