"""GPU tests of the rules that include/sps_hip.h documents for the radius grid and the localisers, on the inputs where
they decide the result (tests/boundary_inputs.py; their properties are pinned by tests/test_boundary_inputs_cpu.py):
ties to the lowest map index, the inclusive d2 <= r*r, floor on a cell face, at negative coordinates and at the key limit,
scans that do not fill their last workgroup or launch B's runs of blocks, the exits of the 6 x 6 solve, the edges of the
thinning.  The other localiser tests run on random data and assert that these cases are absent.

Tolerances: bit-equality, and the two bounds derived in test_hip_localiser.py (n_corr * 2^-52 * sum |t|) and
test_hip_ndt.py ((m + 6) * 2^-52 * sum |t|).  Nothing else."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import boundary_inputs as BI
from tests import localiser_reference as LR
from tests import ndt_reference as NR

pytestmark = pytest.mark.gpu

CAP = 4096
THIN = 2.0 ** -5          # thinning leaf below the 2^-4 spacing of the dyadic set: every row is its own voxel and survives
BLOCK_EDGES = (1, 31, 32, 33, 255, 256, 257, 511, 513)      # 1, 8, 9, 16, 17 workgroups of LOC_PTS = 32, around LOC_SEG = 8


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rows32(xyz):
    out = np.zeros((len(xyz), 4), dtype=np.float32)
    out[:, :3] = xyz
    assert np.array_equal(out[:, :3].astype(np.float64), xyz)          # the scan is exact in float32
    return out


def align_points(loc, pts, T, iters):
    """sps_loc_align / sps_ndt_align on float64 points as given (the wrapper's thinning takes float32 rows; this is its
    submit() without that step) -> PoseResult with the normal rows"""
    from sps_amd.localiser import PendingPose, _pose_layout
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    n, K = len(pts), int(iters)
    assert n <= loc.capacity
    if n:
        loc._pts[:n].copy_(torch.from_numpy(pts))
    n_dev = torch.full((1,), n, dtype=torch.int32, device="cuda")
    o = _pose_layout(K, True)
    out = torch.zeros(o["total"], dtype=torch.float64, device="cuda")
    base = out.data_ptr()
    loc._align(n_dev.data_ptr(), np.asarray(T, dtype=np.float64), K, base + o["T_out"] * 8, base + o["status"] * 8,
               base + o["trace"] * 8 if K else None, base + o["normal"] * 8 if K else None, stream())
    torch.cuda.synchronize()
    loc.ctx.check_errors(stream())
    ev = torch.cuda.Event()
    ev.record()
    return PendingPose(K, True, out.cpu(), ev, None).result()


def icp(map_xyz, r=1.0, **kw):
    from sps_amd.localiser import ScanToMapLocaliser
    kw = {**dict(max_distance=r, leaf=THIN, min_correspondences=1, capacity=CAP), **kw}
    return ScanToMapLocaliser(map_xyz, **kw)


def ndt(map_xyz, neighbours=7, **kw):
    from sps_amd.localiser import NDTLocaliser
    kw = {**dict(resolution=1.0, neighbours=neighbours, leaf=THIN, min_correspondences=1, capacity=CAP), **kw}
    return NDTLocaliser(map_xyz, **kw)


def assert_terms_within(res_normal, terms, n_addends_factor, tag):
    """|device - fsum| <= factor * 2^-52 * sum |t| for all 28 entries (terms carry b's sign)"""
    for k in range(28):
        sum_abs = math.fsum(np.abs(terms[:, k]))
        bound = n_addends_factor * 2.0 ** -52 * sum_abs
        exact = math.fsum(terms[:, k])
        print(f"{tag} normal[{k}]: device {res_normal[k]!r} exact {exact!r} |diff| {abs(res_normal[k] - exact):.3e} bound {bound:.3e}")
        assert abs(res_normal[k] - exact) <= bound, (tag, k)


# ---- radius query on the lattice -------------------------------------------------------------------------------------------
def exact_cell_submap(map_xyz, r):
    """DeviceRadiusSubmap with cell_size = r, which sps_radius_grid_upload allows (cell_size >= r) and the ICP uses; the
    wrapper itself always takes r (1 + 1e-7), which moves every face off the lattice.  A context of its own."""
    from sps_amd import _native
    from sps_amd.datasets.blt_dataset import DeviceRadiusSubmap, radius_grid_cells
    sub = DeviceRadiusSubmap(map_xyz, r, ctx=_native.Context(0))
    xyz = dev(np.ascontiguousarray(map_xyz, dtype=np.float64))
    keys, start, pts = radius_grid_cells(xyz, r)
    sub.ctx.radius_grid_upload(keys.contiguous().data_ptr(), start.data_ptr(), pts.data_ptr(), xyz.data_ptr(), len(keys), len(xyz),
                               r, r, stream())
    return sub


def sorted_lists(flat, counts):
    """a concatenation of per-point lists -> the same with every list sorted (rows: lexicographically)"""
    owner = np.repeat(np.arange(len(counts)), counts)
    flat = np.asarray(flat)
    keys = (flat,) if flat.ndim == 1 else tuple(flat[:, k] for k in range(flat.shape[1] - 1, -1, -1))
    return flat[np.lexsort(keys + (owner,))]


@pytest.mark.parametrize("c", [0.1, 0.7, 1.3, 1.0])
def test_grid_cells_group_by_division(c):
    """radius_grid_cells on the device groups by floor(v / c), a true division (torch's device kernel turns a division by a
    Python number into a product with 1 / c, which is the other rule): keys, starts and lists equal numpy's"""
    from sps_amd.datasets.blt_dataset import radius_grid_cells
    mp = BI.lattice(c)
    assert c == 1.0 or np.any(BI.floor_div(mp, c) != BI.floor_mul(mp, c))
    keys, start, pts = radius_grid_cells(dev(mp), c)
    cell = BI.floor_div(mp, c) + (1 << 20)
    want = (cell[:, 2] << 42) | (cell[:, 1] << 21) | cell[:, 0]
    order = np.argsort(want, kind="stable")
    ukeys, counts = np.unique(want, return_counts=True)
    assert np.array_equal(keys.cpu().numpy(), ukeys)
    assert np.array_equal(start.cpu().numpy(), np.r_[0, np.cumsum(counts)])
    assert np.array_equal(pts.cpu().numpy(), order)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("c", [0.1, 0.7, 1.3, 1.0])
def test_radius_query_on_the_lattice(c, dtype):
    from sps_amd.datasets.blt_dataset import DeviceRadiusSubmap, device_item
    from sps_amd import _native
    mp = BI.lattice(c)
    scan = mp.astype(dtype)
    ref = BI.hit_lists(scan.astype(np.float64), mp, c)
    ref_counts = np.array([len(l) for l in ref])
    ref_flat = np.concatenate(ref)
    assert ref_counts.min() >= 1 and ref_counts.sum() > len(mp)
    labels = (np.arange(len(scan)) % 3).astype(dtype)
    ds = SimpleNamespace(scans=[np.c_[scan, labels].astype(dtype)], map=mp)
    want_sub = sorted_lists(mp[ref_flat].astype(np.float32), ref_counts)
    for name, sub in (("cell = r", exact_cell_submap(mp, c)), ("wrapper", DeviceRadiusSubmap(mp, c, ctx=_native.Context(0)))):
        idx, counts = sub.query(scan)
        idx, counts = idx.cpu().numpy(), counts.cpu().numpy()
        lost = int(np.sum(ref_counts > counts))
        print(f"c = {c} {np.dtype(dtype).name} {name}: {ref_counts.sum()} hits wanted, {counts.sum()} found, {lost} points short")
        assert np.array_equal(counts, ref_counts), (name, np.nonzero(counts != ref_counts)[0][:8])
        assert np.array_equal(sorted_lists(idx, counts), ref_flat), name                   # the hit set of every scan point
        item = device_item(ds, 0, sub).cpu().numpy()
        n = len(scan)
        assert item.shape == (n + len(ref_flat), 5)
        assert np.array_equal(item[:n], np.c_[scan.astype(np.float32), np.ones(n, np.float32), labels.astype(np.float32)])
        assert np.array_equal(sorted_lists(item[n:, :3], ref_counts), want_sub)
        assert (item[n:, 3] == 0).all() and (item[n:, 4] == 1).all()
        # the fused item kernel (the scan in its own dtype; float rows are promoted on the device)
        raw = dev(ds.scans[0])
        rows = torch.full((n + len(ref_flat) + 16, 6), -7.0, dtype=torch.float32, device="cuda")
        n_rows = torch.zeros(4, dtype=torch.int32, device="cuda")
        sub.ctx.radius_item(raw.data_ptr(), dtype == np.float64, 4, n, 2.0, None, rows.data_ptr(), 6, rows.shape[0],
                            n_rows.data_ptr(), stream())
        torch.cuda.synchronize()
        sub.ctx.check_errors(stream())
        got = rows.cpu().numpy()
        assert int(n_rows[0].item()) == n + len(ref_flat)
        assert np.array_equal(got[:n, 1:], item[:n]) and (got[:n + len(ref_flat), 0] == 2.0).all()
        assert np.array_equal(sorted_lists(got[n:n + len(ref_flat), 1:4], ref_counts), want_sub)
        assert (got[n + len(ref_flat):] == -7.0).all()                                     # nothing written past the count


# ---- ICP: exact sums on the dyadic set -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dy():
    return BI.dyadic()


@pytest.fixture(scope="module")
def dy_icp(dy):
    return icp(dy["map"])


def icp_dyadic_exact(loc, dy, n, t, count=None):
    rows = rows32(dy["q"][:n] - np.asarray(t))
    n_corr, terms, _ = BI.icp_terms(rows[:, :3].astype(np.float64), dy["map"], BI.DYADIC_R, BI.pose_of(t))
    res = loc(dev(rows), n if count is None else count, BI.pose_of(t), with_normal=True, iterations=1)
    assert res.n_points == n and res.iterations == 1
    assert res.n_corr == n_corr and res.trace[0, 0] == n_corr
    want = BI.exact_normal(terms)
    assert res.normal[0].tobytes() == want.tobytes(), (n, t, np.nonzero(res.normal[0] != want)[0])
    assert res.trace[0, 1] == want[27]
    return res


@pytest.mark.parametrize("t", BI.DYADIC_SHIFTS)
def test_icp_ties_and_the_r_boundary_bit_for_bit(dy, dy_icp, t):
    """ties to the lowest map index, d2 == r*r inside, one ulp beyond outside: all 28 sums are exact, so they equal
    math.fsum of the brute-force terms bit for bit, whatever the order"""
    res = icp_dyadic_exact(dy_icp, dy, BI.DYADIC_N, t)
    assert res.n_corr == 312


@pytest.mark.parametrize("n", BLOCK_EDGES)
def test_icp_block_and_segment_edges(dy, dy_icp, n):
    a = icp_dyadic_exact(dy_icp, dy, n, BI.DYADIC_SHIFTS[1])
    rows = dev(rows32(dy["q"][:n] - np.asarray(BI.DYADIC_SHIFTS[1])))
    big = torch.tensor([n + 77], dtype=torch.int32, device="cuda")     # a device count beyond the rows: clamped to them
    b = dy_icp(rows, big, BI.pose_of(BI.DYADIC_SHIFTS[1]), with_normal=True, iterations=1)
    assert (b.n_points, b.n_corr, b.status) == (a.n_points, a.n_corr, a.status)
    assert b.normal.tobytes() == a.normal.tobytes() and b.pose.tobytes() == a.pose.tobytes()


# ---- ICP on the lattice ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [0.7, 1.3])
def test_icp_on_the_lattice(c):
    scan, mp = BI.lattice_split(c)
    n_corr, terms, a = BI.icp_terms(scan, mp, c, np.eye(4))
    assert a["ties"] > 100 and a["on_r"] > 0
    res = align_points(icp(mp, r=c), scan, np.eye(4), 1)
    print(f"c = {c}: n_corr device {res.n_corr} reference {n_corr}")
    assert res.n_corr == n_corr and res.iterations == 1
    signed = terms.copy()
    signed[:, 21:27] *= -1.0
    assert_terms_within(res.normal[0], signed, n_corr, f"lattice {c}")


# ---- NDT: block and segment edges ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dy_ndt(dy):
    mp = BI.ndt_block_map(dy["q"])
    return {7: ndt(mp, 7), 1: ndt(mp, 1), "cmap": NR.cells(mp, 1.0)}


@pytest.mark.parametrize("neighbours", [7, 1])
@pytest.mark.parametrize("n", BLOCK_EDGES)
def test_ndt_block_and_segment_edges(dy, dy_ndt, n, neighbours):
    t = BI.DYADIC_SHIFTS[2]
    T = BI.pose_of(t)
    rows = rows32(dy["q"][:n] - np.asarray(t))
    ref = NR.align(rows[:, :3].astype(np.float64), dy_ndt["cmap"], T, iters=1, neighbours=neighbours, min_corr=1)
    assert ref["n_corr"] == n and ref["boundary"] == 0
    loc = dy_ndt[neighbours]
    res = loc(dev(rows), n, T, with_normal=True, iterations=1)
    assert res.n_points == n and res.iterations == 1 and res.n_corr == n
    terms = ref["terms"][0]
    assert_terms_within(res.normal[0], terms, len(terms) + 6, f"ndt n = {n}")
    big = torch.tensor([n + 77], dtype=torch.int32, device="cuda")
    b = loc(dev(rows), big, T, with_normal=True, iterations=1)
    assert (b.n_points, b.n_corr, b.status) == (res.n_points, res.n_corr, res.status)
    assert b.normal.tobytes() == res.normal.tobytes() and b.pose.tobytes() == res.pose.tobytes()


# ---- NDT: cell faces and the key limit -------------------------------------------------------------------------------------
@pytest.mark.parametrize("neighbours", [7, 1])
def test_ndt_cell_faces_and_the_key_limit(neighbours):
    mp, q, names = BI.ndt_face_case()
    cmap = NR.cells(mp, 1.0)
    loc = ndt(mp, neighbours)
    d1, d2 = NR.gauss(loc.outlier_ratio, 1.0)
    t = (0.5, -0.25, 2.0)
    T = BI.pose_of(t)
    pts = q - np.asarray(t)
    assert np.array_equal(LR.transform(pts, T), q)                     # q is exact
    ref = NR.align(pts, cmap, T, iters=1, neighbours=neighbours, min_corr=1)
    res = align_points(loc, pts, T, 1)
    assert res.n_corr == ref["n_corr"] and (neighbours == 1 or ref["n_corr"] == len(q) - 3)
    terms = ref["terms"][0]
    assert_terms_within(res.normal[0], terms, len(terms) + 6, "faces")
    # point by point: whether it counts, and the score of its contributing cells
    h = NR.hits(q, cmap, neighbours, d1, d2)
    for i, name in enumerate(names):
        one = align_points(loc, pts[i:i + 1], T, 1)
        mine = h["terms"][h["i"] == i, 27]
        print(f"{name}: cells {h['c'][h['i'] == i].tolist()} score device {one.normal[0, 27]!r} reference {math.fsum(mine)!r}")
        assert one.n_corr == (1 if len(mine) else 0), name
        assert abs(one.normal[0, 27] - math.fsum(mine)) <= (len(mine) + 6) * 2.0 ** -52 * math.fsum(np.abs(mine)), name
    # -0.0: R p + t gives it only from p = (-0.0, < 0, < 0) and t.x = -0.0; its cell is 0, not -1
    Tz = np.eye(4)
    Tz[0, 3] = -0.0
    pz = np.array([[-0.0, -0.5, -0.5]])
    qz = LR.transform(pz, Tz)
    assert qz[0, 0] == 0.0 and np.signbit(qz[0, 0])
    hz = NR.hits(qz, cmap, neighbours, d1, d2)
    assert 0 in hz["c"].tolist() and NR.cell_index(qz, 1.0)[0, 0] == 0
    one = align_points(loc, pz, Tz, 1)
    mine = hz["terms"][:, 27]
    assert one.n_corr == 1
    assert abs(one.normal[0, 27] - math.fsum(mine)) <= (len(mine) + 6) * 2.0 ** -52 * math.fsum(np.abs(mine))


# ---- the exits of the solve (launch B), through both localisers ------------------------------------------------------------
X_AXIS = np.array([[x, 0.0, 0.0] for x in (1.5, 2.5, 3.5, 5.5, 6.5, 9.5)])             # cell centres on the x axis
PLANE = np.array([[1.5, 0.5, 0.0], [2.5, -1.5, 0.0], [-3.5, 2.5, 0.0], [-1.5, -2.5, 0.0], [4.5, 3.5, 0.0], [0.5, -0.5, 0.0]])
SHIFT = np.array([0.125, -0.0625, 0.25])


def solver_case(kind, name):
    """(localiser factory, scan points, reference align(pts, T, **kw)) for the ICP or the NDT on the point set `name`"""
    pts = dict(axis=X_AXIS, single=X_AXIS[:1], plane=PLANE, subset=None)[name]
    if kind == "icp":
        if name == "subset":
            d = BI.dyadic()
            mp = d["map"]
            pts = mp[np.all(mp * 16 == np.round(mp * 16), axis=1)][:200]                  # scan == a map subset: e = 0
        else:
            mp = pts + SHIFT                                                               # one partner each, e = -SHIFT
        index = BI.AllPairs(mp, 1.0)
        return (lambda **kw: icp(mp, **kw)), pts, (lambda p, T, **kw: LR.align(p, index, T, **kw))
    if name == "subset":
        cells = [(x, y, z) for x in range(-2, 2) for y in range(-2, 2) for z in range(-2, 2)]
        mp = BI.cell_points(cells)
        pts = np.asarray(cells, dtype=np.float64) + 0.5                                    # the cell means, exactly: x = q - mean = 0
    else:
        mp = BI.cell_points(np.unique(np.floor(pts).astype(np.int64), axis=0))
    cmap = NR.cells(mp, 1.0)
    return (lambda **kw: ndt(mp, 1, **kw)), pts, (lambda p, T, **kw: NR.align(p, cmap, T, neighbours=1, **kw))


def same_exit(res, ref, T):
    assert (res.status, res.iterations, res.n_corr) == (ref["status"], ref["iterations"], ref["n_corr"])
    if ref["status"] in (2, 3):
        assert res.pose.tobytes() == np.asarray(T, dtype=np.float64).tobytes()             # T_init, bit for bit


T_DYADIC = BI.pose_of((0.25, -0.5, 0.125))


@pytest.mark.parametrize("kind", ["icp", "ndt"])
def test_min_corr_is_inclusive(kind):
    make, pts, ref_align = solver_case(kind, "plane")
    p = pts - T_DYADIC[:3, 3]
    n = len(pts)
    for min_corr, want in ((n, None), (n + 1, 2)):
        ref = ref_align(p, T_DYADIC, iters=1, min_corr=min_corr)
        assert ref["n_corr"] == n and (ref["status"] == 2) == (want == 2)
        res = align_points(make(min_correspondences=min_corr), p, T_DYADIC, 1)
        same_exit(res, ref, T_DYADIC)
        if want is None:
            assert res.status in (0, 1) and res.pose.tobytes() != T_DYADIC.tobytes()       # n_corr == min_corr proceeds


@pytest.mark.parametrize("name", ["single", "axis", "plane"])
@pytest.mark.parametrize("kind", ["icp", "ndt"])
def test_singular_systems_end_as_the_restatement_says(kind, name):
    """Points on the x axis make the first column of J zero, so H[0][0] is exactly 0 on either side and the first pivot
    fails: status 3 whatever exp rounds to.  Points spread over a plane through the origin are regular: no status 3."""
    make, pts, ref_align = solver_case(kind, name)
    T = np.eye(4)
    ref = ref_align(pts, T, iters=3, min_corr=1)
    assert ref["n_corr"] == len(pts)
    assert (ref["status"] == 3 and ref["iterations"] == 1) if name in ("single", "axis") else ref["status"] != 3
    res = align_points(make(), pts, T, 3)
    if ref["status"] == 3:
        same_exit(res, ref, T)
        assert (res.trace[0, 2:] == 0).all()
    else:
        assert res.status in (0, 1) and res.n_corr == len(pts)
    if kind == "icp" and name == "plane":
        # exact sums and a solve of correctly rounded operations only: the step lengths agree bit for bit
        one, ref1 = align_points(make(), pts, T, 1), ref_align(pts, T, iters=1, min_corr=1)
        assert one.trace[0].tobytes() == ref1["trace"][0].tobytes() and one.status == ref1["status"] == 1


@pytest.mark.parametrize("kind", ["icp", "ndt"])
def test_iteration_limits_and_tolerances(kind):
    make, pts, ref_align = solver_case(kind, "plane")
    p = pts - T_DYADIC[:3, 3]
    zero = align_points(make(), p, T_DYADIC, 0)                          # iters = 0
    assert (zero.status, zero.iterations, zero.n_corr) == (1, 0, 0) and zero.pose.tobytes() == T_DYADIC.tobytes()
    strict = align_points(make(tol_t=0.0, tol_r=0.0), p, T_DYADIC, 6)    # |v| < 0 never holds
    assert (strict.status, strict.iterations) == (1, 6) and len(strict.trace) == 6
    loose = align_points(make(tol_t=math.inf, tol_r=math.inf), p, T_DYADIC, 6)
    assert (loose.status, loose.iterations) == (0, 1)
    assert loose.trace[0].tobytes() == strict.trace[0].tobytes()         # the same first iteration


@pytest.mark.parametrize("kind", ["icp", "ndt"])
def test_a_zero_step_leaves_the_identity_bit_for_bit(kind):
    """The scan is a map subset (ICP) or the cell means (NDT) at the identity: g = 0, so x = 0, Rodrigues takes its
    first-order branch, the pose stays the identity and the first iteration converges; with tolerance 0 it never does."""
    make, pts, ref_align = solver_case(kind, "subset")
    T = np.eye(4)
    ref = ref_align(pts, T, iters=4, min_corr=1)
    assert (ref["status"], ref["iterations"]) == (0, 1) and ref["pose"].tobytes() == T.tobytes()
    assert (ref["trace"][0, 2:] == 0).all() and ref["n_corr"] == len(pts)
    res = align_points(make(), pts, T, 4)
    same_exit(res, ref, T)
    assert res.pose.tobytes() == T.tobytes() and (res.trace[0, 2:4] == 0).all()
    strict = align_points(make(tol_t=0.0, tol_r=0.0), pts, T, 4)
    assert (strict.status, strict.iterations) == (1, 4) and strict.pose.tobytes() == T.tobytes()


# ---- thinning edges --------------------------------------------------------------------------------------------------------
def downsample(rows, n_dev, leaf, cap):
    from sps_amd import _native
    from sps_amd.models.models import get_context
    ctx = get_context(0, stream())
    d = dev(rows)
    out = torch.full((cap + 2, 3), -7.0, dtype=torch.float64, device="cuda")
    count = torch.full((1,), -3, dtype=torch.int32, device="cuda")
    nd = torch.tensor([n_dev], dtype=torch.int32, device="cuda")
    scratch = torch.empty(_native.lib.sps_loc_downsample_scratch(len(rows)), dtype=torch.uint8, device="cuda")
    ctx.loc_downsample(d.data_ptr(), rows.shape[1], len(rows), nd.data_ptr(), leaf, out.data_ptr(), cap, count.data_ptr(),
                       scratch.data_ptr(), stream())
    torch.cuda.synchronize()
    ctx.check_errors(stream())
    return out.cpu().numpy(), int(count.item())


def assert_thinned_exactly(rows, n, leaf, cap):
    keep, want = LR.downsample(rows, n, leaf, cap)
    got, count = downsample(rows, n, leaf, cap)
    assert count == len(keep), (n, cap)
    assert got[:count].tobytes() == want.tobytes(), (n, cap)           # the survivors, their order, the sign of a zero
    assert (got[count:] == -7.0).all(), (n, cap)                       # nothing written past the count
    return len(keep)


def test_thinning_on_voxel_faces_and_at_the_key_limit():
    rows = BI.thinning_rows()
    survivors = assert_thinned_exactly(rows, len(rows), 0.5, len(rows))
    assert survivors == 8
    assert_thinned_exactly(rows, len(rows), 0.5, survivors)            # cap == the survivor count
    assert_thinned_exactly(rows, len(rows), 0.5, survivors - 1)        # one below: saturates
    assert_thinned_exactly(rows[::-1].copy(), len(rows), 0.5, len(rows))   # the other row of every voxel comes first


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2047, 2048, 2049])
def test_thinning_around_the_workgroup_size(n):
    """SCAN_BLOCK = 1024 rows per workgroup: one below, at and one above one and two workgroups; the special rows sit at the
    end, in the last (partly filled) workgroup"""
    special = BI.thinning_rows()
    rows = np.concatenate([BI.thinning_fill(n - len(special)), special])
    assert len(rows) == n
    survivors = assert_thinned_exactly(rows, n, 0.5, n)
    assert_thinned_exactly(rows, n, 0.5, survivors)
    assert_thinned_exactly(rows, n, 0.5, survivors - 1)
    assert_thinned_exactly(rows, n - 1, 0.5, n)                        # the device count one below the rows
