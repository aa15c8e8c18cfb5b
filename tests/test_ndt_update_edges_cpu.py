"""CPU tests of the inputs in tests/ndt_update_edge_inputs.py: every builder has the property it is named for, so that the GPU
cases of tests/test_hip_ndt_update_edges.py reach the branch they are meant for; and the restatement
(tests/ndt_update_reference.py) is itself right at the new shapes, against a two-pass np.longdouble computation.  No GPU."""
import numpy as np
import pytest

from tests import ndt_reference as NR
from tests import ndt_update_edge_inputs as E
from tests import ndt_update_reference as UR

TOL_FLOOR = 1e-12              # this project's rule for float64 comparisons that differ only in the order of a sum
EYE = np.eye(4)


def cells_with_indices(pts, resolution=1.0):
    """{cell triple: ascending point indices}"""
    out = {}
    for i, c in enumerate(E.cell_index(pts, resolution)):
        out.setdefault(tuple(int(v) for v in c), []).append(i)
    return out


# ---- the builders have the properties they are named for -------------------------------------------------------------------
def test_dense_cells_hold_the_listed_batch_counts():
    for seed in (1, 2, 3):
        pts = E.dense_cells(seed)
        by = cells_with_indices(pts)
        assert len(pts) == 879 and [len(by[(i, 0, 0)]) for i in range(9)] == list(E.DENSE_COUNTS) and len(by) == 9
        # the permutation spreads every larger cell over the whole index range: no list is one run of consecutive indices
        assert all(by[(i, 0, 0)][-1] - by[(i, 0, 0)][0] > 2 * len(by[(i, 0, 0)]) for i in range(2, 9))
    # at the pyramid's coarse levels the cells merge into cells of several hundred points
    assert sorted(len(v) for v in cells_with_indices(E.dense_cells(1), 4.0).values()) == [130, 300, 449]
    assert max(len(v) for v in cells_with_indices(E.dense_cells(1), 2.0).values()) == 300


def test_bitmap_groups_hold_the_listed_indices():
    pts = E.bitmap_groups()
    by = cells_with_indices(pts)
    assert len(pts) == E.BITMAP_N == 4100
    for idx, c in zip((E.BITMAP_STRADDLE, E.BITMAP_WORDS, E.BITMAP_RUN, E.BITMAP_LATE), E.BITMAP_SPECIAL_CELLS):
        assert by[c] == list(idx), c
    assert E.BITMAP_STRADDLE == (0, 2047, 2048, 4095, 4096, 4099) and E.BITMAP_LATE[0] == 4097
    assert 190 <= len(by) - 4 <= 200                                           # the filler cells
    leads = np.array([v[0] for v in by.values()])
    assert (leads % 32 != 0).sum() > 150                                       # w0 = lead / 32 rounds down for most cells
    assert sum(1 for v in by.values() if v[0] // 2048 != v[-1] // 2048) > 190  # and nearly every list crosses a group border
    assert sorted(n % 32 for n in E.BITMAP_COUNTS) == [0, 0, 1, 1, 4, 31] and max(E.BITMAP_COUNTS) == E.BITMAP_N
    # every device count leaves the straddling cell at least one index on either side of the first border
    for n in E.BITMAP_COUNTS:
        kept = [i for i in E.BITMAP_STRADDLE if i < n]
        assert kept[:3] == [0, 2047, 2048] and (len(kept) == 6) == (n == 4100)


def test_full_limit_fills_the_bitmap():
    pts = E.full_limit()
    by = cells_with_indices(pts)
    assert len(pts) == E.MAX_POINTS == 65536 and len(by) == E.FULL_CELLS + 1 == 513
    assert by[E.FULL_EXTRA_CELL] == list(E.FULL_EXTRA) and by[E.FULL_EXTRA_CELL][0] == 0 and by[E.FULL_EXTRA_CELL][-1] == 65535
    assert sum(1 for i in E.FULL_EXTRA[1:-1] if i % 2048 == 0) == 4
    assert min(len(v) for c, v in by.items() if c != E.FULL_EXTRA_CELL) > 64     # every other cell takes several chunks


@pytest.mark.parametrize("k", [300, 3])
def test_many_cells_touch_more_cells_than_workgroups(k):
    pts = E.many_cells(k)
    m = UR.build(np.zeros((0, 3)), max(k, 4))
    assert UR.update(m, pts, EYE) == [k, k, 0, k]
    groups = min(max(k // 4, 1), 2048)                                         # the stats kernel's grid for cap = k
    assert k > groups and (groups == 1) == (k == 3)
    # forward, the leads follow the ids; reversed, they run against them
    ids = {int(key): c for c, key in enumerate(m["keys"])}
    order = [ids[int(key)] for key in NR.cell_key(E.cell_index(pts[::-1]))]
    assert order == list(range(k))[::-1]


def test_founder_run_cuts_beyond_the_first_block():
    cells = E.founder_cells()
    pts = E.founder_run()
    assert len(pts) == E.FOUNDER_N == 3000 and (E.cell_index(pts) == cells).all()
    seen, founder_at, repeats = {}, [], []
    for i, c in enumerate(map(tuple, cells)):
        if c in seen:
            repeats.append((i, seen[c]))                                       # (index, founder rank of its key)
        else:
            seen[c] = len(founder_at)
            founder_at.append(i)
    assert len(founder_at) == 2500 >= 2049 and len(repeats) == 500
    start = E.founder_start_map()
    assert len(cells_with_indices(start)) == 5 and not set(map(tuple, E.cell_index(start))) & set(seen)
    for n0, start_pts in ((0, np.zeros((0, 3))), (5, start)):
        for cut in E.FOUNDER_CUTS:
            m = UR.build(start_pts, n0 + cut)
            info = UR.update(m, pts, EYE)
            last = cut - 1                                                     # global rank of the last admitted founder
            assert last in (1022, 1023, 1024, 2047) and info[:3] == [n0 + cut, cut, 2500 - cut]
            assert int(m["keys"][-1]) == int(NR.cell_key(cells[founder_at[last]]))
            # the cut lies beyond the first 1024 points, where the in-block rank is not the global one
            assert founder_at[last] >= 1024 and founder_at[last] % 1024 != last % 1024
            # admitted and dropped keys both have later points that are not founders
            assert sum(1 for i, r in repeats if r <= last) > 50 and sum(1 for i, r in repeats if r > last) > 5
            assert info[3] == cut + sum(1 for i, r in repeats if r <= last)
            # a second run founds nothing and drops the same keys again
            assert UR.update(m, pts, EYE)[1:3] == [0, 2500 - cut] and m["dropped"] == 2 * (2500 - cut)


def test_one_key_sets():
    single, two = E.one_key(5000)
    assert len(single) == len(two) == 5000 and len(cells_with_indices(single)) == 1
    by = cells_with_indices(two)
    assert by[(0, 0, 0)] == list(range(0, 5000, 2)) and by[(7, 0, 0)] == list(range(1, 5000, 2))


def test_hash_cluster_homes_on_the_last_three_slots():
    cells = E.hash_cluster_cells()
    assert len(cells) == 20 >= 8 and {(1, 1, -5), (-5, -6, 2), (-8, 21, -3)} <= set(map(tuple, cells.tolist()))
    # hash64 as restated: two values worked out by hand from the definition with Python integers
    for k in (0x123456789ABCDEF, int(NR.cell_key(np.array([1, 1, -5])))):
        x, M = k, (1 << 64) - 1
        x ^= x >> 33
        x = (x * 0xff51afd7ed558ccd) & M
        x ^= x >> 33
        x = (x * 0xc4ceb9fe1a85ec53) & M
        x ^= x >> 33
        assert int(E.hash64(np.array([k], dtype=np.uint64))[0]) == x & 0xFFFFFFFF
    assert (E.radius_key(cells) == NR.cell_key(cells)).all()
    h = E.hash64(NR.cell_key(cells))
    for bits in range(10, 18):                                                 # 1024 .. 131 072 slots
        slots = 1 << bits
        home = (h & np.uint64(slots - 1)).astype(np.int64)
        assert home.min() >= slots - 3, bits
        # linear probing from there: at most three keys fit before the end, so the chain wraps at least 17 deep
        table = {}
        wrapped = 0
        for s in home:
            s, w = int(s), False
            while s in table:
                s, w = (s + 1) & (slots - 1), w or s + 1 == slots
            table[s] = True
            wrapped += w or s < slots - 3
        assert wrapped >= 17 and sum(1 for s in table if s < slots - 3) >= 17, bits
    pts = E.hash_cluster()
    by = cells_with_indices(pts)
    assert len(pts) == 160 and all(by[tuple(c)] == list(range(i, 160, 20)) for i, c in enumerate(cells.tolist()))


def test_the_lattices_tell_the_cell_rules_apart():
    """A case can tell floor(q / res) from floor(q * (1 / res)) only where the two differ.  They do at 0.7 and at 0.1.  At 0.3
    they never do: 1 / 0.3 rounds to a double whose relative error is 2e-18, fifty times below half an ulp, and an
    exhaustive search over every face of the key range and the four doubles on either side of it finds no point where the
    two floors part.  So 0.3 stays for flooring against truncation and for the faces whose float product falls into the
    cell below, and 0.1 joins 0.7 as the second resolution at which the reciprocal rule would show."""
    differ = {}
    for res in E.LATTICE_RES:
        pts, inner = E.lattice(res)
        q = pts[inner]
        r = np.float64(res)
        by_div, by_mul = np.floor(q / r), np.floor(q * (np.float64(1.0) / r))
        differ[res] = int((by_div != by_mul).any(axis=1).sum())
        neg = q < 0
        assert ((by_div != np.trunc(q / r)) & neg).any(axis=1).sum() > 100     # negative points that floor, not truncate
        assert (np.signbit(q).all(axis=1) & (q == 0).all(axis=1)).sum() == 1   # the negative zeros
        # the guard: the restatement admits exactly the two inner ones
        g = pts[~inner]
        f = np.floor(g[:, 0] / r)
        assert list(f) == [E.KEY_LIMIT, -E.KEY_LIMIT, E.KEY_LIMIT + 1, -(E.KEY_LIMIT + 1)]
        m = UR.build(np.zeros((0, 3)), 1024, res)
        info = UR.update(m, pts, EYE)
        assert info[3] == len(pts) - 2 and info[2] == 0
        assert {int(NR.cell_key(np.array([s * E.KEY_LIMIT, 0, 0]))) for s in (1, -1)} <= {int(k) for k in m["keys"]}
        # a map BUILD takes the inner rows only
        assert np.abs(E.cell_index(q, res)).max() < E.KEY_LIMIT - 1
    print("points where floor(q / res) != floor(q * (1 / res)):", differ)
    assert differ[0.7] >= 1 and differ[0.1] >= 1 and differ[1.0] == 0 and differ[0.3] == 0
    # at 0.3 the float product of some faces lies below the face: the point belongs to the cell below its lattice index
    x = np.arange(-E.LATTICE_RUN, E.LATTICE_RUN + 1).astype(np.float64)
    assert (np.floor((x * np.float64(0.3)) / np.float64(0.3)) != x).sum() >= 4


def test_forgetting_inputs_sit_on_the_boundary():
    stored, batches = E.forgetting()
    m = UR.build(stored, 4)
    assert list(m["count"]) == [9, 10, 11, 100] == list(E.FORGET_STORED) and E.FORGET_MAX == 10
    for b, pts in batches.items():
        by = cells_with_indices(pts)
        assert len(by) == 4 and all(len(by[(i, 0, 0)]) == b for i in range(4))
    assert 70 in batches and 70 > 11                                           # a batch larger than the stored count
    for mcp, forgets in ((0, 0), (1, 0), (2, 4), (10, 2)):                     # cells with a stored n above the cap
        assert int((m["count"] > mcp).sum()) * (mcp >= 2) == forgets


# ---- the restatement at the new shapes -------------------------------------------------------------------------------------
def by_key(m):
    o = np.argsort(m["keys"], kind="stable")
    return m["keys"][o], m["count"][o], m["mean"][o], m["S"][o]


def long_double_moments(points, keys):
    """two-pass mean and S per cell in np.longdouble over all the points, cells in the order of ``keys``"""
    pk = NR.cell_key(E.cell_index(points))
    mean, S = np.zeros((len(keys), 3)), np.zeros((len(keys), 6))
    for c, key in enumerate(keys):
        x = points[pk == key].astype(np.longdouble)
        mu = x.sum(axis=0) / np.longdouble(len(x))
        d = x - mu
        mean[c] = mu.astype(np.float64)
        S[c] = [float((d[:, i] * d[:, j]).sum()) for i in range(3) for j in range(i, 3)]
    return mean, S


def check_against_long_double(batches, what):
    """Merged mean and S after the batches (the last one under max_cell_points = 0, stated) against the two-pass long-double
    moments of the union.  Tolerance: the project's rule (test_merge_route_against_rebuild_route): 100 x the spread between
    the forward and the reversed point order, relative to the largest coordinate (means) and to the norm of the cell's S,
    floored at TOL_FLOOR."""
    def run(rev):
        m = UR.build(np.zeros((0, 3)), 16)
        for i, b in enumerate(batches):
            kw = dict(max_cell_points=0) if i == len(batches) - 1 else {}
            UR.update(m, b[::-1] if rev else b, EYE, **kw)
        return by_key(m)
    kf, cf, mean_f, S_f = run(False)
    kr, cr, mean_r, S_r = run(True)
    union = np.concatenate(batches)
    assert (kf == kr).all() and (cf == cr).all() and cf.sum() == len(union)
    mean_l, S_l = long_double_moments(union, kf)
    scale = np.abs(union).max()
    nrm = np.sqrt((S_l ** 2).sum(axis=1))
    many = cf >= 2                                                             # S of a single point is zero on every route
    spread_mean = float(np.abs(mean_f - mean_r).max() / scale)
    spread_S = float((np.sqrt(((S_f - S_r)[many] ** 2).sum(axis=1)) / nrm[many]).max())
    tol_mean, tol_S = max(100.0 * spread_mean, TOL_FLOOR), max(100.0 * spread_S, TOL_FLOOR)
    got_mean = float(np.abs(mean_f - mean_l).max() / scale)
    got_S = float((np.sqrt(((S_f - S_l)[many] ** 2).sum(axis=1)) / nrm[many]).max())
    print(f"{what}: counts {cf.tolist()}")
    print(f"{what}: mean forward/reversed spread {spread_mean:.3e} -> tolerance {tol_mean:.3e}; merge vs long double {got_mean:.3e}")
    print(f"{what}: S    forward/reversed spread {spread_S:.3e} -> tolerance {tol_S:.3e}; merge vs long double {got_S:.3e}")
    assert got_mean <= tol_mean and got_S <= tol_S
    assert (S_f[~many] == 0).all()


def test_the_restatement_matches_long_double_on_dense_cells():
    check_against_long_double([E.dense_cells(1), E.dense_cells(2), E.dense_cells(3)], "dense cells")


def test_the_restatement_matches_long_double_on_one_key():
    single, two = E.one_key(5000)
    check_against_long_double([single, E.one_key(5000, seed=51)[0]], "one key")
    check_against_long_double([two], "two keys")
