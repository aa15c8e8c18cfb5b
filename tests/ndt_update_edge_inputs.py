"""Hand-built inputs that drive the online NDT map's update (sps_amd/csrc/ndt_update_kernels.inc.h) into the branches the
realistic scans leave to chance: more than 64 points of one batch in one cell, cell lists that straddle the 2048-index groups
of the ordering bitmap, the full 65 536-point limit, more touched cells than workgroups, a capacity cut beyond the first
1024 points, thousands of points on one new key, hash probes that wrap past the end of the table, cell faces under
floor(q / res), and the forgetting branch at its boundary.  No GPU, no native library: numpy only.

Every builder returns float64 points in the map frame (the poses of the tests are the identity, so q = p exactly) at
resolution 1 unless it says otherwise.  A point of cell c sits at c + 0.05 + 0.9 * rng.random, well inside the cell."""
import numpy as np

KEY_LIMIT = 1048575
MAX_POINTS = 65536                                     # SPS_NDT_UPDATE_MAX_POINTS

DENSE_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 300)  # around the 64-point chunks of k_ndt_upd_stats: 879 points
BITMAP_N = 4100
BITMAP_COUNTS = (4064, 4065, 4095, 4096, 4097, 4100)   # device counts: n % 32 in {0, 1, 31}, both sides of 4096
BITMAP_STRADDLE = (0, 2047, 2048, 4095, 4096, 4099)    # one cell across both 2048-index group borders
BITMAP_WORDS = (31, 32, 63, 64, 95)                    # one cell on both sides of three word borders
BITMAP_RUN = tuple(i for i in range(2040, 2056) if i not in (2047, 2048))   # a run over the first group border
BITMAP_LATE = (4097, 4098)                             # a cell whose lead is 4097: w0 = 128, the bitmap's last word
BITMAP_SPECIAL_CELLS = ((0, 0, 5), (1, 0, 5), (2, 0, 5), (3, 0, 5))
BITMAP_FILLERS = 200
FULL_CELLS = 512
FULL_EXTRA = (0, 2048, 14336, 32768, 63488, 65535)     # the first and last index and four multiples of 2048
FULL_EXTRA_CELL = (20, 20, 20)
FOUNDER_N, FOUNDER_REPEATS = 3000, 500
FOUNDER_CUTS = (1023, 1024, 1025, 2048)                # founders admitted: the last one has global rank 1022, 1023, 1024, 2047
FORGET_MAX = 10
FORGET_STORED = (FORGET_MAX - 1, FORGET_MAX, FORGET_MAX + 1, 10 * FORGET_MAX)
FORGET_BATCHES = (1, 70)
LATTICE_RES = (0.3, 0.7, 1.0, 0.1)                     # 0.1: see test_the_lattices_tell_the_cell_rules_apart
LATTICE_RUN = 64


def in_cells(cells, rng):
    """one point inside each of the cells [n, 3] (integer triples, resolution 1)"""
    cells = np.asarray(cells, dtype=np.float64).reshape(-1, 3)
    return cells + 0.05 + 0.9 * rng.random((len(cells), 3))


def cell_index(xyz, resolution=1.0):
    return np.floor(np.asarray(xyz, dtype=np.float64) / float(resolution)).astype(np.int64)


def grid_cells(k, width):
    """k distinct cells (i % width, i // width, 0)"""
    i = np.arange(k)
    return np.stack([i % width, i // width, np.zeros(k, dtype=np.int64)], axis=1)


# ---- the 64-point chunks ---------------------------------------------------------------------------------------------------
def dense_cells(seed):
    """Cells (i, 0, 0) with DENSE_COUNTS[i] points each, the indices randomly permuted: every cell's list spans the whole
    index range.  At 2 m and 4 m the cells merge into cells of several hundred points."""
    rng = np.random.default_rng(seed)
    cells = np.concatenate([np.tile([[i, 0, 0]], (c, 1)) for i, c in enumerate(DENSE_COUNTS)])
    return in_cells(cells, rng)[rng.permutation(len(cells))]


# ---- the ordering bitmap ---------------------------------------------------------------------------------------------------
def bitmap_cells():
    """the cell of every one of the BITMAP_N indices"""
    rng = np.random.default_rng(41)
    cells = grid_cells(BITMAP_FILLERS, 20)[rng.integers(0, BITMAP_FILLERS, BITMAP_N)]
    for idx, c in zip((BITMAP_STRADDLE, BITMAP_WORDS, BITMAP_RUN, BITMAP_LATE), BITMAP_SPECIAL_CELLS):
        cells[list(idx)] = c
    return cells


def bitmap_groups():
    """BITMAP_N points: the four special cells hold exactly the indices named above, about 200 filler cells the rest"""
    return in_cells(bitmap_cells(), np.random.default_rng(42))


def full_limit():
    """MAX_POINTS points over the 512 cells of [0, 8)^3, and one more cell that holds exactly the indices FULL_EXTRA"""
    rng = np.random.default_rng(43)
    c = rng.integers(0, FULL_CELLS, MAX_POINTS)
    cells = np.stack([c % 8, (c // 8) % 8, c // 64], axis=1)
    cells[list(FULL_EXTRA)] = FULL_EXTRA_CELL
    return in_cells(cells, rng)


# ---- the grid-stride loop over the touched cells ---------------------------------------------------------------------------
def many_cells(k):
    """k points in k distinct cells.  Founded in this order the cell ids follow the indices; the same points reversed
    (``many_cells(k)[::-1]``) then have their leads in the reverse of the id order."""
    return in_cells(grid_cells(k, 20), np.random.default_rng(44))


# ---- the founder scan ------------------------------------------------------------------------------------------------------
def founder_cells():
    """the cell of every one of the FOUNDER_N indices: 2 500 new cells in index order and, interleaved from index 8 on, 500
    second points of keys met earlier (early keys, which every capacity of the tests admits, and late ones, which it
    drops)"""
    rng = np.random.default_rng(45)
    repeat = np.zeros(FOUNDER_N, dtype=bool)
    repeat[8 + rng.choice(FOUNDER_N - 8, FOUNDER_REPEATS, replace=False)] = True
    new = grid_cells(FOUNDER_N - FOUNDER_REPEATS, 50)
    cells = np.zeros((FOUNDER_N, 3), dtype=np.int64)
    founded = 0
    for i in range(FOUNDER_N):
        if repeat[i]:
            cells[i] = new[rng.integers(0, founded)]
        else:
            cells[i] = new[founded]
            founded += 1
    return cells


def founder_run():
    return in_cells(founder_cells(), np.random.default_rng(46))


def founder_start_map():
    """five cells away from the run's (z = 3), eight points each: a map that starts with 5 cells"""
    cells = np.repeat(np.array([[0, 0, 3], [1, 0, 3], [2, 0, 3], [3, 0, 3], [4, 0, 3]]), 8, axis=0)
    return in_cells(cells, np.random.default_rng(47))


# ---- one key under contention ----------------------------------------------------------------------------------------------
def one_key(n, seed=48):
    """(n points in one cell, n points alternating between two cells)"""
    rng = np.random.default_rng(seed)
    single = in_cells(np.tile([[2, 3, 4]], (n, 1)), rng)
    two = np.where((np.arange(n) % 2 == 0)[:, None], [[0, 0, 0]], [[7, 0, 0]])
    return single, in_cells(two, rng)


# ---- probing that wraps ----------------------------------------------------------------------------------------------------
def hash64(k):
    """keys_hash.inc.h's hash64 on numpy uint64 (the multiplications wrap, as the device's do)"""
    k = np.asarray(k, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xff51afd7ed558ccd)
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xc4ceb9fe1a85ec53)
        k ^= k >> np.uint64(33)
    return (k & np.uint64(0xFFFFFFFF)).astype(np.uint64)


def radius_key(c):
    c = np.asarray(c, dtype=np.int64)
    return (((c[..., 2] + (1 << 20)) << 42) | ((c[..., 1] + (1 << 20)) << 21) | (c[..., 0] + (1 << 20))).astype(np.uint64)


def hash_cluster_cells():
    """The cells of [-48, 48)^3 whose hash has its low 17 bits at 2^17 - 3 or above: in every power-of-two table of up to
    2^17 slots they home on the last three slots, so all but three of them are stored past the wrap."""
    r = np.arange(-48, 48)
    c = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    low = hash64(radius_key(c)) & np.uint64((1 << 17) - 1)
    return c[low >= np.uint64((1 << 17) - 3)]


def hash_cluster(per_cell=8):
    """eight points in each cluster cell, interleaved (point i lies in cell i % cells)"""
    cells = hash_cluster_cells()
    return in_cells(np.tile(cells, (per_cell, 1)), np.random.default_rng(49))


# ---- cell faces ------------------------------------------------------------------------------------------------------------
def lattice(res):
    """(points, inner): the lattice (i, j, k) * res for i, j, k in -3 .. 3 as float products (points on cell faces), each
    followed by a second point half a cell further in the same cell; a point of negative zeros (cell 0); the faces
    i * res for i in -64 .. 64 along x, each with its two neighbouring doubles (among -3 .. 3 the rules floor(q / res) and
    floor(q * (1 / res)) part only at neighbours of faces, and only for some resolutions: tests/test_ndt_update_edges_cpu.py);
    then the guard along x: the last admitted cells +-KEY_LIMIT and the first refused ones +-(KEY_LIMIT + 1).  ``inner`` marks the rows before the guard: the guard's cells are beyond what a map BUILD takes
    (radius_grid_cells asserts |cell| < KEY_LIMIT), so a built map gets points[inner] and only the update sees the rest."""
    res = np.float64(res)
    r = np.arange(-3, 4).astype(np.float64)
    ijk = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    face = ijk * res
    body = np.stack([face, face + res * 0.5], axis=1).reshape(-1, 3)
    zero = np.array([[-0.0, -0.0, -0.0]])
    half = res * 0.5
    x = np.arange(-LATTICE_RUN, LATTICE_RUN + 1).astype(np.float64) * res
    x = np.stack([np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)], axis=1).reshape(-1)
    run = np.stack([x, np.full(len(x), half), np.full(len(x), half)], axis=1)
    guard = np.array([[s * k * res + half, half, half] for k in (KEY_LIMIT, KEY_LIMIT + 1) for s in (1.0, -1.0)])
    pts = np.concatenate([body, zero, run, guard])
    inner = np.arange(len(pts)) < len(pts) - len(guard)
    return pts, inner


# ---- forgetting ------------------------------------------------------------------------------------------------------------
def forgetting():
    """(stored, batches): the stored map's points, cells (i, 0, 0) with FORGET_STORED[i] points, and per batch size of
    FORGET_BATCHES that many points into each of the four cells, interleaved"""
    rng = np.random.default_rng(50)
    stored = in_cells(np.concatenate([np.tile([[i, 0, 0]], (c, 1)) for i, c in enumerate(FORGET_STORED)]), rng)
    four = np.array([[i, 0, 0] for i in range(len(FORGET_STORED))])
    return stored, {b: in_cells(np.tile(four, (b, 1)), rng) for b in FORGET_BATCHES}
