"""Inputs of the training-backward edge tests (tests/test_train_edges_cpu.py, tests/test_hip_train_edges.py): scenes
built from explicit voxel lattices, so the number of rows at every level is CHOSEN (each case states its level counts,
the CPU test asserts them with the oracle's CoordinateManager); cotangents other than the MSE's; the capacities that move
the launch plan of the weight gradients; the tolerance, measured from the float32 / float64 runs of the autograd oracle;
and three mutants of the oracle's backward that the tolerance must catch.  No GPU, no native library.

A point sits at the centre of its voxel: (i + 0.5) * 0.1 in float32, whose float32 quotient by 0.1 floors to i."""
import contextlib
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import sps_oracle as O
from oracle import train_oracle as T
from sps_amd import synthetic

VS = 0.1
PARAMS_SEED = 0

# the ranges of the voxel key (include/sps_hip.h: SPS_COORD_MIN / MAX, SPS_T_MIN / MAX, SPS_BATCH_MAX): a row outside them
# gets inverse -1 and a NaN score, and the forward sets the sticky out-of-range flag (tests/test_hip_parity.py)
COORD_MIN, COORD_MAX, T_MIN, T_MAX, BATCH_MAX = -131072, 131071, -16, 15, 30


# ---- scenes ----------------------------------------------------------------------------------------------------------------
def rows_at(ijk, t, seed, frac=None):
    """[n, 6] float32 rows (b, x, y, z, t, label): one point per integer voxel `ijk`, at the voxel's centre (or at the
    in-voxel position `frac` in (0, 1)^3); labels uniform in (0, 1) from `seed`"""
    ijk = np.asarray(ijk, dtype=np.float64).reshape(-1, 3)
    f = 0.5 if frac is None else np.asarray(frac, dtype=np.float64)
    out = np.zeros((len(ijk), 6), dtype=np.float32)
    out[:, 1:4] = ((ijk + f) * VS).astype(np.float32)
    out[:, 4] = np.broadcast_to(np.asarray(t, dtype=np.float32), (len(ijk),))
    out[:, 5] = np.random.default_rng(seed).uniform(0.0, 1.0, len(ijk)).astype(np.float32)
    return out


def grid(nx, ny, nz, origin=(0, 0, 0), step=1):
    """integer voxels of an nx x ny x nz lattice, x fastest"""
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1) * step + np.asarray(origin)


def with_duplicates(rows, every, seed):
    """`rows` followed by a second point (another in-voxel position, another label) in every `every`-th voxel"""
    rng = np.random.default_rng(seed)
    dup = rows[::every].copy()
    dup[:, 1:4] += ((rng.uniform(-0.3, 0.3, (len(dup), 3))) * VS).astype(np.float32)
    dup[:, 5] = rng.uniform(0.0, 1.0, len(dup)).astype(np.float32)
    return np.concatenate([rows, dup])


FAR = (32, 0, 0)            # a voxel in another cell of the coarsest level (16 voxels wide): a second coarsest row
def far_clusters():
    """10 voxels in four far cells of the coarsest level (none adjacent to another at any level): lines of 1, 2, 3 and 4
    voxels along x, y, z and x.  Four coarse rows with four different neighbourhoods: single far voxels would all carry
    the same features, and a BatchNorm over rows that take two distinct values is a constant of its input (as at the two
    coarsest rows of `min`) -- everything upstream of it then has a gradient of rounding noise, in the oracle too, and
    the float32 / float64 yardstick measures nothing."""
    return np.array([(32, 0, 0), (0, 32, 0), (0, 33, 0), (32, 32, 5), (32, 32, 6), (32, 32, 7),
                     (1, 0, 64), (2, 0, 64), (3, 0, 64), (4, 0, 64)])


def tile_edge_voxels(n):
    """n level-0 voxels: the first n - 10 of a 4 x 4 x Z box (x fastest) and far_clusters()"""
    return np.concatenate([grid(4, 4, (n + 5) // 16 + 1)[: n - 10], far_clusters()])


def _min():
    # 16 voxels of a 2 x 2 x 4 column (two level-1 rows, one row from level 2 up) and FAR: one full 16-row tile plus one row
    return with_duplicates(rows_at(np.concatenate([grid(2, 2, 4), [FAR]]), 1, seed=11), 5, seed=12)


def _tile_edges(n):
    return with_duplicates(rows_at(tile_edge_voxels(n), 1, seed=20 + n), 7, seed=21 + n)


def _dust():
    # isolated voxels 40 apart (no spatial neighbour at any level: the coarsest cells are 16 wide), every third one also in
    # time slice 0 (pairs along t only), and one run of three x-adjacent voxels: a few spatial offsets have a pair, in one tile
    sites = grid(5, 4, 3, step=40)
    a = rows_at(sites, 1, seed=31)
    b = rows_at(sites[::3], 0, seed=32)
    c = rows_at([(1, 0, 0), (2, 0, 0), (11, 6, 1)], 1, seed=33)
    return with_duplicates(np.concatenate([a, b, c]), 9, seed=34)


def _brick():
    # a full 6 x 6 x 6 block in time slice 1 (all 27 spatial offsets for its interior) over a 6 x 6 x 3 slab in time slice 0
    # (offsets along t); the block straddles the 8-voxel cell faces, so level 3 has 8 cells per time slice
    a = rows_at(grid(6, 6, 6, origin=(6, 6, 6)), 1, seed=41)
    b = rows_at(grid(6, 6, 3, origin=(6, 6, 6)), 0, seed=42)
    return with_duplicates(np.concatenate([a, b]), 11, seed=43)


def _dupes():
    # 40 points in the voxel (2, 2, 0), single points in the other 49 voxels of a 5 x 5 x 2 patch and in far_clusters()
    rng = np.random.default_rng(51)
    many = rows_at(np.tile([(2, 2, 0)], (40, 1)), 1, seed=52, frac=rng.uniform(0.1, 0.9, (40, 3)))
    rest = [v for v in grid(5, 5, 2).tolist() if v != [2, 2, 0]] + far_clusters().tolist()
    rows = np.concatenate([rows_at(rest, 1, seed=53), many])
    return rows[np.random.default_rng(54).permutation(len(rows))]


def _off_range():
    # a 4 x 4 x 4 block, FAR and a second time slice, with rows outside the key range at the start, inside and at the end:
    # x and y beyond +-131072 voxels, t = 16 and t = -17, batch index 31
    good = with_duplicates(np.concatenate([rows_at(np.concatenate([grid(4, 4, 4), [FAR]]), 1, seed=61),
                                           rows_at(grid(4, 4, 1), 0, seed=62)]), 6, seed=63)
    bad = rows_at([(0, 0, 0)] * 6, 0, seed=64)
    bad[0, 1] = 2.0e4                       # 200 000 voxels
    bad[1, 2] = -1.4e4                      # -140 000 voxels
    bad[2, 4] = 16
    bad[3, 4] = -17
    bad[4, 0] = 31
    bad[5, 3] = np.float32(COORD_MAX + 1) * np.float32(VS) * np.float32(1.001)
    k = len(good) // 2
    return np.concatenate([bad[:2], good[:k], bad[2:4], good[k:], bad[4:]])


def _big():
    return synthetic.small_scene(seed=3, n_scan=3000)


def _key_limit(name, every, seed):
    # a scene of tests/key_limit_inputs.py (which imports this module: hence here): `corners` has rows at both ends of every
    # coordinate field of the voxel key, `chain40x8` blocks that collide in the block hash at levels 0 to 3
    from tests import key_limit_inputs
    return with_duplicates(key_limit_inputs.case(name).copy(), every, seed)


# name -> (builder, rows at levels 0..4)
CASES = {
    "min": (_min, (17, 3, 2, 2, 2)),
    "tile16": (lambda: _tile_edges(16), (16, 9, 6, 5, 5)),
    "tile17": (lambda: _tile_edges(17), (17, 9, 6, 5, 5)),
    "tile64": (lambda: _tile_edges(64), (64, 15, 6, 5, 5)),
    "tile65": (lambda: _tile_edges(65), (65, 15, 6, 5, 5)),
    "tile257": (lambda: _tile_edges(257), (257, 39, 9, 6, 5)),
    "dust": (_dust, (83, 82, 81, 81, 80)),
    "brick": (_brick, (324, 45, 16, 16, 2)),
    "dupes": (_dupes, (60, 16, 9, 5, 5)),
    "off_range": (_off_range, (81, 13, 3, 3, 3)),
    "corners": (lambda: _key_limit("corners", 9, seed=71), (270, 80, 10, 10, 10)),
    "chain40x8": (lambda: _key_limit("chain40x8", 7, seed=72), (160, 160, 160, 160, 160)),
}
TILE_EDGES = ("tile16", "tile17", "tile64", "tile65", "tile257")


_SCORES64 = {}          # case -> the float64 oracle's train-mode scores [N] (NaN on out-of-range rows)


@functools.lru_cache(maxsize=None)
def case(name):
    """[N, 6] float32 batch of a case (read-only).  The labels of the lattice cases lie within 0.02 of the float64 oracle's
    train-mode scores: the MSE cotangent is then that of a nearly converged step, 1e-3 and below, the magnitude at which a
    coarse dlogit shows (with labels uniform in (0, 1) the 17-row scenes give dlogit ~ 1e-2 and hide it)."""
    if name == "big":
        batch = _big()
    else:
        batch = CASES[name][0]()
        ok = in_range(batch)
        s = np.full(len(batch), np.nan)
        with one_thread():
            _, s[ok], _, _ = T.train_step(params(), batch[ok], VS, dscores=np.zeros(int(ok.sum())))
        batch[ok, 5] = (s[ok] + np.random.default_rng(len(batch)).uniform(-0.02, 0.02, int(ok.sum()))).astype(np.float32)
        _SCORES64[name] = s
    batch.setflags(write=False)
    return batch


def in_range(batch):
    """rows inside the voxel-key range: the others have inverse -1 on the device and do not exist for the oracle"""
    q = O.quantize(batch[:, :5], VS).astype(np.int64)            # (every coordinate here is far inside int32)
    ok = (q[:, 0] >= 0) & (q[:, 0] <= BATCH_MAX) & (q[:, 4] >= T_MIN) & (q[:, 4] <= T_MAX)
    return ok & np.all((q[:, 1:4] >= COORD_MIN) & (q[:, 1:4] <= COORD_MAX), axis=1)


def level_counts(batch):
    """rows per level by the oracle's coordinate manager, and the inverse map of the in-range rows"""
    vox, inv = O.unique_first(O.quantize(batch[in_range(batch), :5], VS))
    cm = O.CoordinateManager(vox)
    cm.ensure_stride(16)
    return tuple(len(cm.coords[1 << l]) for l in range(5)), inv


@functools.lru_cache(maxsize=None)
def params():
    return O.random_params(seed=PARAMS_SEED)


# ---- cotangents ------------------------------------------------------------------------------------------------------------
# cot(name, batch, inv) -> float32 [N]; inv [N] is the point -> level-0 row map (-1 on out-of-range rows) of whoever runs the
# backward: the row ORDER is the implementation's, so "the last row" is too.  A cotangent is a fixed vector: the oracle in
# both precisions and the device all receive the same numbers.
def cot_mse(name, batch, inv):
    """d MSE / d scores of common_step, 2 (s - y) / count on the rows with t == 1 and 0 elsewhere, at the float64 oracle's
    scores s (at each implementation's own scores, the float32 / float64 yardstick would measure the scores' difference
    times 2 / count against a cotangent of 0.04 / count, not the backward)"""
    scan = batch[:, 4] == 1
    g = np.zeros(len(batch), dtype=np.float64)
    g[scan] = 2.0 * (_SCORES64[name][scan] - batch[scan, 5].astype(np.float64)) / int(scan.sum())
    return g.astype(np.float32)


def cot_random(name, batch, inv):
    return np.random.default_rng(7 + len(batch)).standard_normal(len(batch)).astype(np.float32)


def cot_onehot_last(name, batch, inv):
    g = np.zeros(len(batch), dtype=np.float32)
    g[np.flatnonzero(np.asarray(inv) == np.max(inv))[0]] = 1.0
    return g


def cot_off_range_only(name, batch, inv):
    g = np.zeros(len(batch), dtype=np.float32)
    bad = ~in_range(batch)
    g[bad] = np.random.default_rng(9).standard_normal(int(bad.sum())).astype(np.float32) + np.float32(3.0)
    return g


COTANGENTS = {"mse": cot_mse, "random": cot_random, "onehot_last": cot_onehot_last, "off_range_only": cot_off_range_only}

# the (case, cotangent) pairs of the GPU gradient test.  Every scene gets the MSE cotangent (small and smooth) and the
# sign-mixed unit-scale one (the out-of-range rows of off_range have t != 1: the MSE does not select their NaN scores)
PAIRS = ([(c, g) for c in CASES for g in ("mse", "random")]
         + [("min", "onehot_last"), ("tile17", "onehot_last"), ("tile65", "onehot_last"), ("dupes", "onehot_last"),
            ("off_range", "onehot_last"), ("off_range", "off_range_only")])


# ---- the launch plan of the weight gradients -------------------------------------------------------------------------------
# train_reserve (sps_amd/csrc/train_host.inc.h) derives, for every k_wgrad job, gshift (4: rows read 16 at a time, 6: 64 at a
# time) and nwg (workgroups per (offset, block); > 1: partials in the slab, summed by k_wgrad_reduce_all) from the CAPACITY:
#   tiles  = max(64, floor(prior[level] * cap) / 16),  prior = 1, 0.5, 0.2, 0.06, 0.02
#   gshift = 4 if K * zblocks * (tiles / 8) < 4096 else 6
#   groups = tiles (gshift 4) or tiles / 4 (gshift 6)
#   want   = min(1024, max(16, 16384 / (K * zblocks)));  nwg = ceil(want / 16), halved while nwg * 16 * (4 or 2) > groups
# with zblocks = ceil(C_in / (16 aw)) * ceil(C_out / (16 bw)), aw = 2 from C_in 24, bw = 2 from C_out 32, 4 from 64.
# plan(cap) below is that arithmetic; the tables are what it gives, asserted by the CPU test.
WG_LAYERS = (  # name, K, C_in, C_out, level whose rows the map lists
    ("conv1p1s2", 8, 8, 8, 1), ("block1.0.conv1", 81, 8, 8, 1), ("block1.0.conv2", 81, 8, 8, 1),
    ("conv2p2s2", 8, 8, 8, 2), ("block2.0.conv1", 81, 8, 16, 2), ("block2.0.conv2", 81, 16, 16, 2), ("block2.0.downsample.0", 1, 8, 16, 2),
    ("conv3p4s2", 8, 16, 16, 3), ("block3.0.conv1", 81, 16, 32, 3), ("block3.0.conv2", 81, 32, 32, 3), ("block3.0.downsample.0", 1, 16, 32, 3),
    ("conv4p8s2", 8, 32, 32, 4), ("block4.0.conv1", 81, 32, 64, 4), ("block4.0.conv2", 81, 64, 64, 4), ("block4.0.downsample.0", 1, 32, 64, 4),
    ("convtr4p16s2", 8, 64, 64, 4), ("block5.0.conv1", 81, 96, 64, 3), ("block5.0.conv2", 81, 64, 64, 3), ("block5.0.downsample.0", 1, 96, 64, 3),
    ("convtr5p8s2", 8, 64, 32, 3), ("block6.0.conv1", 81, 48, 32, 2), ("block6.0.conv2", 81, 32, 32, 2), ("block6.0.downsample.0", 1, 48, 32, 2),
    ("convtr6p4s2", 8, 32, 16, 2), ("block7.0.conv1", 81, 24, 16, 1), ("block7.0.conv2", 81, 16, 16, 1), ("block7.0.downsample.0", 1, 24, 16, 1),
    ("convtr7p2s2", 8, 16, 8, 1), ("block8.0.conv1", 81, 16, 8, 0), ("block8.0.conv2", 81, 8, 8, 0), ("block8.0.downsample.0", 1, 16, 8, 0),
)
LEVEL_PRIOR = (1.0, 0.5, 0.2, 0.06, 0.02)


def plan(cap):
    """name -> (gshift, nwg) of every k_wgrad job at context capacity `cap`"""
    out = {}
    for name, K, cin, cout, level in WG_LAYERS:
        aw = 2 if cin >= 24 else 1
        bw = 4 if cout >= 64 else 2 if cout >= 32 else 1
        nb = (cout + 16 * bw - 1) // (16 * bw)
        zblocks = ((cin + 16 * aw - 1) // (16 * aw)) * nb
        tiles = max(64, int(LEVEL_PRIOR[level] * float(cap)) // 16)
        gshift = 4 if K * zblocks * (tiles // 8) < 4096 else 6
        groups = tiles if gshift == 4 else tiles // 4
        want = min(1024, max(16, 16384 // (K * zblocks)))
        nwg = (want + 15) // 16
        while nwg > 1 and nwg * 16 * (4 if gshift == 4 else 2) > groups:
            nwg >>= 1
        out[name] = (gshift, nwg)
    return out


def in_words(pl):
    """the plan by layer group: {(gshift, nwg): sorted layer names}"""
    out = {}
    for name, v in pl.items():
        out.setdefault(v, []).append(name)
    return out


# the capacities of the GPU tests (a context's capacity is the row count it was reserved for, rounded up to 1024; it never
# shrinks), with plan(cap) by layer group as (gshift, nwg):
#   1024    every layer (4, 1): rows 16 at a time, one workgroup per (offset, block), no slab
#   16384   layers disagree -- level 0: block8 conv1 / conv2 (6, 6), block8 downsample (4, 16); level 1: block1 / block7
#           conv1 / conv2 (6, 3), conv1p1s2 / convtr7p2s2 / block7 downsample (4, 8); level 2: block2 / block6 conv1 / conv2
#           (4, 3), conv2p2s2 / convtr6p4s2 / their downsamples (4, 2); levels 3 and 4: (4, 1)
#   262144  level 0: block8 conv1 / conv2 (6, 13), downsample (4, 64); level 1: block1 / block7 conv1 / conv2 (6, 13),
#           conv1p1s2 / convtr7p2s2 (6, 64), block7 downsample (4, 64); level 2: block2 conv1 / conv2, block6 conv2 (6, 13),
#           block6 conv1 (6, 7), the 8- and 1-offset layers (4, 32); level 3: block3 conv1 / conv2 (6, 6), block5 conv1 (6, 5),
#           conv2 (6, 7), the others (4, 8); level 4: block4 conv1 (4, 3), conv2 (6, 1), the others (4, 4)
CAP_MIN, CAP_MIXED, CAP_WIDE = 1024, 16384, 262144
PLAN_CASES = ("min", "tile65", "brick")


# ---- the reference and the tolerance ---------------------------------------------------------------------------------------
def rel_err(got, want):
    """max |got - want| relative to the tensor's maximum (0 / 0 = 0: an all-zero tensor met exactly)"""
    d = float(np.max(np.abs(np.asarray(got, dtype=np.float64).reshape(np.shape(want)) - want)))
    m = float(np.max(np.abs(want)))
    return d / m if m > 0 else (0.0 if d == 0 else float("inf"))


@contextlib.contextmanager
def one_thread():
    """torch's CPU index_add and matmul split their sums over the threads they are given: with one thread the float32 oracle,
    and with it the yardstick, is the same on every run of a machine (and on machines whose torch picks the same BLAS
    kernels; another instruction set may group the sums differently and give another sample of float32 rounding)"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def oracle_step(batch, dscores, dtype, mutant=None):
    """The autograd oracle on the in-range rows of `batch` with the cotangent `dscores` ([N]; None: the MSE of common_step).
    -> (scores [N] float64, NaN on out-of-range rows; gradients name -> array)"""
    ok = in_range(batch)
    with mutated(mutant), one_thread():
        _, s, grads, _ = T.train_step(params(), batch[ok], VS, dtype=dtype, dscores=np.asarray(dscores)[ok])
    scores = np.full(len(batch), np.nan)
    scores[ok] = s
    return scores, grads


_REFS = {}


def reference(case_name, dscores):
    """The float64 and the float32 oracle of a (case, cotangent), computed once and shared.  -> dict(s64, g64, s32, g32,
    e32 name -> rel_err of the float32 gradient, e32_scores)"""
    key = (case_name, np.asarray(dscores, dtype=np.float32).tobytes())
    if key not in _REFS:
        batch = case(case_name)
        s64, g64 = oracle_step(batch, dscores, torch.float64)
        s32, g32 = oracle_step(batch, dscores, torch.float32)
        ok = in_range(batch)
        _REFS[key] = dict(s64=s64, g64=g64, s32=s32, g32=g32, e32={k: rel_err(g32[k], g64[k]) for k in g64},
                          e32_scores=rel_err(s32[ok], s64[ok]))
    return _REFS[key]


MARGIN, FLOOR = 16.0, 1e-6


def allowed(e32):
    """The tolerance of a tensor, relative to its maximum: 16 x the float32 oracle's own distance from the float64 one
    (at least 1e-6).  The 16 is a margin over ONE sample of float32 rounding: the device is another float32 implementation
    of the same sums with another grouping.  Measured against the reference, never against the device."""
    if isinstance(e32, dict):
        return {k: allowed(v) for k, v in e32.items()}
    return MARGIN * max(float(e32), FLOOR)


def cotangent(case_name, cot_name, inv=None):
    """the cotangent of a pair; inv: the point -> level-0 row map of the implementation under test (default: the oracle's)"""
    batch = case(case_name)
    if inv is None:
        inv = np.full(len(batch), -1, dtype=np.int64)
        inv[in_range(batch)] = level_counts(batch)[1]
    return COTANGENTS[cot_name](case_name, batch, np.asarray(inv))


ADDITIVE_CASES = ("tile65", "dupes")


def additive_parts(case_name, inv=None):
    """(g1, g2, g1 + g2) of the additivity test: the sign-mixed cotangent, and the one-hot one plus half-scale noise"""
    g1 = cotangent(case_name, "random", inv)
    noise = np.random.default_rng(77).standard_normal(len(g1)) * 0.5
    g2 = (cotangent(case_name, "onehot_last", inv) + noise).astype(np.float32)
    return g1, g2, (g1 + g2).astype(np.float32)


# ---- mutants of the oracle's backward (the forward stays intact) -----------------------------------------------------------
class _DropPair(torch.autograd.Function):
    """x @ W whose weight gradient misses the first row (one pair of the kernel map)"""

    @staticmethod
    def forward(ctx, x, W):
        ctx.save_for_backward(x, W)
        return x @ W

    @staticmethod
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        return dy @ W.t(), x[1:].t() @ dy[1:]


MUTANT_LAYER_SHAPE = (81, 16, 8)            # block8.0.conv1: the only kernel of that shape, an 81-offset layer at level 0
CENTRE = 40


def _conv_drop_pair(feats, n_out, kmap, W, transpose=False):
    if tuple(W.shape) != MUTANT_LAYER_SHAPE:
        return _CONV(feats, n_out, kmap, W, transpose)
    target = next(k for k, (i, o) in enumerate(kmap) if k != CENTRE and len(i))
    out = torch.zeros((n_out, W.shape[-1]), dtype=feats.dtype)
    for k, (i, o) in enumerate(kmap):
        if len(i):
            x = feats.index_select(0, torch.from_numpy(np.asarray(i, np.int64)))
            y = _DropPair.apply(x, W[k]) if k == target else x @ W[k]
            out = out.index_add(0, torch.from_numpy(np.asarray(o, np.int64)), y)
    return out


class _BnNminus1(torch.autograd.Function):
    """train-mode BatchNorm whose backward divides its two means by n - 1"""

    @staticmethod
    def forward(ctx, x, w, b):
        y = F.batch_norm(x, None, None, w, b, True, 0.1, O.BN_EPS)
        mean, var = x.mean(0), x.var(0, unbiased=False)
        ctx.save_for_backward((x - mean) / torch.sqrt(var + O.BN_EPS), w / torch.sqrt(var + O.BN_EPS))
        return y

    @staticmethod
    def backward(ctx, dy):
        xhat, scale = ctx.saved_tensors
        n = xhat.shape[0]
        m1, m2 = dy.sum(0) / (n - 1), (dy * xhat).sum(0) / (n - 1)
        return scale * (dy - m1 - xhat * m2), (dy * xhat).sum(0), dy.sum(0)


def _bn_nminus1(p, name, x, stats):
    stats[name] = (x.mean(0).detach(), x.var(0, unbiased=False).detach(), x.shape[0])
    return _BnNminus1.apply(x, p[name + ".bn.weight"], p[name + ".bn.bias"])


class _RoundGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return torch.round(g * 2.0 ** 20) / 2.0 ** 20


def _head_coarse_dlogit(logits, inv):
    return _HEAD(_RoundGrad.apply(logits), inv)


_CONV, _BN, _HEAD = T._conv, T._bn, T._head
MUTANTS = {"drop_pair": ("_conv", _conv_drop_pair), "bn_n_minus_1": ("_bn", _bn_nminus1), "dlogit_2^-20": ("_head", _head_coarse_dlogit)}


@contextlib.contextmanager
def mutated(name):
    """the oracle with one function of its backward replaced (None: as it is)"""
    if name is None:
        yield
        return
    attr, fn = MUTANTS[name]
    saved = getattr(T, attr)
    setattr(T, attr, fn)
    try:
        yield
    finally:
        setattr(T, attr, saved)
