"""Inputs of the key-limit and block-hash tests of the voxel front-end (tests/test_key_limits_cpu.py,
tests/test_hip_key_limits.py): scenes whose rows sit at the ends of every field of the block key
[b:5 | t+16:5 | BZ:18 | BY:18 | BX:18], and scenes whose blocks collide in the block hash by construction.  Points sit at
voxel centres (train_edge_inputs.rows_at); each case states its rows per level, the CPU test asserts them with the oracle.
No GPU, no native library.

The colliding blocks: the block hash is linear in the block coordinates, and the block offset V = (-200, 185, 126) changes
it by -67 (mod 2^32).  A slot is the top bits of the hash, so in a table of 2048 slots (2^21 hash values per slot) the K
blocks at A + k m V, k < K, have their homes in one slot or two neighbouring ones as long as 67 m K < 2^21: a chain of K
slots.  A chain voxel has x = 31, y = 0, z = 31 (mod 32): at every level 0..3 it lies in the +x, -y and +z face of its
block, and its three neighbour voxels (x + 1, y - 1, z + 1) lie in the adjacent blocks -- three more chains, and every
adjacency hit of the 3x3x3x3 map lies up to K slots behind the first slot probed."""
import functools

import numpy as np

from tests.train_edge_inputs import BATCH_MAX, COORD_MAX, COORD_MIN, T_MAX, T_MIN, grid, rows_at

V_BLOCKS = (-200, 185, 126)         # block offset whose hash difference is HASH_STEP
HASH_STEP = -67
SLOTS = 2048                        # slots per level of a context reserved for up to 1024 rows


def _rows(ijk, t, b, seed):
    r = rows_at(ijk, t, seed)
    r[:, 0] = b
    return r


# ---- the ends of the coordinate fields ---------------------------------------------------------------------------------------
INSET = 80                          # five cells of the coarsest level, more than a level-4 block (64 voxels)


def corner_cubes():
    """origins of the 3x3x3 cubes of `corners`: both corners of the range, and each of them with one axis at its limit"""
    hi, lo = COORD_MAX - 2, COORD_MIN
    out = [((hi, hi, hi), (0, 1)), ((lo, lo, lo), (0, 1))]
    for a in range(3):
        out.append((tuple(hi if i == a else hi - INSET for i in range(3)), (1,)))
        out.append((tuple(lo if i == a else lo + INSET for i in range(3)), (1,)))
    return out


def _corners():
    parts = []
    for n, (origin, ts) in enumerate(corner_cubes()):
        for t in ts:
            parts.append(_rows(grid(3, 3, 3, origin=origin), t, 0, seed=100 + 2 * n + t))
    return np.concatenate(parts)


def bad_rows():
    """one row one step outside each limit: x, y, z at + and -, t = 16, t = -17, b = 31"""
    bad = _rows([(5, 5, 5)] * 9, 1, 0, seed=140)
    for a in range(3):
        bad[2 * a, 1 + a] = rows_at([(COORD_MAX + 1,) * 3], 1, 0)[0, 1]
        bad[2 * a + 1, 1 + a] = rows_at([(COORD_MIN - 1,) * 3], 1, 0)[0, 1]
    bad[6, 4] = T_MAX + 1
    bad[7, 4] = T_MIN - 1
    bad[8, 0] = BATCH_MAX + 1
    return bad


BAD_AT = tuple(range(0, 270, 30))   # where the nine bad rows stand among the 270 rows of `corners`


def _limits_with_bad_rows():
    good, bad = _corners(), bad_rows()
    assert len(good) == 270
    parts, last = [], 0
    for i, at in enumerate(BAD_AT):
        parts += [good[last:at], bad[i:i + 1]]
        last = at
    return np.concatenate(parts + [good[last:]])


# ---- the ends of the time and batch fields -------------------------------------------------------------------------------------
def _time_batch_carry():
    patch = grid(2, 2, 2, origin=(8, 8, 8))
    where = [(0, 15), (1, -16), (29, 15), (30, -16), (30, 15), (0, 14), (1, -15)]
    return np.concatenate([_rows(patch, t, b, seed=200 + i) for i, (b, t) in enumerate(where)])


def _all_time_indices():
    patch = grid(3, 3, 2, origin=(-2, 6, 3))
    return np.concatenate([_rows(patch, t, 0, seed=300 + t) for t in range(T_MIN, T_MAX + 1)])


# ---- colliding blocks ------------------------------------------------------------------------------------------------------------
FAMILIES = ((0, 0, 0), (1, 0, 0), (0, -1, 0), (0, 0, 1))        # the chain voxel and its +x, -y, +z neighbours


def chain_voxels(K, m, anchor):
    """[4 K, 3] voxels: family-major, k ascending; `anchor` = (31, 0, 31) mod 32"""
    assert tuple(c % 32 for c in anchor) == (31, 0, 31)
    k = np.arange(K)[:, None]
    main = np.asarray(anchor) + k * (4 * m * np.asarray(V_BLOCKS))
    return np.concatenate([main + np.asarray(f) for f in FAMILIES])


def chain(K, m, anchor, reverse=False):
    rows = _rows(chain_voxels(K, m, anchor), 1, 0, seed=400 + K + m)
    return rows[::-1].copy() if reverse else rows


# anchors: A_160 in the middle of the range; A_40 at its edge (the chain of 40 steps of 8 blocks spans 95 % of every axis);
# A_WRAP / A_WRAP_X found on the CPU (tests/test_key_limits_cpu.py re-derives what they were chosen for): the level-0 homes
# of the main chain (A_WRAP), or of its +x neighbours and of no other family (A_WRAP_X), lie in the last 8 of 2048 slots
A_160 = (64031, -60000 + 32, -40001)
A_40 = (COORD_MAX - 32, COORD_MIN + 32, COORD_MIN + 31)
A_WRAP = (70111, -59968, -40001)
A_WRAP_X = (71615, -59968, -40001)

# name -> (builder, rows at levels 0..4)
CASES = {
    "corners": (_corners, (270, 80, 10, 10, 10)),
    "time_batch_carry": (_time_batch_carry, (56, 7, 7, 7, 7)),
    "all_time_indices": (_all_time_indices, (576, 256, 256, 128, 64)),
    "limits_with_bad_rows": (_limits_with_bad_rows, (270, 80, 10, 10, 10)),
    "chain160": (lambda: chain(160, 1, A_160), (640, 640, 640, 560, 440)),
    "chain160_rev": (lambda: chain(160, 1, A_160, reverse=True), (640, 640, 640, 560, 440)),
    "chain40x8": (lambda: chain(40, 8, A_40), (160,) * 5),
    "chain40x8_rev": (lambda: chain(40, 8, A_40, reverse=True), (160,) * 5),
    "chain_wrap": (lambda: chain(160, 1, A_WRAP), (640, 640, 640, 560, 440)),
    "chain_wrap_rev": (lambda: chain(160, 1, A_WRAP, reverse=True), (640, 640, 640, 560, 440)),
    "chain_wrap_x": (lambda: chain(160, 1, A_WRAP_X), (640, 640, 640, 560, 440)),
    "chain_wrap_x_rev": (lambda: chain(160, 1, A_WRAP_X, reverse=True), (640, 640, 640, 560, 440)),
}
# case -> (K, block step m, anchor, levels at which the four families are chains of K blocks)
CHAINS = {
    "chain160": (160, 1, A_160, (0,)), "chain160_rev": (160, 1, A_160, (0,)),
    "chain40x8": (40, 8, A_40, (0, 1, 2, 3)), "chain40x8_rev": (40, 8, A_40, (0, 1, 2, 3)),
    "chain_wrap": (160, 1, A_WRAP, (0,)), "chain_wrap_rev": (160, 1, A_WRAP, (0,)),
    "chain_wrap_x": (160, 1, A_WRAP_X, (0,)), "chain_wrap_x_rev": (160, 1, A_WRAP_X, (0,)),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """[N, 6] float32 batch of a case (read-only)"""
    batch = CASES[name][0]()
    batch.setflags(write=False)
    return batch


@functools.lru_cache(maxsize=None)
def oracle_structure(name):
    """the oracle's coordinate manager of the in-range rows of a case, all five levels, and the inverse map"""
    from oracle import sps_oracle as O
    from tests.train_edge_inputs import VS, in_range
    batch = case(name)
    vox, inv = O.unique_first(O.quantize(batch[in_range(batch), :5], VS))
    cm = O.CoordinateManager(vox)
    cm.ensure_stride(16)
    return cm, inv
