"""CPU half of the key-limit and block-hash tests of the voxel front-end: the scenes of tests/key_limit_inputs.py reach what
they are named after (both ends of every key field at every level; chains of colliding blocks of the stated length in a
2048-slot table, through slot 0 where they say so), the model of tests/block_hash_reference.py reproduces the oracle's
block adjacency and 3x3x3x3 maps on every one of them, and the model with a guard dropped does not -- for the one guard
whose loss can make a pair.  No GPU, no native library.

Which guard a case catches.  The coordinate fields of the key are 18 bits wide and hold values below 2^(16 - level): + 1
at the upper limit cannot carry into the next field, and - 1 at 0 borrows from the next field but leaves 2^18 - 1 behind,
which no block has.  So without the x, y and z guards of k_link_adj the neighbour key is still the key of no block: the
guards save a probe, they make no pair (test_coordinate_guards_cannot_make_a_pair proves it for every level and limit).
A `wrap_partners` scene -- voxels (MAX, y, z) beside (MIN, y + one block, z) -- would therefore catch nothing and is not
among the cases; `corners` keeps the coordinate limits covered.  The time field is 5 bits wide and full: t = 15 plus one
carries into the batch index.  `time_batch_carry` catches the loss of that guard, and only that one."""
import functools

import numpy as np
import pytest

from tests import block_hash_reference as B
from tests import key_limit_inputs as KL
from tests import train_edge_inputs as TE


def level_coords(name, level):
    cm, _ = KL.oracle_structure(name)
    return cm.coords[1 << level]


@functools.lru_cache(maxsize=None)
def oracle_k3(name, level):
    cm, _ = KL.oracle_structure(name)
    return frozenset(B.oracle_pairs(cm.k3(1 << level)))


def block_keys(name, level):
    """distinct block keys of a level in first-occurrence order of the oracle's rows"""
    return list(dict.fromkeys(k for k, _ in B.keys_of(level_coords(name, level), level)))


# ---- the lattice vector ------------------------------------------------------------------------------------------------------
def test_the_block_offset_changes_the_hash_by_minus_67():
    assert KL.HASH_STEP == -67 and KL.V_BLOCKS == (-200, 185, 126)
    vx, vy, vz = KL.V_BLOCKS
    assert (vx * B.H_X + vy * B.H_Y + vz * B.H_Z) % (1 << 32) == (1 << 32) - 67
    for level in range(5):
        for m in (1, 2, 4, 8):
            k0 = B.block_key(3, 40000, -70000, -90000, -5, level)
            s = 4 << level
            k1 = B.block_key(3, 40000 + m * vx * s, -70000 + m * vy * s, -90000 + m * vz * s, -5, level)
            assert (B.bhash32(k1) - B.bhash32(k0)) % (1 << 32) == (-67 * m) % (1 << 32)
    # 160 blocks along it share a home slot, or two neighbouring ones, in every table of up to 2^17 slots
    assert 160 * 67 < 1 << (32 - 17)


# ---- every case is what it says ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(KL.CASES))
def test_case_has_the_level_counts_it_claims(name):
    cm, inv = KL.oracle_structure(name)
    batch = KL.case(name)
    assert tuple(len(cm.coords[1 << l]) for l in range(5)) == KL.CASES[name][1]
    assert len(batch) <= 1024 and len(inv) == int(TE.in_range(batch).sum())
    assert len(cm.coords[1]) == len(inv)                                   # one point per voxel: nothing merged by rounding


def test_corners_reach_both_limits_of_every_axis_at_every_level():
    from oracle import sps_oracle as O
    batch = KL.case("corners")
    want = np.concatenate([TE.grid(3, 3, 3, origin=o) for o, ts in KL.corner_cubes() for _ in ts])
    np.testing.assert_array_equal(O.quantize(batch[:, :5], TE.VS)[:, 1:4], want)       # float32 centres quantise to their voxel
    assert set(np.unique(batch[:, 4])) == {0.0, 1.0}
    for level in range(5):
        c = level_coords("corners", level)
        keys = block_keys("corners", level)
        for a in range(3):
            assert c[:, 1 + a].max() == 131072 - (1 << level) and c[:, 1 + a].min() == -131072, (level, a)
            field = [B.unpack(k)[2 + a] for k in keys]
            assert min(field) == 0 and max(field) == B.lim(level) - 1, (level, a)
        # the cubes with one axis at its limit: some block is at the limit of exactly one axis
        at = np.array([[B.unpack(k)[2 + a] in (0, B.lim(level) - 1) for a in range(3)] for k in keys])
        for a in range(3):
            assert np.any(at[:, a] & (at.sum(1) == 1)), (level, a)


def test_time_and_batch_cases_occupy_the_ends_of_their_fields():
    tb = level_coords("time_batch_carry", 0)
    have = {(int(b), int(t)) for b, t in tb[:, [0, 4]]}
    assert have == {(0, 15), (1, -16), (29, 15), (30, -16), (30, 15), (0, 14), (1, -15)}
    assert len({tuple(r) for r in tb[:, 1:4].tolist()}) == 8                 # the same 2 x 2 x 2 patch everywhere
    assert max(k >> 54 for k in block_keys("time_batch_carry", 0)) == (30 << 5) | 31      # the largest (b, t) the key holds
    at = level_coords("all_time_indices", 0)
    assert sorted(set(at[:, 4].tolist())) == list(range(-16, 16)) and set(at[:, 0].tolist()) == {0}
    # every row has both time neighbours, except the two end slices
    centre_up, centre_down = 40 + 27, 40 - 27
    k3 = oracle_k3("all_time_indices", 0)
    up = {o for k, i, o in k3 if k == centre_up}
    down = {o for k, i, o in k3 if k == centre_down}
    t = at[:, 4]
    assert up == set(np.flatnonzero(t < 15).tolist()) and down == set(np.flatnonzero(t > -16).tolist())


def test_bad_rows_are_one_step_outside_one_limit_each():
    from oracle import sps_oracle as O
    batch, good = KL.case("limits_with_bad_rows"), KL.case("corners")
    bad = np.flatnonzero(~TE.in_range(batch))
    assert bad.tolist() == [at + i for i, at in enumerate(KL.BAD_AT)] and len(bad) == 9
    np.testing.assert_array_equal(batch[TE.in_range(batch)], good)             # the other rows are `corners`, in its order
    q = O.quantize(batch[bad, :5], TE.VS).astype(np.int64)
    lo = np.array([0, TE.COORD_MIN, TE.COORD_MIN, TE.COORD_MIN, TE.T_MIN])
    hi = np.array([TE.BATCH_MAX, TE.COORD_MAX, TE.COORD_MAX, TE.COORD_MAX, TE.T_MAX])
    over, under = q - hi, lo - q
    step = np.maximum(over, under)                                             # > 0: that far outside
    assert (np.sort(step, axis=1)[:, -1] == 1).all() and ((step > 0).sum(1) == 1).all()
    assert sorted((int(np.argmax(s)), bool(o[np.argmax(s)] == 1)) for s, o in zip(step, over)) == \
        [(0, True), (1, False), (1, True), (2, False), (2, True), (3, False), (3, True), (4, False), (4, True)]


# ---- the chains ----------------------------------------------------------------------------------------------------------------
def family_keys(name, level):
    """the block keys of the four families of a chain case at `level`, family-major, k ascending"""
    K, m, anchor, _ = KL.CHAINS[name]
    v = KL.chain_voxels(K, m, anchor)
    return [[B.block_key(0, x, y, z, 1, level) for x, y, z in v[f * K:(f + 1) * K].tolist()] for f in range(4)]


def home_span(keys, slots):
    """slots from the first to the last home of `keys`, around the table"""
    h = sorted({B.home(k, slots) for k in keys})
    gaps = [(h[(i + 1) % len(h)] - h[i]) % slots for i in range(len(h))] if len(h) > 1 else [slots]
    return slots - max(gaps) if len(h) > 1 else 0


@pytest.mark.parametrize("name", list(KL.CHAINS))
def test_chain_cases_make_the_chains_they_claim(name):
    K, m, anchor, levels = KL.CHAINS[name]
    for level in range(5):
        keys = block_keys(name, level)
        table, disp = B.build_table(keys, KL.SLOTS)
        other, _ = B.build_table(keys[::-1], KL.SLOTS)
        assert set(table) == set(other)                                       # the occupied set is order-free
        assert B.is_probe_layout({k: s for s, k in table.items()}, KL.SLOTS)
        if level not in levels:
            continue
        fam = family_keys(name, level)
        assert sorted(k for f in fam for k in f) == sorted(keys) and len(keys) == 4 * K      # four families of K distinct blocks
        for f in fam:
            span = home_span(f, KL.SLOTS)
            assert span <= 1, (level, span)                                   # one home slot, or two neighbouring ones
            assert max(disp[k] for k in f) >= K - 1 - span, level
        # every family is the +x / -y / +z neighbour of the main one: each adjacency hit lies in a chain
        adj = B.block_adjacency(keys, level)
        for f, off in zip(fam[1:], ((1, 0, 0, 0), (0, -1, 0, 0), (0, 0, 1, 0))):
            assert all((a, off, b) in adj for a, b in zip(fam[0], f)), (level, off)
        k3 = oracle_k3(name, level)
        for k in (40 + 1, 40 - 3, 40 + 9):
            assert sum(1 for kk, _, _ in k3 if kk == k) == K, (level, k)       # and is a pair of the 3x3x3x3 map


@pytest.mark.parametrize("name,family", [("chain_wrap", 0), ("chain_wrap_rev", 0), ("chain_wrap_x", 1), ("chain_wrap_x_rev", 1)])
def test_wrap_cases_run_through_slot_0(name, family):
    keys = block_keys(name, 0)
    table, disp = B.build_table(keys, KL.SLOTS)
    fam = family_keys(name, 0)
    for f in range(4):
        homes = {B.home(k, KL.SLOTS) for k in fam[f]}
        if f == family:
            assert min(homes) >= KL.SLOTS - 8                                 # within 8 slots of the end of the table
            wrapped = [k for k in fam[f] if B.home(k, KL.SLOTS) + disp[k] >= KL.SLOTS]
            assert len(wrapped) >= 160 - 8
        else:
            assert all(B.home(k, KL.SLOTS) + disp[k] < KL.SLOTS for k in fam[f])      # the other chains stay inside
    assert {KL.SLOTS - 1, 0, 1} <= set(table)


# ---- the guards ----------------------------------------------------------------------------------------------------------------
def test_coordinate_guards_cannot_make_a_pair():
    """at either limit of a coordinate field, the unguarded sum is a key whose field lies outside [0, lim): no block has it"""
    for level in range(5):
        top = B.lim(level) - 1
        for axis in range(3):
            for at, d in ((0, -1), (top, 1)):
                for others in ((0, 0), (top, top), (5, top)):
                    field = list(others)
                    field.insert(axis, at)
                    key = (7 << 59) | (9 << 54) | (field[2] << 36) | (field[1] << 18) | field[0]
                    off = tuple(d if a == axis else 0 for a in range(3)) + (0,)
                    assert B.neighbour_keys(key, level, True)[off] is None
                    nk = B.neighbour_keys(key, level, False)[off]
                    assert not 0 <= B.unpack(nk)[2 + axis] < B.lim(level), (level, axis, at)


def test_dropping_the_time_guard_pairs_two_batch_items():
    for level in range(5):
        coords = level_coords("time_batch_carry", level)
        want = oracle_k3("time_batch_carry", level)
        assert B.kernel_map_3(coords, level, True) == want
        for keep in (("y", "z", "t"), ("x", "z", "t"), ("x", "y", "t")):
            assert B.kernel_map_3(coords, level, keep) == want, (level, keep)      # the coordinate guards: no difference
        for guards in (("x", "y", "z"), False):
            got = B.kernel_map_3(coords, level, guards)
            extra = got - want
            assert extra and not (want - got), level
            b, t = coords[:, 0], coords[:, 4]
            for k, i, o in extra:                                             # (b, 15) paired with (b + 1, -16), both ways
                assert {(int(b[i]), int(t[i])), (int(b[o]), int(t[o]))} in ({(0, 15), (1, -16)}, {(29, 15), (30, -16)})
            # the true neighbours (0, 14) / (0, 15) and (1, -16) / (1, -15) are pairs with and without the guard
            assert any({(int(b[i]), int(t[i])), (int(b[o]), int(t[o]))} == {(0, 14), (0, 15)} for k, i, o in want)
            assert any({(int(b[i]), int(t[i])), (int(b[o]), int(t[o]))} == {(1, -16), (1, -15)} for k, i, o in want)


def oracle_block_adjacency(coords, level):
    """{(block, offset, block)} from the oracle's coordinates by integer arithmetic on (b, t, x, y, z) tuples"""
    s = 4 << level
    blocks = {(int(b), int(t), int(x) // s, int(y) // s, int(z) // s) for b, x, y, z, t in np.asarray(coords).tolist()}
    out = set()
    for blk in blocks:
        b, t, x, y, z = blk
        for dt in (-1, 0, 1):
            for dz in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        n = (b, t + dt, x + dx, y + dy, z + dz)
                        if n in blocks:
                            out.add((blk, (dx, dy, dz, dt), n))
    return out


@pytest.mark.parametrize("name", list(KL.CASES))
def test_guarded_model_reproduces_the_oracle(name):
    for level in range(5):
        coords = level_coords(name, level)
        bias = B.XBIAS >> (level + 2)

        def plain(key):
            b, t, bx, by, bz = B.unpack(key)
            return (b, t, bx - bias, by - bias, bz - bias)

        got = {(plain(a), off, plain(n)) for a, off, n in B.block_adjacency(block_keys(name, level), level)}
        assert got == oracle_block_adjacency(coords, level), level
        assert B.kernel_map_3(coords, level) == oracle_k3(name, level), level
