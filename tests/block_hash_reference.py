"""A plain-Python model of the block key, the block hash and the block adjacency of the voxel front-end, written from the
header comments of sps_amd/csrc/grid_kernels.inc.h (not from its kernels), for tests/test_key_limits_cpu.py and
tests/test_hip_key_limits.py.  Integers are Python ints: nothing here can overflow, so what wraps is wrapped on purpose.

  key (level l)  [b:5 | t+16:5 | BZ:18 | BY:18 | BX:18],  BX = (x + 2^17) >> (l + 2): 0 <= BX < 2^(16 - l)
  bit            (pz << 4) | (py << 2) | px,  p = ((x + 2^17) >> l) & 3
  hash           BX * H_X + BY * H_Y + BZ * H_Z + (b:t+16) * H_T  mod 2^32 -- linear in the block coordinates
  slot           the TOP log2(slots) bits of the hash; a taken slot sends the key to the next one, modulo the table
  neighbour key  key + dx + (dy << 18) + (dz << 36) + (dt << 54), formed only where every coordinate stays in
                 [0, 2^(16 - l)) and the biased time index in [0, 32)
"""
import numpy as np

XBIAS, TBIAS = 1 << 17, 16
FIELD = 18
FMASK = (1 << FIELD) - 1
H_X, H_Y, H_Z, H_T = 0x9E3779B1, 0x85EBCA77, 0xC2B2AE3D, 0x27D4EB2F
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
GUARDS = ("x", "y", "z", "t")


# ---- keys --------------------------------------------------------------------------------------------------------------------
def block_key(b, x, y, z, t, level):
    """key of the 4x4x4 block (in units of 2^level voxels) that holds the voxel (b, x, y, z, t) -- level-0 coordinates"""
    s = level + 2
    return (int(b) << 59) | ((int(t) + TBIAS) << 54) | (((int(z) + XBIAS) >> s) << 36) | (((int(y) + XBIAS) >> s) << 18) | ((int(x) + XBIAS) >> s)


def block_pos(x, y, z, level):
    """(px, py, pz) of the voxel inside its block"""
    return tuple(((int(c) + XBIAS) >> level) & 3 for c in (x, y, z))


def block_bit(x, y, z, level):
    px, py, pz = block_pos(x, y, z, level)
    return (pz << 4) | (py << 2) | px


def unpack(key):
    """key -> (b, t, BX, BY, BZ): t unbiased, the block coordinates biased as in the key"""
    return key >> 59, ((key >> 54) & 31) - TBIAS, key & FMASK, (key >> 18) & FMASK, (key >> 36) & FMASK


def lim(level):
    """block coordinates of a level live in [0, lim)"""
    return 1 << (16 - level)


def keys_of(coords, level):
    """coords [V, 5] (b, x, y, z, t) integers -> list of (block key, bit) per row"""
    return [(block_key(b, x, y, z, t, level), block_bit(x, y, z, level)) for b, x, y, z, t in np.asarray(coords).tolist()]


# ---- the hash and its table --------------------------------------------------------------------------------------------------
def bhash32(key):
    _, _, bx, by, bz = unpack(key)
    return (bx * H_X + by * H_Y + bz * H_Z + (key >> 54) * H_T) & M32


def home(key, n_slots):
    bits = n_slots.bit_length() - 1
    assert 1 << bits == n_slots
    return bhash32(key) >> (32 - bits)


def build_table(keys, n_slots):
    """Linear probing of the distinct `keys`, inserted in the given order, into 2^n slots.
    -> (slot -> key, key -> displacement = slots walked from the key's home, modulo the table).  The SET of occupied slots
    does not depend on the insertion order (the displacements do)."""
    table, disp = {}, {}
    for k in keys:
        if k in disp:
            continue
        s = h = home(k, n_slots)
        while s in table:
            s = (s + 1) & (n_slots - 1)
        table[s] = k
        disp[k] = (s - h) & (n_slots - 1)
        assert len(table) < n_slots
    return table, disp


def is_probe_layout(slot_of, n_slots):
    """key -> slot is a layout that a walk from the home slot finds every key in: all slots from home(key) to slot_of[key]
    are taken, and no two keys share a slot"""
    taken = set(slot_of.values())
    if len(taken) != len(slot_of):
        return False
    for k, s in slot_of.items():
        h = home(k, n_slots)
        for i in range((s - h) & (n_slots - 1)):
            if ((h + i) & (n_slots - 1)) not in taken:
                return False
    return True


# ---- adjacency ---------------------------------------------------------------------------------------------------------------
def _enforced(guards):
    if guards is True:
        return frozenset(GUARDS)
    if guards is False:
        return frozenset()
    g = frozenset(guards)
    assert g <= set(GUARDS)
    return g


def neighbour_keys(key, level, guards=True):
    """{(dx, dy, dz, dt) in {-1, 0, 1}^4: key of the block at that offset, or None where an enforced guard stops it}.
    guards: True (all four), False (none: the plain sum modulo 2^64) or the names of the guards that stay, of "x", "y", "z"
    (the coordinate stays in [0, lim)) and "t" (the biased time index stays in [0, 32))."""
    g = _enforced(guards)
    _, t, bx, by, bz = unpack(key)
    tt = t + TBIAS
    out = {}
    for dt in (-1, 0, 1):
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    ok = (("x" not in g or 0 <= bx + dx < lim(level)) and ("y" not in g or 0 <= by + dy < lim(level))
                          and ("z" not in g or 0 <= bz + dz < lim(level)) and ("t" not in g or 0 <= tt + dt < 32))
                    out[(dx, dy, dz, dt)] = (key + dx + (dy << 18) + (dz << 36) + (dt << 54)) & M64 if ok else None
    return out


def block_adjacency(keys, level, guards=True):
    """{(key, offset, neighbour key)} over the distinct block keys: the neighbour exists"""
    have = set(keys)
    out = set()
    for k in have:
        for off, nk in neighbour_keys(k, level, guards).items():
            if nk is not None and nk in have:
                out.add((k, off, nk))
    return out


def kernel_map_3(coords, level, guards=True):
    """The 3x3x3x3 kernel map of the voxel set coords [V, 5] (b, x, y, z, t; level-0 units, multiples of 2^level) as the
    front-end derives it: neighbour voxel = adjacent block (by key arithmetic) + bit inside it.
    -> set of (k, in row, out row), k = (dx + 1) + 3 (dy + 1) + 9 (dz + 1) + 27 (dt + 1), in = out + offset"""
    c = np.asarray(coords).tolist()
    row = {}
    for r, (b, x, y, z, t) in enumerate(c):
        row[(block_key(b, x, y, z, t, level), block_bit(x, y, z, level))] = r
    assert len(row) == len(c)
    nbk = {}
    out = set()
    for r, (b, x, y, z, t) in enumerate(c):
        key = block_key(b, x, y, z, t, level)
        if key not in nbk:
            nbk[key] = neighbour_keys(key, level, guards)
        px, py, pz = block_pos(x, y, z, level)
        for dt in (-1, 0, 1):
            for dz in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        qx, qy, qz = px + dx, py + dy, pz + dz
                        nk = nbk[key][(qx >> 2, qy >> 2, qz >> 2, dt)]
                        if nk is None:
                            continue
                        i = row.get((nk, ((qz & 3) << 4) | ((qy & 3) << 2) | (qx & 3)))
                        if i is not None:
                            out.add(((dx + 1) + 3 * (dy + 1) + 9 * (dz + 1) + 27 * (dt + 1), i, r))
    return out


def oracle_pairs(kmap):
    """an oracle kernel map (per offset the (in, out) index lists) as the same kind of set"""
    return {(k, int(a), int(b)) for k, (i, o) in enumerate(kmap) for a, b in zip(i, o)}
