"""(no GPU) The scenes of tests/coarse_conv_inputs.py make k_conv at levels 2-4 do what they were built for, and the
restatement of tests/coarse_conv_reference.py is the oracle's network."""
import numpy as np
import pytest

from oracle import sps_oracle as O
from tests import coarse_conv_inputs as I
from tests import coarse_conv_reference as R


@pytest.fixture(scope="module")
def facts():
    return {name: I.tile_facts(b) for name, b in I.scenes().items()}


def test_scenes_are_small(facts):
    for name, b in I.scenes().items():
        assert len(b) <= 4200, (name, len(b))


@pytest.mark.parametrize("level", I.LEVELS)
def test_unit_lists_of_every_length(facts, level):
    """nk = 1 .. 5 and 9 in the level's own scene, tile by tile as built; a tile with all 27 spatial offsets and more."""
    nk = facts[f"units_l{level}"][level]["nk"]
    n = len(I.UNIT_NK)
    assert nk[:n].tolist() == list(I.UNIT_NK), nk[:n + 1]
    assert nk[n] == 2                                      # isolated voxels with a partner in the other time slice
    # the 13 clusters lie along the 13 directions: the short-list tiles hold the centre and all 26 other offsets of dt = 0,
    # and nothing else -- no offset is left to the dense block alone
    short = facts[f"units_l{level}"][level]["pres"][:n].any(0)
    assert short[27:54].all() and not short[:27].any() and not short[54:].any(), np.nonzero(~short[27:54])[0]
    assert {1, 2, 3, 4, 5} <= set(nk.tolist()) and ({8, 9} & set(nk.tolist())) and nk.max() >= 27, sorted(set(nk.tolist()))
    # upk = 2, 4, 8, 12, 16, 24 (the C_in of levels 2-4 / 4): which splits of S = 4 get units, and where the last one ends
    shapes = set()
    for upk in (2, 4, 8, 12, 16, 24):
        for n in set(nk.tolist()):
            U = n * upk
            per = (-(-U // 4) + 3) & ~3
            shapes.add((min(4, -(-U // per)), U % per != 0, per % upk != 0))
    assert {s[0] for s in shapes} == {1, 2, 3, 4}         # splits that hold units: 1 (three empty) .. 4
    assert any(s[1] for s in shapes) and any(s[2] for s in shapes)      # a short last split; a boundary inside an offset
    assert (1, True, False) in shapes                      # nk = 1, upk = 2 (block2.conv1): 2 of split 0's 4 slots, no more


@pytest.mark.parametrize("level", I.LEVELS)
def test_last_tiles_and_tile_counts(facts, level):
    rows = {name: f[level]["rows"] for name, f in facts.items()}
    assert rows["single"] == 1
    for n in I.COUNT_ROWS:
        assert rows[f"count_{n}"] == n                     # the same count at every level
    last = {(r - 1) % 16 + 1 for r in rows.values()}
    assert {1, 15, 16} <= last
    tiles = {-(-r // 16) for r in rows.values()}
    want = {63, 64, 65, 127, 128, 129} | ({255, 256, 257} if level == 2 else set())
    assert want <= tiles, sorted(tiles)


@pytest.mark.parametrize("level", I.LEVELS)
def test_child_octant_masks(facts, level):
    """Tiles whose children miss octants (one child each: 0x0F over 16 isolated rows, a single bit elsewhere) and tiles with
    all eight: what the fused convtr6p4s2 (level 2) and k_upconv (levels 3, 4) skip by."""
    om = np.concatenate([f[level]["omask"] for f in facts.values()])
    assert (om > 0).all()                                  # every row has a child
    assert (om == 0xFF).any() and (om == 0x0F).any() and (om == 1).any(), sorted(set(om.tolist()))
    own = facts[f"units_l{level}"][level]["omask"]
    assert own[0] == 0x0F and (own == 0xFF).sum() >= 4


@pytest.fixture(scope="module")
def oracle_run():
    params = O.random_params(seed=0)
    batch = I.units_scene(3)
    _, info = O.sps_forward(params, batch[:, :5], I.VS, keep=True)
    return params, info


@pytest.mark.parametrize("block", R.BLOCKS)
def test_restatement_is_the_oracles_network(oracle_run, block):
    """The float32 form, offsets in ascending order, fed the ORACLE's taps gives the oracle's next tap; the float64 form
    differs from it by float32 rounding only."""
    params, info = oracle_run
    taps = info["inter"]
    got = R.block_from_taps(params, info["cm"], taps, block, np.float32, "ascending")
    np.testing.assert_array_equal(got, taps[block])
    ref = R.block_from_taps(params, info["cm"], taps, block, np.float64)
    assert ref.dtype == np.float64
    np.testing.assert_allclose(taps[block], ref, rtol=0, atol=2e-5 * max(1.0, np.abs(ref).max()))
    for order in ("descending", "splits"):
        alt = R.block_from_taps(params, info["cm"], taps, block, np.float32, order)
        np.testing.assert_allclose(alt, ref, rtol=0, atol=2e-5 * max(1.0, np.abs(ref).max()))
    spread = R.spread(params, info["cm"], taps, block, ref)
    assert 0 < spread < 1e-4 * max(1.0, np.abs(ref).max())


def test_launch_getter_rejects_bad_arguments_without_a_gpu():
    """sps_get_conv_launch: host only; null arguments fail before anything is read."""
    import ctypes
    from sps_amd import _native
    out = (ctypes.c_int32 * 8)()
    assert _native.lib.sps_get_conv_launch(None, b"block3.0.conv1", out) < 0
    assert b"null argument" in _native.lib.sps_last_error()
