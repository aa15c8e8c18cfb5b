"""GPU tests of the voxel front-end (k_points_to_blocks, the ranking kernels, link_levels, k_link_adj, build_nbr3_t) on the
scenes of tests/key_limit_inputs.py: rows at both ends of every field of the block key, all 32 time indices at once, the
carry from t = 15 into the batch index, rows one step outside each limit, and blocks that collide in the block hash by
construction -- chains of 160 slots, through the end of the table, in the tables of 2048 slots of a context of their own.

Everything is compared as test_hip_parity.check_full compares it: voxel sets, parents, inverse, all ten kernel maps and the
rulebooks exactly as pair sets, every tapped feature map within 2e-4, logits within 1e-3, scores within 1e-4.  The block
hash is observed, not assumed: sps_get_block_slots gives the table size and the slot of every block, and the occupied slots
must be those of the plain model in tests/block_hash_reference.py (test_key_limits_cpu.py holds that model against the
oracle).

Features do not depend on where a structure sits, so the 2e-4 of the small scenes is kept for the scenes at 13 km."""
import numpy as np
import pytest
import torch

from oracle import sps_oracle as O
from sps_amd import synthetic
from tests import block_hash_reference as B
from tests import key_limit_inputs as KL
from tests import train_edge_inputs as TE
from tests.helpers import net_from_params, state_dict_from_params, straddle_params
from tests.test_hip_parity import check_full, ctx, get_feature, get_voxels, run

pytestmark = pytest.mark.gpu

VS = TE.VS
TAPS = ("out_p1", "block1", "block2", "block3", "block4", "block5", "block6", "block7", "block8")


@pytest.fixture(scope="module")
def params():
    return straddle_params(O.random_params(seed=0), synthetic.small_scene(seed=11, n_scan=2500))


@pytest.fixture(scope="module")
def net(params):
    assert torch.cuda.is_available()
    return net_from_params(params).cuda().eval().freeze()


@pytest.fixture(scope="module")
def side():
    """a stream of its own: models.get_context gives it a fresh context, which the first forward (every scene here has at
    most 1024 rows) reserves for 1024 rows -- 2048 slots in the block hash of every level"""
    from sps_amd.models import models as M
    st = torch.cuda.Stream()
    yield st
    st.synchronize()
    c = M._CONTEXTS.pop((0, int(st.cuda_stream)), None)
    if c is not None:
        c.close()


def scene(name):
    """a writable copy of a case (torch.from_numpy warns about read-only arrays)"""
    return KL.case(name).copy()


def no_flag():
    ctx().check_errors(torch.cuda.current_stream().cuda_stream)


# ---- the ends of the key fields ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["corners", "time_batch_carry", "all_time_indices"])
def test_key_limits_full_parity(net, params, name):
    """corners: block coordinates 0 and lim - 1 at every level -- the x / y / z guards of k_link_adj, the shifts of
    k_rank_points and link_levels at full field width.  time_batch_carry: (b, t = 15) and (b + 1, t = -16) in the same
    voxels -- without the time guard of k_link_adj (0 <= tt < 32) and of build_nbr3_t they would be neighbours; b = 30.
    all_time_indices: the occupancy word of the time indices is all ones, the shift by tt reaches bit 31."""
    check_full(net, params, scene(name))
    assert tuple(ctx().level_counts()) == KL.CASES[name][1]
    no_flag()


def test_rows_one_step_outside_each_limit(net, params):
    """limits_with_bad_rows = corners + nine rows one step beyond x, y, z (both ways), t = 16, t = -17, b = 31: NaN scores
    and inverse -1 on those, the sticky range error once, and the bits of `corners` on every other row"""
    from sps_amd import _native
    good, batch = scene("corners"), scene("limits_with_bad_rows")
    bad = ~TE.in_range(batch)
    _, s = run(net, good)
    want = s.cpu().numpy().copy()
    no_flag()
    _, s = run(net, batch)
    with pytest.raises(_native.SpsError) as e:
        no_flag()
    assert e.value.code == -4
    no_flag()                                                    # raised once
    got = s.cpu().numpy()
    assert np.isnan(got[bad]).all()
    np.testing.assert_array_equal(got[~bad], want)
    assert tuple(ctx().level_counts()) == KL.CASES["limits_with_bad_rows"][1]
    inv = torch.empty(len(batch), dtype=torch.int64, device="cuda")
    _native.check(_native.lib.sps_get_inverse(ctx().handle, inv.data_ptr()))
    inv = inv.cpu().numpy()
    assert (inv[bad] == -1).all() and sorted(set(inv[~bad].tolist())) == list(range(270))


# ---- colliding blocks --------------------------------------------------------------------------------------------------------
def check_tables(name):
    """The block hash of every level of the last forward (of scene `name`) against the model: 2048 slots; the occupied slots
    are the model's; every block is where a walk from its home slot finds it; at the levels where the scene makes chains,
    some block of each of the four families sits at least K - 1 - (slots between the family's homes) slots from home.
    -> the slots by rank, per level"""
    c = ctx()
    counts = c.level_counts()
    cm, _ = KL.oracle_structure(name)
    out = []
    for level in range(5):
        slots, bslot = c.block_slots(level)
        assert slots == KL.SLOTS, (level, slots)
        keys = list(dict.fromkeys(k for k, _ in B.keys_of(get_voxels(level, counts[level]), level)))    # rows are block-contiguous
        want_keys = {k for k, _ in B.keys_of(cm.coords[1 << level], level)}
        assert set(keys) == want_keys and len(keys) == len(bslot), level
        table, _ = B.build_table(sorted(want_keys), slots)
        assert set(bslot.tolist()) == set(table), level
        slot_of = dict(zip(keys, bslot.tolist()))
        assert B.is_probe_layout(slot_of, slots), level
        if name in KL.CHAINS and level in KL.CHAINS[name][3]:
            K, m, anchor, _ = KL.CHAINS[name]
            v = KL.chain_voxels(K, m, anchor)
            for f in range(4):
                fam = [B.block_key(0, x, y, z, 1, level) for x, y, z in v[f * K:(f + 1) * K].tolist()]
                homes = sorted({B.home(k, slots) for k in fam})
                span = 0 if len(homes) == 1 else min((homes[-1] - homes[0]) % slots, (homes[0] - homes[-1]) % slots)
                assert span <= 1
                disp = max((slot_of[k] - B.home(k, slots)) % slots for k in fam)
                print(f"CHAIN {name} level {level} family {f}: homes {homes} largest displacement {disp}")
                assert disp >= K - 1 - span, (level, f, disp)
        out.append(bslot)
    return out


@pytest.mark.parametrize("name", list(KL.CHAINS))
def test_chains_full_parity(net, params, side, name):
    """k_link_adj's probes land in the chain's home slot, which holds another block: every adjacency hit goes through
    bhash_find_from, up to 160 slots far (chain160), at levels 0 to 3 (chain40x8), through `& hmask` at the end of the
    level-0 table, whose neighbour in memory is the level-1 table (chain_wrap: the main chain, chain_wrap_x: the +x one).
    The reversed point order changes every rank and no pair."""
    with torch.cuda.stream(side):
        check_full(net, params, scene(name))
        assert tuple(ctx().level_counts()) == KL.CASES[name][1]
        check_tables(name)
        no_flag()


def snapshot(net, params, name):
    dev, s, _ = check_full(net, params, scene(name))
    return dict(scores=s.copy(), slots=check_tables(name), feats={n: get_feature(n) for n in TAPS},
                maps=[ctx().kernel_map(w, 0).cpu().numpy() for w in range(10)])


@pytest.mark.parametrize("name", ["chain_wrap", "chain_wrap_x"])
def test_cleanup_after_a_wrapped_chain(net, params, side, name):
    """bhash_cleanup frees the slots of a chain that ran through the end of the table: a collision-free scene on the same
    context is right in full afterwards (a key left behind would be a block that is not there, a slot left taken would move
    its blocks), its tables are the model's, and the wrapped scene run again gives the bits of its first run."""
    with torch.cuda.stream(side):
        first = snapshot(net, params, name)
        control = synthetic.small_scene(seed=8, n_scan=600)
        assert len(control) < 1024
        check_full(net, params, control, both_classes=True)
        for level in range(5):
            slots, bslot = ctx().block_slots(level)
            counts = ctx().level_counts()
            keys = list(dict.fromkeys(k for k, _ in B.keys_of(get_voxels(level, counts[level]), level)))
            assert slots == KL.SLOTS and len(keys) == len(bslot)
            table, _ = B.build_table(keys, slots)
            assert set(bslot.tolist()) == set(table), level          # nothing of the chain is in the way
            assert B.is_probe_layout(dict(zip(keys, bslot.tolist())), slots), level
        again = snapshot(net, params, name)
        np.testing.assert_array_equal(first["scores"], again["scores"])
        for level in range(5):
            # (which block of a chain gets which of its slots follows the order the inserting waves arrive in: the occupied
            # set is fixed, a block's slot is not, and nothing downstream depends on it)
            assert set(first["slots"][level].tolist()) == set(again["slots"][level].tolist()), level
        for n in TAPS:
            np.testing.assert_array_equal(first["feats"][n], again["feats"][n], err_msg=n)
        for w in range(10):
            np.testing.assert_array_equal(first["maps"][w], again["maps"][w], err_msg=f"kernel map {w}")
        no_flag()


# ---- the heads: a scan index far outside the key's time field ----------------------------------------------------------------
def test_rebased_scan_indices_give_the_same_bits():
    """A 4DMOS-style buffer of 16 scans with indices 1234 .. 1249 (baselines._t_base re-bases them to 0 .. 15, the upper end
    of the time field) against the same cloud with indices 0 .. 15: all three columns bit for bit, and the oracle's values"""
    from sps_amd.models.baselines import MOS4DNet
    from sps_amd.models.models import get_context
    p = O.random_params(seed=4, out_channels=3)
    m = MOS4DNet(VS)
    m.MinkUNet.load_state_dict(state_dict_from_params(p, prefix=""))
    m = m.cuda().eval().freeze()
    rows = KL.case("all_time_indices")
    c = rows[rows[:, 4] >= 0, :5].copy()
    assert sorted(set(c[:, 4].tolist())) == list(range(16))
    far = c.copy()
    far[:, 4] += 1234
    out = {}
    for tag, arr in (("near", c), ("far", far)):
        out[tag] = m._run(torch.from_numpy(arr).cuda(), None, VS).cpu().numpy()
        get_context(0).check_errors(torch.cuda.current_stream().cuda_stream)
    assert out["near"].shape == (len(c), 3)
    np.testing.assert_array_equal(out["far"], out["near"])
    want, _ = O.head_forward(p, c, VS)
    np.testing.assert_allclose(out["near"], want, rtol=0, atol=2e-4)      # the bound of tests/test_hip_heads.py for this network
