"""CPU half of the training-backward edge tests: the scenes of tests/train_edge_inputs.py have the level counts they claim,
the plan tables are what train_reserve's arithmetic gives, the float32 / float64 yardstick is finite, and the tolerance
built from it has teeth -- three mutants of the oracle's backward exceed it while the float32 oracle stays inside.
No GPU, no native library."""
import numpy as np
import pytest
import torch

from tests import train_edge_inputs as TE


@pytest.mark.parametrize("name", list(TE.CASES))
def test_case_has_the_level_counts_it_claims(name):
    batch = TE.case(name)
    counts, inv = TE.level_counts(batch)
    assert counts == TE.CASES[name][1]
    assert counts[4] >= 2 and min(counts) >= 2                  # train-mode BatchNorm refuses a single row
    assert len(inv) == int(TE.in_range(batch).sum()) and len(batch) > counts[0]      # some voxel holds several points


def test_the_cases_are_the_edges_they_are_named_after():
    assert TE.CASES["min"][1][0] == 17 and TE.CASES["min"][1][4] == 2
    assert [TE.CASES[n][1][0] for n in TE.TILE_EDGES] == [16, 17, 64, 65, 257]
    # dupes: 40 points in one voxel
    _, inv = TE.level_counts(TE.case("dupes"))
    assert np.bincount(inv).max() == 40
    # off_range: six rows outside the key range, at the start, inside and at the end; none of them is a scan row
    batch = TE.case("off_range")
    bad = np.flatnonzero(~TE.in_range(batch))
    assert len(bad) == 6 and bad[0] == 0 and bad[-1] == len(batch) - 1 and 2 < bad[2] < len(batch) - 3
    assert not np.any(batch[bad, 4] == 1)
    # dust and brick fill two time slices
    for name in ("dust", "brick"):
        assert set(np.unique(TE.case(name)[:, 4])) == {0.0, 1.0}
    big, _ = TE.level_counts(TE.case("big"))
    assert big[0] > 3000


def _offsets_with_pairs(name, ts):
    from oracle import sps_oracle as O
    batch = TE.case(name)
    vox, _ = O.unique_first(O.quantize(batch[TE.in_range(batch), :5], TE.VS))
    cm = O.CoordinateManager(vox)
    cm.ensure_stride(16)
    return cm, cm.k3(ts)


def test_dust_leaves_most_offsets_empty_and_brick_fills_all_27():
    for l in range(5):
        cm, km = _offsets_with_pairs("dust", 1 << l)
        n = len(cm.coords[1 << l])
        tiles = (n + 15) // 16
        # (tile, offset) slots that hold a pair: the centre in every tile, few others
        used = sum(len(np.unique(np.asarray(o) // 16)) for i, o in km if len(i))
        assert used < 0.1 * 81 * tiles, (l, used, tiles)
        assert sum(1 for k, (i, o) in enumerate(km) if len(i) and k != TE.CENTRE) >= 2, l      # but not none
    _, km = _offsets_with_pairs("brick", 1)
    assert sum(1 for i, o in km if len(i)) == 81


def test_plans_are_the_three_the_capacities_were_chosen_for():
    p = TE.plan(TE.CAP_MIN)
    assert set(p.values()) == {(4, 1)} and len(p) == 31
    p = TE.plan(TE.CAP_WIDE)
    for name in ("block8.0.conv1", "block8.0.conv2"):
        assert p[name] == (6, 13)                               # 64 rows per step, a slab of 13 partials: not a power of two
    assert TE.in_words(p) == {
        (4, 3): ["block4.0.conv1"], (4, 4): ["conv4p8s2", "block4.0.downsample.0", "convtr4p16s2"],
        (4, 8): ["conv3p4s2", "block3.0.downsample.0", "block5.0.downsample.0", "convtr5p8s2"],
        (4, 32): ["conv2p2s2", "block2.0.downsample.0", "block6.0.downsample.0", "convtr6p4s2"],
        (4, 64): ["block7.0.downsample.0", "block8.0.downsample.0"], (6, 1): ["block4.0.conv2"], (6, 5): ["block5.0.conv1"],
        (6, 6): ["block3.0.conv1", "block3.0.conv2"], (6, 7): ["block5.0.conv2", "block6.0.conv1"],
        (6, 13): ["block1.0.conv1", "block1.0.conv2", "block2.0.conv1", "block2.0.conv2", "block6.0.conv2", "block7.0.conv1",
                  "block7.0.conv2", "block8.0.conv1", "block8.0.conv2"],
        (6, 64): ["conv1p1s2", "convtr7p2s2"]}
    p = TE.plan(TE.CAP_MIXED)
    assert TE.in_words(p) == {
        (4, 1): ["conv3p4s2", "block3.0.conv1", "block3.0.conv2", "block3.0.downsample.0", "conv4p8s2", "block4.0.conv1",
                 "block4.0.conv2", "block4.0.downsample.0", "convtr4p16s2", "block5.0.conv1", "block5.0.conv2",
                 "block5.0.downsample.0", "convtr5p8s2"],
        (4, 2): ["conv2p2s2", "block2.0.downsample.0", "block6.0.downsample.0", "convtr6p4s2"],
        (4, 3): ["block2.0.conv1", "block2.0.conv2", "block6.0.conv1", "block6.0.conv2"],
        (4, 8): ["conv1p1s2", "block7.0.downsample.0", "convtr7p2s2"], (4, 16): ["block8.0.downsample.0"],
        (6, 3): ["block1.0.conv1", "block1.0.conv2", "block7.0.conv1", "block7.0.conv2"],
        (6, 6): ["block8.0.conv1", "block8.0.conv2"]}
    # the weight-gradient layers are the network's: every kernel but conv0 (its own kernel) and final (the head)
    from oracle import sps_oracle as O
    kernels = {k[: -len(".kernel")] for k in O.random_params(seed=0) if k.endswith(".kernel")}
    assert {n for n, *_ in TE.WG_LAYERS} == kernels - {"conv0p1s1", "final"}


@pytest.mark.parametrize("case,cot", TE.PAIRS)
def test_yardstick_is_finite_and_the_float32_oracle_is_inside_the_tolerance(case, cot):
    ref = TE.reference(case, TE.cotangent(case, cot))
    assert set(ref["e32"]) == set(ref["g64"]) and len(ref["e32"]) > 90
    for name, e in ref["e32"].items():
        assert np.isfinite(e), name
        assert e <= TE.allowed(e)
    assert np.isfinite(ref["e32_scores"])
    if cot != "off_range_only":
        assert max(np.abs(v).max() for v in ref["g64"].values()) > 0


@pytest.mark.parametrize("case", TE.ADDITIVE_CASES)
def test_yardstick_of_the_summed_cotangent_is_finite(case):
    g1, g2, both = TE.additive_parts(case)
    assert np.array_equal(both, (g1 + g2).astype(np.float32)) and np.abs(g2).max() > 0
    ref = TE.reference(case, both)
    assert all(np.isfinite(e) for e in ref["e32"].values())
    assert max(np.abs(v).max() for v in ref["g64"].values()) > 0


def test_off_range_only_gives_exactly_zero_in_the_oracle():
    g = TE.cotangent("off_range", "off_range_only")
    bad = ~TE.in_range(TE.case("off_range"))
    assert np.all(g[bad] != 0) and np.all(g[~bad] == 0)
    ref = TE.reference("off_range", g)
    for which in ("g64", "g32"):
        for name, v in ref[which].items():
            assert np.all(v == 0.0), (which, name)
    assert all(e == 0.0 for e in ref["e32"].values())


@pytest.mark.parametrize("case", list(TE.CASES))
def test_every_mutant_exceeds_the_tolerance(case):
    """Per case, every mutant is caught by at least one of the cotangents the GPU test runs on it, on at least one
    tensor (a dlogit rounded to 2^-20 cannot show under a cotangent of unit scale: the MSE's is the one that is small
    enough).  The unmutated float32 oracle is inside the tolerance on every tensor by construction (16 x its own
    distance); what the test adds is that a SECOND float32 run gives the same bits -- the oracle runs on one thread, so
    the yardstick is reproducible."""
    caught = {m: [] for m in TE.MUTANTS}
    batch = TE.case(case)
    for c, cot in TE.PAIRS:
        if c != case or cot == "off_range_only":
            continue
        g = TE.cotangent(case, cot)
        ref = TE.reference(case, g)
        ok = TE.allowed(ref["e32"])
        _, again = TE.oracle_step(batch, g, torch.float32)
        for name, want in ref["g64"].items():
            np.testing.assert_array_equal(again[name], ref["g32"][name], err_msg=name)
            assert TE.rel_err(again[name], want) <= ok[name], (cot, name)
        for m in TE.MUTANTS:
            s, grads = TE.oracle_step(batch, g, torch.float32, mutant=m)
            np.testing.assert_array_equal(s, ref["s32"])         # the forward stays intact
            over = [name for name, want in ref["g64"].items() if TE.rel_err(grads[name], want) > ok[name]]
            if over:
                caught[m].append((cot, len(over)))
    assert all(caught.values()), caught


def test_drop_pair_mutant_changes_one_offset_of_one_layer():
    g = TE.cotangent("brick", "random")
    ref = TE.reference("brick", g)
    _, grads = TE.oracle_step(TE.case("brick"), g, torch.float32, mutant="drop_pair")
    changed = [name for name in grads if not np.array_equal(grads[name], ref["g32"][name])]
    assert changed == ["block8.0.conv1.kernel"]
    d = np.abs(grads[changed[0]] - ref["g32"][changed[0]]).reshape(81, -1).max(axis=1)
    assert np.count_nonzero(d) == 1 and d[TE.CENTRE] == 0
