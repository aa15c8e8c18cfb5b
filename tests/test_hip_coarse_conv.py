"""k_conv at levels 2-4 (conv_kernels.inc.h) in every launch geometry, on scenes built for what it does with a tile.

Which instantiation runs follows from the arena capacity of the context and its pipelined hint (conv_geometry, sps_hip.hip),
and the capacity of a context only grows: on the shared default context the kernels under test depend on which tests ran
before.  Here every geometry gets a FRESH context on a stream of its own, reserved to one capacity of its regime, and
sps_get_conv_launch says what was launched -- the expected values stand in ONE table (geometry(), NTW_OF) below.

Per scene of tests/coarse_conv_inputs.py (counts asserted without a GPU in tests/test_coarse_conv_cpu.py):
  * scores and all nine taps are bit-identical in all five geometries, and a second forward repeats the first;
  * they match the oracle (check_full of test_hip_parity: integer structure exactly, features to 2e-4) where all six wide
    layers run one column tile per wave and where all run two;
  * the device's own kernel maps give the CPU's present-offset count and child octants tile by tile;
  * every block 2 .. 7 equals a float64 reference of that block computed from the DEVICE's upstream taps, within
    max(16 spread, 1e-6 max|ref|), spread = what the float32 form of the reference itself loses in three summation orders
    (tests/coarse_conv_reference.py).  Measured (profiles/coarse_conv/README.md): device error / spread 0.51 .. 2.21.

Arena of the largest context (524 288 rows, full-size levels): 3 747 MiB by arena_bytes(); the five together hold 6.5 GiB
and are destroyed when the module is done."""
import numpy as np
import pytest
import torch

from oracle import sps_oracle as O
from tests import coarse_conv_inputs as I
from tests import coarse_conv_reference as R
from tests import test_hip_parity as P
from tests.helpers import net_from_params, straddle_params

pytestmark = pytest.mark.gpu

TAPS = ("out_p1", "block1", "block2", "block3", "block4", "block5", "block6", "block7", "block8")

# name -> (rows reserved, pipelined hint).  One capacity per regime of the rule below.
REGIMES = {"cap8k": (8192, False), "cap128k": (131072, False), "cap256k": (262144, False), "cap512k": (524288, False),
           "cap8k_pipelined": (8192, True)}
# The 800-workgroup rule (conv_geometry): a serial context runs the wide 3x3x3x3 layers of levels 3-4 with ONE column tile per
# wave while (expected tiles) x (column tiles) <= 800, expected tiles = cap * 33 / 1000 / 16 at level 3, cap * 11 / 1000 / 16
# at level 4 -- block5 (4 column tiles, level 3) up to 97 280 rows, block3 (2, level 3) up to 193 536, block4 (4, level 4) up to
# 291 840; a pipelined context always two.  A retune of the rule edits NTW_OF and nothing else.
NTW_OF = {"cap8k": {"block3": 1, "block4": 1, "block5": 1}, "cap128k": {"block3": 1, "block4": 1, "block5": 2},
          "cap256k": {"block3": 2, "block4": 1, "block5": 2}, "cap512k": {"block3": 2, "block4": 2, "block5": 2},
          "cap8k_pipelined": {"block3": 2, "block4": 2, "block5": 2}}
WIDE = {"block3": 2, "block4": 4, "block5": 4}             # column tiles (C_out / 16) of the six layers the rule is about
ORDER_WAYS = 256                                           # positions per tier of the balanced order, over the column groups


def geometry(regime):
    """layer -> (family, ntw, S, U4, fused transposed convolution, order_ways) expected in `regime`."""
    g = {"conv0p1s1": ("conv0", 0, 0, False, False, 0),
         "conv1p1s2": ("k_conv", 1, 1, False, False, 0), "conv2p2s2": ("k_conv", 1, 1, False, False, 0),
         "conv3p4s2": ("k_conv", 1, 4, True, False, 0), "conv4p8s2": ("k_conv", 2, 4, True, False, 0),
         "convtr4p16s2": ("k_upconv", 0, 0, False, False, 0), "convtr5p8s2": ("k_upconv", 0, 0, False, False, 0),
         "convtr6p4s2": ("none", 0, 0, False, False, 0), "convtr7p2s2": ("none", 0, 0, False, False, 0),
         # level 2: C_in = 8 (two units per offset) and the 8-channel downsample keep block2 off the U4 loop
         "block2.0.conv1": ("k_conv", 1, 4, False, False, ORDER_WAYS), "block2.0.conv2": ("k_conv", 1, 4, False, False, ORDER_WAYS),
         "block6.0.conv1": ("k_conv", 2, 4, True, False, ORDER_WAYS), "block6.0.conv2": ("k_conv", 2, 4, True, True, ORDER_WAYS)}
    for b in ("block1", "block7", "block8"):
        for c in ("conv1", "conv2"):
            g[f"{b}.0.{c}"] = ("k_conv_px", 1, 1, False, b == "block7" and c == "conv2", 0)
    for b, nt in WIDE.items():
        ntw = NTW_OF[regime][b]
        for c in ("conv1", "conv2"):
            g[f"{b}.0.{c}"] = ("k_conv", ntw, 4, True, False, ORDER_WAYS // (nt // ntw))
    return g


def launched(c, cap, pipelined):
    out = {}
    for name in geometry("cap8k"):
        d = c.conv_launch(name)
        if d["family"] != "none":
            assert (d["cap"], d["pipelined"]) == (cap, pipelined), (name, d)
        out[name] = (d["family"], d["ntw"], d["S"], d["U4"], d["fused_up"], d["order_ways"])
    return out


@pytest.fixture(scope="module")
def params():
    from sps_amd import synthetic
    return straddle_params(O.random_params(seed=0), synthetic.small_scene(seed=11, n_scan=2500))


@pytest.fixture(scope="module")
def net(params):
    assert torch.cuda.is_available()
    return net_from_params(params).cuda().eval().freeze()


@pytest.fixture(scope="module")
def contexts():
    """regime -> (stream, fresh context reserved to the regime's capacity); destroyed afterwards."""
    from sps_amd.models import models as M
    out = {}
    for name, (cap, pipelined) in REGIMES.items():
        st = torch.cuda.Stream()
        assert (0, st.cuda_stream) not in M._CONTEXTS
        c = M.get_context(0, st.cuda_stream)
        c.reserve(cap)
        c.set_pipelined(pipelined)
        out[name] = (st, c)
    print(f"\narena_bytes: " + ", ".join(f"{n} {c.arena_bytes() / 2**20:.0f} MiB" for n, (_, c) in out.items()))
    yield out
    torch.cuda.synchronize()
    for st, c in out.values():
        M._CONTEXTS.pop((0, st.cuda_stream), None)
        c.close()


def forward_everywhere(contexts, net, batch):
    """regime -> (scores, taps) of one forward per context, with the launches checked against the table."""
    out = {}
    for name, (st, c) in contexts.items():
        with torch.cuda.stream(st):
            _, s = P.run(net, batch)
            c.check_errors(st.cuda_stream)
            assert launched(c, *REGIMES[name]) == geometry(name), name
            out[name] = (s.cpu().numpy().copy(), {t: P.get_feature(t, c) for t in TAPS})
    return out


def test_every_geometry_is_launched(contexts, net):
    """The table, layer by layer and regime by regime; all six wide layers seen with one AND with two column tiles per wave."""
    batch = I.scenes()["units_l3"]
    seen, ways = {}, set()
    for name, (st, c) in contexts.items():
        with torch.cuda.stream(st):
            P.run(net, batch)
            got, want = launched(c, *REGIMES[name]), geometry(name)
            for layer in want:
                assert got[layer] == want[layer], (name, layer, got[layer], want[layer])
                seen.setdefault(layer, set()).add(got[layer][1])
            ways |= {got[f"{b}.0.conv1"][5] for b in WIDE}
    for b in WIDE:
        for cv in ("conv1", "conv2"):
            assert seen[f"{b}.0.{cv}"] == {1, 2}, (b, cv, seen[f"{b}.0.{cv}"])
    assert ways == {64, 128, 256}                          # ... and the balanced order with every tier size


SCENES = I.scenes()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scene_in_every_geometry(contexts, net, params, name):
    batch = SCENES[name]
    assert len(batch) <= 4200
    oracle = O.sps_forward(params, batch[:, :5], I.VS, keep=True)
    cm = oracle[1]["cm"]
    facts = I.tile_facts(batch, cm)
    out = forward_everywhere(contexts, net, batch)
    # --- the same bits whatever was launched, and again on a second forward
    s0, f0 = out["cap8k"]
    assert np.isfinite(s0).all()
    for regime, (s, f) in out.items():
        np.testing.assert_array_equal(s, s0, err_msg=regime)
        for t in TAPS:
            np.testing.assert_array_equal(f[t], f0[t], err_msg=f"{regime} {t}")
    again = forward_everywhere(contexts, net, batch)
    for regime, (s, f) in again.items():
        np.testing.assert_array_equal(s, s0, err_msg=f"second forward, {regime}")
        np.testing.assert_array_equal(f["block7"], f0["block7"], err_msg=f"second forward, {regime}")
    # --- every block against float64, from the device's own upstream taps (rows in the oracle's order).  Before the
    # comparison with the oracle: its 2e-4 must not be what stops a wrong kernel first
    st, c = contexts["cap512k"]
    with torch.cuda.stream(st):
        counts = c.level_counts()
        perm = [P.match_rows(P.get_voxels(l, counts[l], c), cm.coords[1 << l]) for l in range(5)]
    inv = [np.argsort(p) for p in perm]
    taps0 = {t: f0[t][inv[P.TAP_LEVEL[t]]] for t in TAPS}
    for block in R.BLOCKS:
        ref = R.block_from_taps(params, cm, taps0, block, np.float64)
        spread = R.spread(params, cm, taps0, block, ref)
        bound = R.bound(spread, ref)
        # (the five contexts hold the same bits, asserted above: one figure stands for all of them)
        errs = {regime: float(np.abs(f[block][inv[P.TAP_LEVEL[block]]].astype(np.float64) - ref).max()) for regime, (_, f) in out.items()}
        err = max(errs.values())
        ratio = f"{err / spread:6.2f}" if spread > 0 else "   inf" if err > 0 else "     -"
        print(f"{name:12s} {block}: spread {spread:.3e}  device error {err:.3e} (all {len(errs)} contexts: "
              f"{'the same' if len(set(errs.values())) == 1 else sorted(errs.items())})  ratio {ratio}  bound {bound:.3e}  "
              f"max|ref| {np.abs(ref).max():.3f}")                                     # (pytest -s shows the lines)
        for regime, e in errs.items():
            assert e <= bound, (name, regime, block, e, spread, bound)
    # --- the oracle, with one and with two column tiles per wave in all six wide layers
    for regime in ("cap8k", "cap512k"):
        st, c = contexts[regime]
        with torch.cuda.stream(st):
            P.check_full(net, params, batch, c=c, oracle=oracle)
            assert launched(c, *REGIMES[regime]) == geometry(regime)
    # --- what the kernels walked: present offsets and child octants per tile, from the device's own maps
    st, c = contexts["cap512k"]
    with torch.cuda.stream(st):
        for l in I.LEVELS:
            assert counts[l] == facts[l]["rows"]
            nt = (counts[l] + 15) // 16
            pad = nt * 16 - counts[l]
            pres = np.pad(c.kernel_map(l, 0).cpu().numpy() >= 0, ((0, 0), (0, pad))).reshape(81, nt, 16).any(2)
            np.testing.assert_array_equal(pres.T, facts[l]["pres"], err_msg=f"present offsets per tile, level {l}")
            kids = np.pad(c.kernel_map(5 + l, 0).cpu().numpy() >= 0, ((0, 0), (0, pad))).reshape(8, nt, 16).any(2)
            np.testing.assert_array_equal((kids * (1 << np.arange(8))[:, None]).sum(0), facts[l]["omask"],
                                          err_msg=f"child octants per tile, level {l}")
