"""GPU edge tests of the training backward (sps_train_forward / sps_train_backward behind SPSNet in train mode) on the scenes,
cotangents, capacities and tolerance of tests/train_edge_inputs.py: arbitrary cotangents against the float64 autograd
oracle, the same gradients under three launch plans of the weight gradients, neighbour tables dirtied by a larger forward,
a cotangent on out-of-range rows only, linearity and the fixed-point head, and cotangents the head cannot hold.

Every test runs on torch streams of its own: a native context belongs to a (device, stream), its capacity never shrinks and
decides the summation order of the weight gradients, so the contexts of the other test files are left as they are."""
import numpy as np
import pytest
import torch

from tests import train_edge_inputs as TE
from tests.helpers import net_from_params

pytestmark = pytest.mark.gpu


class Rig:
    """a stream, its native context reserved for `cap` rows, and a network in train mode whose tensors live on that stream"""

    def __init__(self, cap, params=None):
        from sps_amd.models.models import get_context
        self.stream = torch.cuda.Stream()
        self.ctx = get_context(0, self.stream.cuda_stream)
        self.ctx.reserve(cap)
        with torch.cuda.stream(self.stream):
            self.net = net_from_params(TE.params() if params is None else params).cuda().train()

    def close(self):
        from sps_amd.models import models as M
        self.stream.synchronize()
        M._CONTEXTS.pop((0, int(self.stream.cuda_stream)), None)
        self.ctx.close()

    def inverse(self, n):
        from sps_amd import _native
        inv = torch.empty(n, dtype=torch.int64, device="cuda")
        _native.check(_native.lib.sps_get_inverse(self.ctx.handle, inv.data_ptr()))
        return inv.cpu().numpy()

    def check(self):
        self.ctx.check_errors(self.stream.cuda_stream)

    def step(self, batch, cot, expect_range_error=False):
        """train-mode forward, scores.backward(cot) -- cot [N] or a function of the device's inverse map.
        -> (scores, gradients name -> array, cot)"""
        from sps_amd._native import ERR_RANGE, SpsError
        with torch.cuda.stream(self.stream):
            self.net.zero_grad(set_to_none=True)
            scores = self.net(torch.from_numpy(np.array(batch, dtype=np.float32)).cuda())
            if expect_range_error:                              # the forward flags the out-of-range rows: consume that flag
                with pytest.raises(SpsError) as e:
                    self.check()
                assert e.value.code == ERR_RANGE
            g = cot(self.inverse(len(batch))) if callable(cot) else cot
            scores.backward(torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32)).cuda())
            self.stream.synchronize()
            grads = {k.replace("model.MinkUNet.", ""): p.grad.detach().cpu().numpy().copy() for k, p in self.net.named_parameters()}
            return scores.detach().cpu().numpy(), grads, g


@pytest.fixture(scope="module")
def rigs():
    made = {}

    def get(key, cap):
        if key not in made:
            made[key] = Rig(cap)
        return made[key]

    yield get
    for r in made.values():
        r.close()


def assert_plan(rig, cap):
    """the device's (gshift, nwg) of every k_wgrad job are what TE.plan derives for the capacity the test chose"""
    got = {name: rig.ctx.train_wgrad_plan(name) for name, *_ in TE.WG_LAYERS}
    assert got == TE.plan(cap), {k: (v, TE.plan(cap)[k]) for k, v in got.items() if v != TE.plan(cap)[k]}


def run_pair(rig, case, cot):
    batch = TE.case(case)
    bad = ~TE.in_range(batch)
    scores, grads, g = rig.step(batch, lambda inv: TE.cotangent(case, cot, inv), expect_range_error=bool(bad.any()))
    rig.check()                                                 # a valid step leaves no flag behind
    return batch, bad, scores, grads, g


def assert_matches_oracle(case, cot, tag, batch, bad, scores, grads, g):
    """scores and every gradient within 16 x max(e32, 1e-6) of the float64 oracle, relative to the tensor's maximum; every
    figure is printed first (profiles/train_edges/ is made of them)"""
    ref = TE.reference(case, g)
    assert np.isnan(scores[bad]).all() and np.isfinite(scores[~bad]).all()
    es = TE.rel_err(scores[~bad], ref["s64"][~bad])
    print(f"EDGE {case} {cot} {tag} scores dev={es:.3e} e32={ref['e32_scores']:.3e} ratio={es / max(ref['e32_scores'], TE.FLOOR):.2f}")
    assert set(grads) == set(ref["g64"])
    ok, over = TE.allowed(ref["e32"]), {}
    for name, want in ref["g64"].items():
        assert np.isfinite(grads[name]).all(), name
        err = TE.rel_err(grads[name], want)
        print(f"EDGE {case} {cot} {tag} {name} dev={err:.3e} e32={ref['e32'][name]:.3e} ratio={err / max(ref['e32'][name], TE.FLOOR):.2f}")
        if err > ok[name]:
            over[name] = (err, ok[name])
    assert es <= TE.allowed(ref["e32_scores"]), (es, ref["e32_scores"])
    assert not over, f"gradients beyond 16 x the float32 oracle's own error (relative to the tensor's max): {over}"
    return ref


# ---- 1. gradients against the oracle, every layer on the (gshift 4, nwg 1) plan ---------------------------------------------
@pytest.mark.parametrize("case,cot", TE.PAIRS)
def test_gradients_match_the_oracle(rigs, case, cot):
    rig = rigs("min", TE.CAP_MIN)
    out = run_pair(rig, case, cot)
    assert tuple(rig.ctx.level_counts()) == TE.CASES[case][1]
    assert_plan(rig, TE.CAP_MIN)
    ref = assert_matches_oracle(case, cot, TE.CAP_MIN, *out)
    if cot != "off_range_only":
        assert max(np.abs(v).max() for v in ref["g64"].values()) > 0


# ---- 2. the same gradients under the two other plans ------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [TE.CAP_MIXED, TE.CAP_WIDE])
@pytest.mark.parametrize("case", TE.PLAN_CASES)
def test_gradients_under_the_other_plans(rigs, case, cap):
    small, rig = rigs("min", TE.CAP_MIN), rigs(cap, cap)
    assert rig.ctx.arena_bytes() > small.ctx.arena_bytes()      # the reservation took effect
    for cot in ("mse", "random"):
        out = run_pair(rig, case, cot)
        assert_plan(rig, cap)
        assert_matches_oracle(case, cot, cap, *out)
        again = run_pair(rig, case, cot)
        for name in out[3]:
            np.testing.assert_array_equal(out[3][name], again[3][name], err_msg=name)      # fixed order: the same bits
        np.testing.assert_array_equal(out[2], again[2])


# ---- 3. neighbour tables a larger forward has written all over ---------------------------------------------------------------
@pytest.mark.parametrize("case", ["dust", "tile17"])
def test_stale_table_entries_are_not_read(rigs, case):
    """The map kernels leave the entries of a (tile, offset) without pairs unwritten.  Context A has run a 4000-row scene
    before the sparse one, context B (the same capacity) has not: bit-equal gradients."""
    big = TE.case("big")
    cap = (len(big) + 1023) // 1024 * 1024
    a, b = rigs("stale_a", cap), rigs("stale_b", cap)
    _, gbig, _ = a.step(big, np.random.default_rng(1).standard_normal(len(big)).astype(np.float32))
    a.check()
    assert_plan(a, cap)
    assert a.ctx.level_counts()[0] > 3000 and all(np.isfinite(v).all() for v in gbig.values())
    batch = TE.case(case)
    g = TE.cotangent(case, "random")
    sa, ga, _ = a.step(batch, g)
    sb, gb, _ = b.step(batch, g)
    a.check()
    b.check()
    np.testing.assert_array_equal(sa, sb)
    assert max(np.abs(v).max() for v in ga.values()) > 0
    for name in ga:
        np.testing.assert_array_equal(ga[name], gb[name], err_msg=name)


# ---- 4. a cotangent on rows without a voxel -----------------------------------------------------------------------------------
def test_cotangent_on_out_of_range_rows_only_gives_exact_zeros(rigs):
    _, bad, scores, grads, g = run_pair(rigs("min", TE.CAP_MIN), "off_range", "off_range_only")
    assert np.all(g[bad] != 0) and np.all(g[~bad] == 0) and np.isnan(scores[bad]).all()
    for name, v in grads.items():
        assert np.isfinite(v).all() and np.all(v == 0.0), name


# ---- 5. linearity, and the fixed-point head seen alone through final.bias -----------------------------------------------------
@pytest.mark.parametrize("case", TE.ADDITIVE_CASES)
def test_backward_is_additive(rigs, case):
    """backward(g1 + g2) against backward(g1) + backward(g2), within the tolerance of the summed cotangent's oracle and
    relative to the maximum of the sum's gradient, as everywhere"""
    rig, batch = rigs("min", TE.CAP_MIN), TE.case(case)
    g1, g2, both = TE.additive_parts(case)
    _, ga, _ = rig.step(batch, g1)
    _, gb, _ = rig.step(batch, g2)
    _, gs, _ = rig.step(batch, both)
    rig.check()
    ref = TE.reference(case, both)
    ok = TE.allowed(ref["e32"])
    over = {}
    for name in gs:
        err = TE.rel_err(ga[name].astype(np.float64) + gb[name], gs[name].astype(np.float64))
        print(f"EDGE {case} additive {TE.CAP_MIN} {name} dev={err:.3e} e32={ref['e32'][name]:.3e} ratio={err / max(ref['e32'][name], TE.FLOOR):.2f}")
        if err > ok[name]:
            over[name] = (err, ok[name])
    assert not over, over


def head_bias_gradient(g, scores):
    """sum_p g_p s_p (1 - s_p) as k_dlogit_accum forms its terms: float64 products of the float32 cotangent, the float32
    score and the float32 difference 1 - s; the sum exact (math.fsum)"""
    import math
    s = scores.astype(np.float32)
    t = g.astype(np.float32).astype(np.float64) * s.astype(np.float64) * (np.float32(1.0) - s).astype(np.float64)
    return math.fsum(t[np.isfinite(t)])


@pytest.mark.parametrize("case", ["dupes", "brick", "off_range"])
def test_head_is_homogeneous_within_its_fixed_point_resolution(rigs, case):
    """final.bias' gradient is the sum of the per-voxel 32.32 accumulators: every term is rounded to 2^-32 (error <= 2^-33),
    the integer sums are exact, their float64 sum is exact, and the result is rounded to float32 once.  So
    |db - sum_p g_p s_p (1 - s_p)| <= N 2^-33 + one float32 ulp of the result, at every scale of the cotangent."""
    rig, batch = rigs("min", TE.CAP_MIN), TE.case(case)
    bad = ~TE.in_range(batch)
    base = TE.cotangent(case, "random")
    for scale in (1.0, 2.0 ** -10, 2.0 ** 10, 2.0 ** -20):
        g = (base * np.float32(scale)).astype(np.float32)          # exact: a power of two
        scores, grads, _ = rig.step(batch, g, expect_range_error=bool(bad.any()))
        rig.check()
        got = float(grads["final.bias"].reshape(-1)[0])
        want = head_bias_gradient(g[~bad], scores[~bad])
        bound = int((~bad).sum()) * 2.0 ** -33 + float(np.spacing(np.float32(abs(want))))
        print(f"EDGE head {case} scale={scale:g} db={got:.9e} want={want:.9e} |diff|={abs(got - want):.3e} bound={bound:.3e} "
              f"bound/|want|={bound / abs(want):.2e}")
        assert abs(got - want) <= bound, (scale, got, want, bound)


# ---- 6. cotangents the head cannot hold ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [float("nan"), float("inf"), -float("inf"), 1e6])
def test_bad_loss_gradient_is_reported_not_repaired(rigs, value):
    from sps_amd._native import ERR_INVALID, SpsError
    rig, batch = rigs("min", TE.CAP_MIN), TE.case("tile65")
    good = TE.cotangent("tile65", "random")
    _, clean, _ = rig.step(batch, good)
    rig.check()
    g = np.zeros(len(batch), dtype=np.float32)
    g[len(batch) // 2] = value
    rig.step(batch, g)
    with pytest.raises(SpsError) as e:
        rig.check()
    assert e.value.code == ERR_INVALID and "loss gradient" in str(e.value)
    rig.check()                                                 # reported once
    _, after, _ = rig.step(batch, good)                         # and the context trains normally afterwards
    rig.check()
    for name in clean:
        np.testing.assert_array_equal(clean[name], after[name], err_msg=name)


def test_a_term_of_exactly_2_to_15_is_held_and_the_next_float_is_not(rigs):
    """final.kernel = 0, final.bias = 0: every logit is 0 and every score exactly 0.5, so a cotangent of 131072 is a term of
    exactly 32768 = 2^15, the largest the 32.32 accumulator takes; the next float32 above it is reported."""
    from sps_amd._native import ERR_INVALID, SpsError
    params = dict(TE.params())
    params["final.kernel"] = np.zeros_like(params["final.kernel"])
    params["final.bias"] = np.zeros_like(params["final.bias"])
    rig = Rig(TE.CAP_MIN, params)
    try:
        batch = TE.case("tile17")
        for sign in (1.0, -1.0):
            g = np.zeros(len(batch), dtype=np.float32)
            g[3] = sign * 131072.0
            scores, grads, _ = rig.step(batch, g)
            assert np.all(scores == np.float32(0.5))
            rig.check()
            assert float(grads["final.bias"].reshape(-1)[0]) == sign * 32768.0
            g[3] = np.nextafter(np.float32(131072.0), np.float32(np.inf)) * np.float32(sign)
            rig.step(batch, g)
            with pytest.raises(SpsError) as e:
                rig.check()
            assert e.value.code == ERR_INVALID and "loss gradient" in str(e.value)
    finally:
        rig.close()
