"""Deterministic SPCTReg weights for the LTS tests: integer hash -> float64 -> float32, no RNG and no transcendental,
so every machine builds the same bits.  Scales keep the activations O(1); convs.bias puts the scores of the synthetic
frames of ``lts_cloud`` on both sides of epsilon_1 = 0.84."""
from __future__ import annotations

import numpy as np
import torch

M64 = (1 << 64) - 1
HEAD_BIAS = {"hdl-32": 4.2, "vlp-16": 5.25}   # calibrated once on lts_cloud(lidar, 3): about a third of the scores >= 0.84


def _hash_uniform(seed: int, n: int) -> np.ndarray:
    """n values in [-1, 1): splitmix64 of (seed, index), top 53 bits."""
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) + np.uint64((seed * 0x9E3779B97F4A7C15) & M64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * (2.0 / 2.0 ** 53) - 1.0


def _isqrt(k: int) -> float:
    """sqrt(1 / k) for the fan-ins used here, written out (no transcendental)."""
    return {3: 0.5773502691896258, 128: 0.08838834764831845, 512: 0.04419417382415922,
            2048: 0.02209708691207961, 6144: 0.012757759685074, 256: 0.0625}[k]


def lts_state_dict(seed: int = 1, head_bias: float = HEAD_BIAS["hdl-32"], qk_differ: bool = False,
                   qk_gain: float = 0.35, linear1_bn_bias_override: dict[int, float] | None = None) -> dict:
    """Full SPCTReg state_dict (reference keys and order).  qk_differ: q_conv.weight gets its own values (a checkpoint
    whose shared q / k Parameter was written twice with different values; the reference loads the k_conv one).
    qk_gain: scale of the q / k kernels (the energies grow with its square: a larger gain peaks the softmax).
    linear1_bn_bias_override: {channel: value} written over linear1's BN beta (channels whose pool is all negative).
    The defaults give the bits tests/golden/lts_forward.npz was captured with (tests/test_lts_cpu.py pins them)."""
    from sps_amd.models.lts import SPCTReg
    keys = SPCTReg().state_dict()
    sd = {}
    for i, (name, t) in enumerate(keys.items()):
        shape = tuple(t.shape)
        n = int(np.prod(shape)) if shape else 1
        u = _hash_uniform(seed * 1000 + i + (500 if qk_differ and ".q_conv." in name else 0), n)
        if name.endswith("num_batches_tracked"):
            sd[name] = torch.tensor(0, dtype=torch.long)
            continue
        if name.endswith("running_var"):
            v = 1.0 + 0.5 * u
            if name.startswith("embedding.bn1"):
                v = v * 100.0                          # the raw coordinates are metres
        elif name.endswith("running_mean"):
            v = 0.1 * u
        elif name.endswith(".weight") and len(shape) == 1:   # BN gamma
            v = 1.0 + 0.25 * u
        elif name.endswith(".bias"):
            v = 0.1 * u
            if name == "convs.bias":
                v = np.full(n, head_bias)
        else:                                          # conv kernel [out, in, 1]
            gain = 1.7320508075688772 * _isqrt(shape[1])  # uniform with unit variance gain
            if ".q_conv." in name or ".k_conv." in name:
                gain *= qk_gain                        # 0.35: energies O(1..10), a non-degenerate softmax
            if name == "convs.weight":
                gain *= 4.0
            v = u * gain
        if name == "linear1.1.bias" and linear1_bn_bias_override:
            for ch, val in linear1_bn_bias_override.items():
                v[ch] = val
        sd[name] = torch.from_numpy(v.astype(np.float32).reshape(shape))
    return sd


def lts_cloud(lidar: str, seed: int, n_rays: int = 20000, centred: bool = True, dup: float = 0.1,
              drop: float = 0.05) -> np.ndarray:
    """Synthetic frame [n, 4] (x, y, z, s).  centred: directions at cell centres (no binning ambiguity); duplicates
    of whole rows, same-cell collisions (same direction, other range / label), s == -1 rows, negative azimuths and,
    for hdl-32, elevations below -10 deg that wrap (Python negative row index)."""
    from tests.lts_reference import LIDARS, SLICES
    beams, up, down, _ = LIDARS[lidar]
    u = (_hash_uniform(seed, 6 * n_rays).reshape(6, n_rays) + 1.0) / 2.0     # [0, 1)
    res = (up - down) / (beams - 1)
    lo = -beams if lidar == "hdl-32" else 0           # hdl-32: negative rows too (wrap)
    if centred:
        row = np.floor(lo + u[0] * (beams - lo)) + 0.5
        col = np.floor(u[1] * SLICES) - SLICES / 2 + 0.5
    else:
        row = lo + u[0] * (beams - lo) * 0.9999
        col = u[1] * SLICES - SLICES / 2
    elev = np.deg2rad(down + row * res)
    azim = np.deg2rad(col * 360.0 / SLICES)
    rng = 2.0 + 40.0 * u[2]
    pts = np.c_[rng * np.cos(elev) * np.cos(azim), rng * np.cos(elev) * np.sin(azim), rng * np.sin(elev), u[3]]
    pts[u[4] < drop, 3] = -1.0
    k = int(dup * n_rays)
    pts = np.r_[pts, pts[:k]]                        # exact duplicates
    near = pts[k: 2 * k].copy()
    near[:, :3] *= 0.97                              # same direction, other range: same cell
    near[:, 3] = u[5][:k]
    return np.r_[pts, near].astype(np.float32)


_WINDOWS = {}


def lts_inputs(B: int, N: int) -> np.ndarray:
    """Network input [B, 3, N]: the 16 windows of one projected hdl-32 frame and their point-reversed copies, cut to
    B windows of N points (the input of the forward tests).  N > 2048: window b continues with the points of window
    b - 1."""
    from tests.lts_reference import lts_project, lts_windows
    if "x" not in _WINDOWS:
        fr, _ = lts_project(lts_cloud("hdl-32", 50, n_rays=60000), "hdl-32")
        x, _ = lts_windows(fr, "hdl-32")                              # [16, 3, 2048]
        xx = np.concatenate([x, x[:, :, ::-1]], axis=0)
        _WINDOWS["x"] = np.concatenate([xx, np.roll(xx, 1, axis=0)], axis=2)
    return np.ascontiguousarray(_WINDOWS["x"][:B, :, :N])


# ---- the edge tests' models and inputs (tests/test_hip_lts_edges.py; the conditions they rest on are asserted on the
# f64 restatement by tests/test_lts_cpu.py) ----------------------------------------------------------------------------
PEAKED_K = 4                                  # qk_gain = 0.35 * PEAKED_K: the smallest integer multiple that peaks the softmax
PEAKED_QK_GAIN = 0.35 * PEAKED_K
PEAKED_SHAPE = (2, 1000)                      # (B, N) of the peaked-softmax inputs
NEG_POOL_CHANNELS = (0, 31, 32, 127, 128, 1023, 2047)   # first / last column of a lane group, a wave, a 128-tile, the tensor
NEG_POOL_BIAS = -20.0                         # linear1's BN beta there: every pre-activation of these channels < -1
NEG_POOL_SHAPES = ((2, 1), (2, 129), (2, 1000))


def lts_dup_inputs() -> np.ndarray:
    """PEAKED_SHAPE input whose windows are half one point repeated (identical q rows: energies that tie exactly, as the
    duplicated cells of a real projection give) and half spread points; the repeated half leads in window 0 and trails
    in window 1."""
    B, N = PEAKED_SHAPE
    x = lts_inputs(B, N).copy()
    for b in range(B):
        p = x[b][:, np.flatnonzero(np.any(x[b] != 0, axis=0))[7]].copy()     # a measured point, not an empty cell
        x[b][:, lts_dup_rows(b)] = p[:, None]
    return x


def lts_dup_rows(b: int) -> slice:
    """The repeated half of window b of lts_dup_inputs()."""
    N = PEAKED_SHAPE[1]
    return slice(0, N // 2) if b == 0 else slice(N // 2, N)
