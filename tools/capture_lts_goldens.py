#!/usr/bin/env python3
"""Capture golden vectors of the LTS baseline from the REFERENCE python (c_ws/src/inference_model/lts_filter/scripts:
loader.py and transformer.py, both pure numpy / PyTorch) for tests/test_lts_cpu.py and tests/test_hip_lts.py.
Runs only where the reference tree exists (its lts_filter/scripts directory as the first argument or in
$LTS_REFERENCE); writes tests/golden/lts_*.npz (data only: clouds, cells, key lists,
scores, taps).

  lts_proj_<case>.npz  a synthetic frame (tests/lts_weights.lts_cloud) and, per occupied cell, the row the reference
                       Loader keeps; lts_proj_errors.npz: frames the reference rejects with IndexError
  lts_keys.npz         the reference SPCTReg state_dict keys and shapes
  lts_forward.npz      the reference SPCTReg on 2 windows with tests/lts_weights: scores, taps (every 128th point),
                       linear1 max / mean, and the scores of a checkpoint whose q_conv and k_conv values differ
"""
import os
import sys

import numpy as np
import torch

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LTS_REFERENCE", "")
if not os.path.exists(os.path.join(REF, "transformer.py")):
    raise SystemExit("usage: capture_lts_goldens.py <reference>/c_ws/src/inference_model/lts_filter/scripts")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

import loader as ref_loader  # noqa: E402
import transformer as ref_transformer  # noqa: E402

from tests.lts_weights import HEAD_BIAS, lts_cloud, lts_state_dict  # noqa: E402

STRIDE = 128   # tap columns kept


def proj_case(name, lidar, cloud):
    frame = ref_loader.Loader(cloud, lidar).frame
    flat = frame.reshape(-1, 4)
    cells = np.flatnonzero(np.any(flat != 0, axis=1)).astype(np.int32)
    np.savez_compressed(os.path.join(OUT, f"lts_proj_{name}.npz"), lidar=np.array(lidar), cloud=cloud, cells=cells,
                        rows=flat[cells])
    print(name, lidar, len(cloud), "rows,", len(cells), "cells")
    return frame


def main():
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(8)
    frames = {}
    frames["hdl32"] = proj_case("hdl32", "hdl-32", lts_cloud("hdl-32", 11, n_rays=1500))
    proj_case("vlp16", "vlp-16", lts_cloud("vlp-16", 12, n_rays=1500))
    proj_case("hdl32_random", "hdl-32", lts_cloud("hdl-32", 13, n_rays=1500, centred=False))
    # rejected frames: elevation above the top row, far below the wrap range, a NaN coordinate
    base = lts_cloud("hdl-32", 14, n_rays=50)
    bad = []
    for p in ([10.0, 0.0, 12.0, 0.5], [10.0, 0.0, -30.0, 0.5], [np.nan, 1.0, 0.0, 0.5]):
        c = np.r_[base, np.array([p], np.float32)]
        try:
            ref_loader.Loader(c, "hdl-32")
            raise SystemExit(f"the reference accepted {p}")
        except IndexError:
            bad.append(c)
    # ... while an out-of-image point with s == -1 is dropped before it is indexed
    ok = np.r_[base, np.array([[10.0, 0.0, 12.0, -1.0]], np.float32)]
    ref_loader.Loader(ok, "hdl-32")
    np.savez_compressed(os.path.join(OUT, "lts_proj_errors.npz"), bad=np.stack(bad), dropped_ok=ok)

    model = ref_transformer.SPCTReg().eval()
    sd = model.state_dict()
    np.savez_compressed(os.path.join(OUT, "lts_keys.npz"), keys=np.array(list(sd)),
                        shapes=np.array([list(v.shape) + [-1] * (3 - v.dim()) for v in sd.values()], np.int64))

    fr = frames["hdl32"]
    win = [fr[:, w * 64:(w + 1) * 64].reshape(-1, 4) for w in (0, 7)]
    x = np.stack([w[:, :3].T for w in win]).astype(np.float32)         # [2, 3, 2048]
    model.load_state_dict(lts_state_dict(head_bias=HEAD_BIAS["hdl-32"]))
    taps = {}

    def hook(name):
        def f(_m, _i, out):
            taps[name] = out.detach().clone()
        return f

    for name in ("embedding", "sa1", "sa2", "sa3", "sa4", "linear1"):
        getattr(model, name).register_forward_hook(hook(name))
    with torch.no_grad():
        scores = model(torch.from_numpy(x))[:, 0].numpy()
    l1 = taps.pop("linear1")
    model2 = ref_transformer.SPCTReg().eval()
    model2.load_state_dict(lts_state_dict(head_bias=HEAD_BIAS["hdl-32"], qk_differ=True))
    with torch.no_grad():
        scores_qk = model2(torch.from_numpy(x))[:, 0].numpy()
    out = dict(x=x, scores=scores, scores_qk=scores_qk, tap_stride=np.int32(STRIDE),
               tap_max=l1.max(dim=-1)[0].numpy(), tap_mean=l1.mean(dim=-1).numpy())
    for k, v in taps.items():
        out[f"tap_{k}"] = v[:, :, ::STRIDE].numpy()
    np.savez_compressed(os.path.join(OUT, "lts_forward.npz"), **out)
    print("forward: scores in", scores.min(), scores.max(), "frac >= 0.84:", float((scores >= 0.84).mean()))
    for f in sorted(os.listdir(OUT)):
        if f.startswith("lts_"):
            print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


if __name__ == "__main__":
    main()
