#!/usr/bin/env python3
"""Per-frame time of the LTS baseline's SPCTReg on one MI355X: the HIP path (sps_amd.models.lts.SPCTReg, one
sps_lts_forward of all windows of a frame) against the same network written as eager f32 PyTorch on the same GPU
(batched bmm attention, the way the reference runs it).  hipEvent timing, median of --iters after --warmup.
Prints one line per (lidar, path) and a JSON summary line.

    python tools/lts_timing.py [--iters 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sps_amd.models.lts import SPCTReg  # noqa: E402
from tests.lts_reference import lts_project, lts_windows  # noqa: E402
from tests.lts_weights import HEAD_BIAS, lts_cloud, lts_state_dict  # noqa: E402

def flops(N):
    """Executed FLOP of one window (energy counted twice: pass A + pass B)."""
    gemm = 2 * N * (3 * 128 + 128 * 128 + 4 * (128 * 160 + 128 * 128) + 512 * 2048 + 2048 * 512 + 512 * 256 + 256)
    attn = 4 * (2 * 2 * N * N * 32 + 2 * N * N * 128)
    return gemm + attn


def eager(sd, x):
    """Eager f32 torch SPCTReg on [B, 3, N] (BN eval, dropout identity)."""
    g = {k: v.cuda().float() for k, v in sd.items()}

    def conv(p, h, bias=True):
        y = torch.einsum("oc,bcn->bon", g[p + ".weight"][:, :, 0], h)
        return y + g[p + ".bias"][None, :, None] if bias and p + ".bias" in g else y

    def bn(p, h):
        return (h - g[p + ".running_mean"][None, :, None]) / torch.sqrt(g[p + ".running_var"][None, :, None] + 1e-5) \
            * g[p + ".weight"][None, :, None] + g[p + ".bias"][None, :, None]

    h = torch.relu(bn("embedding.bn1", conv("embedding.conv1", x)))
    h = torch.relu(bn("embedding.bn2", conv("embedding.conv2", h)))
    outs = []
    for k in range(1, 5):
        p = f"sa{k}"
        q = conv(p + ".k_conv", h)
        a = torch.softmax(torch.bmm(q.transpose(1, 2), q), dim=-1)
        a = a / (1e-9 + a.sum(dim=1, keepdim=True))
        h = h + torch.relu(bn(p + ".after_norm", conv(p + ".trans_conv", h - torch.bmm(conv(p + ".v_conv", h), a))))
        outs.append(h)
    y = torch.nn.functional.leaky_relu(bn("linear1.1", conv("linear1.0", torch.cat(outs, 1), False)), 0.2)
    N = y.shape[2]
    y = torch.cat([y, y.max(dim=-1, keepdim=True)[0].expand(-1, -1, N), y.mean(dim=-1, keepdim=True).expand(-1, -1, N)], 1)
    y = torch.nn.functional.silu(bn("linear2.1", conv("linear2.0", y)))
    y = torch.nn.functional.silu(bn("linear3.1", conv("linear3.0", y)))
    return torch.sigmoid(conv("convs", y))


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    torch.backends.cuda.matmul.allow_tf32 = False
    out = {}
    for lidar in ("hdl-32", "vlp-16"):
        sd = lts_state_dict(head_bias=HEAD_BIAS[lidar])
        model = SPCTReg()
        model.load_state_dict(sd)
        model = model.cuda().eval()
        fr, _ = lts_project(lts_cloud(lidar, 7, n_rays=60000), lidar)
        x = torch.from_numpy(lts_windows(fr, lidar)[0]).cuda()
        B, _, N = x.shape
        with torch.no_grad():
            diff = float((model(x) - eager(sd, x)).abs().max())
            t_hip = timed(lambda: model(x), args.iters, args.warmup)
            t_eager = timed(lambda: eager(sd, x), args.iters, args.warmup)
        gf = B * flops(N) / 1e9
        out[lidar] = dict(windows=B, N=N, gflop=round(gf, 1), hip_ms=round(t_hip, 3), eager_ms=round(t_eager, 3),
                          speedup=round(t_eager / t_hip, 2), hip_tflops=round(gf / t_hip, 1),
                          floor_ms_155tf=round(gf / 155e3 * 1e3, 3), max_abs_diff=diff)
        print(f"{lidar}: {B} windows x N={N}  {gf:.1f} GFLOP  HIP {t_hip:.3f} ms ({gf / t_hip:.1f} TF/s)  "
              f"eager torch f32 {t_eager:.3f} ms  speedup {t_eager / t_hip:.2f}x  |HIP - eager| {diff:.2e}")
    print(json.dumps({"lts_timing": out, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
