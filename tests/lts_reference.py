"""Independent restatement of the LTS baseline (reference c_ws/src/inference_model/lts_filter/scripts/) in plain
numpy / torch: the checker of the HIP path (sps_amd/models/lts.py, sps_amd/datasets/lts_loader.py, sps_amd/lts_filter.py).

  lts_project(data, lidar)   range image [beams, 1024, 4] (+ the pre-floor row / column values of every kept row)
  lts_windows(frame, lidar)  network input [windows, 3, N] and cell labels [windows, N]
  lts_forward(sd, x, dtype)  SPCTReg scores [B, N] and taps, in float32 or float64, on the given device
  lts_metrics(scores, labels, eps)   the node's loss / R2 / calculate_metrics
"""
from __future__ import annotations

import numpy as np
import torch

LIDARS = {  # beams, fov up / down (degrees), window size
    "vlp-16": (16, 16.8, -16.8, 128),
    "hdl-32": (32, 30, -10, 64),
}
SLICES = 1024


def lidar_dims(lidar):
    beams, _, _, w = LIDARS[lidar]
    return beams, w, SLICES // w, beams * w


def lts_project(data, lidar):
    """Per cell, the lexicographically largest (x, y, z, s) among the rows with s != -1 that fall in it; angles in
    float32 with numpy's order of operations.  Returns (frame, pre) with pre = float64 [m, 2] pre-floor (row, column)
    values of every kept row (for boundary tolerance).  Raises IndexError like the reference."""
    beams, up, down, _ = LIDARS[lidar]
    d = np.asarray(data, dtype=np.float32)[:, :4]
    d = d[d[:, 3] != np.float32(-1)]
    x, y, z, s = (d[:, k] for k in range(4))
    if np.isnan(d[:, :3]).any():
        raise IndexError("NaN coordinate")
    f180, fpi = np.float32(180), np.float32(np.pi)
    elev = np.arctan2(z, np.sqrt(x * x + y * y)) * f180 / fpi
    azim = np.arctan2(y, x) * f180 / fpi
    row_f = (elev - np.float32(down)) / np.float32((up - down) / (beams - 1))
    col_f = azim / np.float32(360 / SLICES)
    row = np.floor(row_f).astype(np.int64)
    col = np.floor(col_f).astype(np.int64)
    if ((row < -beams) | (row >= beams)).any() or ((col < -SLICES) | (col >= SLICES)).any():
        raise IndexError("row index outside the image")
    row %= beams
    col %= SLICES
    frame = np.zeros((beams, SLICES, 4), np.float32)
    cell = row * SLICES + col
    order = np.lexsort((s, z, y, x, cell))            # by cell, then x, y, z, s ascending: the last of a cell wins
    last = np.ones(len(order), bool)
    last[:-1] = cell[order][1:] != cell[order][:-1]
    win = order[last]
    frame.reshape(-1, 4)[cell[win]] = d[win]
    return frame, np.c_[row_f, col_f].astype(np.float64)


def lts_windows(frame, lidar):
    beams, w, nw, N = lidar_dims(lidar)
    win = frame.reshape(beams, nw, w, 4).transpose(1, 0, 2, 3).reshape(nw, N, 4)
    return np.ascontiguousarray(win[:, :, :3].transpose(0, 2, 1)), np.ascontiguousarray(win[:, :, 3])


def _bn(sd, p, x, dt):
    g, b, m, v = (sd[f"{p}.{k}"].to(device=x.device, dtype=dt) for k in ("weight", "bias", "running_mean", "running_var"))
    return (x - m[:, None]) / torch.sqrt(v[:, None] + 1e-5) * g[:, None] + b[:, None]


def _conv(sd, p, x, dt, bias=True):
    W = sd[f"{p}.weight"].to(device=x.device, dtype=dt)[:, :, 0]
    y = torch.einsum("oc,cn->on", W, x)
    if bias and f"{p}.bias" in sd:
        y = y + sd[f"{p}.bias"].to(device=x.device, dtype=dt)[:, None]
    return y


def _window(sd, x, dt, probes=False):
    """One window x [3, N] -> (scores [N], taps).  probes: the taps also hold, per attention layer k, the energies
    ``energy{k}`` [query, key] and the key columns' sums over the queries ``colsum{k}`` [key], and linear1's
    pre-activation ``linear1_pre`` [2048, N] (what the edge tests state their conditions on)."""
    taps = {}
    h = torch.relu(_bn(sd, "embedding.bn1", _conv(sd, "embedding.conv1", x, dt), dt))
    h = torch.relu(_bn(sd, "embedding.bn2", _conv(sd, "embedding.conv2", h, dt), dt))
    taps["embedding"] = h
    outs = []
    for k in range(1, 5):
        p = f"sa{k}"
        q = _conv(sd, f"{p}.k_conv", h, dt)           # the shared q / k weight (k_conv's value after a load)
        energy = q.t() @ q                            # [query, key]
        att = torch.softmax(energy, dim=1)            # over keys
        if probes:
            taps[f"energy{k}"], taps[f"colsum{k}"] = energy, att.sum(dim=0)
        att = att / (1e-9 + att.sum(dim=0, keepdim=True))   # each key column over its queries
        v = _conv(sd, f"{p}.v_conv", h, dt)
        xr = v @ att
        h = h + torch.relu(_bn(sd, f"{p}.after_norm", _conv(sd, f"{p}.trans_conv", h - xr, dt), dt))
        taps[p] = h
        outs.append(h)
    y = _bn(sd, "linear1.1", _conv(sd, "linear1.0", torch.cat(outs, 0), dt, bias=False), dt)
    if probes:
        taps["linear1_pre"] = y
    y = torch.nn.functional.leaky_relu(y, 0.2)
    mx, mean = y.max(dim=1).values, y.mean(dim=1)
    taps["max"], taps["mean"] = mx, mean
    N = y.shape[1]
    y = torch.cat([y, mx[:, None].expand(-1, N), mean[:, None].expand(-1, N)], 0)
    y = torch.nn.functional.silu(_bn(sd, "linear2.1", _conv(sd, "linear2.0", y, dt), dt))
    y = torch.nn.functional.silu(_bn(sd, "linear3.1", _conv(sd, "linear3.0", y, dt), dt))
    return torch.sigmoid(_conv(sd, "convs", y, dt))[0], taps


@torch.no_grad()
def lts_forward(sd, x, dtype=torch.float64, device=None, probes=False):
    """x [B, 3, N] -> scores [B, N] (numpy, dtype) and taps {name: [B, ...]} (numpy; probes: see _window)."""
    xt = torch.as_tensor(np.asarray(x)).to(device=device or "cpu", dtype=dtype)
    scores, taps = [], {}
    for b in range(xt.shape[0]):
        s, t = _window(sd, xt[b], dtype, probes)
        scores.append(s.cpu().numpy())
        for k, v in t.items():
            taps.setdefault(k, []).append(v.cpu().numpy())
    return np.stack(scores), {k: np.stack(v) for k, v in taps.items()}


def lts_metrics(scores, labels, eps=0.84):
    """stability_filter.py:167-182: MSELoss, R2Score, calculate_metrics(gt, pred) with both thresholded (< eps -> 0)."""
    s = np.asarray(scores, np.float64).reshape(-1)
    g = np.asarray(labels, np.float64).reshape(-1)
    e = np.float32(eps)
    pred = np.asarray(scores, np.float32).reshape(-1) >= e
    gt = np.asarray(labels, np.float32).reshape(-1) >= e
    tp, fp = float(np.sum(pred & gt)), float(np.sum(pred & ~gt))
    fn, tn = float(np.sum(~pred & gt)), float(np.sum(~pred & ~gt))
    loss = float(np.mean((s - g) ** 2))
    r2 = float(1 - np.sum((s - g) ** 2) / np.sum((g - g.mean()) ** 2))
    precision = tp / (tp + fp) if tp + fp else 0
    recall = tp / (tp + fn) if tp + fn else 0
    f1 = 2 * precision * recall / (precision + recall) if precision + recall else 0
    return dict(loss=loss, r2=r2, precision=precision, recall=recall, f1=f1, accuracy=(tp + tn) / (tp + tn + fp + fn),
                dIoU=tp / (tp + fn + fp) if tp + fn + fp else float("nan"), tp=tp, fp=fp, fn=fn, tn=tn)
