"""Online LTS stability filter: the per-frame body of the reference's LTS node
(c_ws/src/inference_model/lts_filter/scripts/stability_filter.py:134-200, ``Stability.infer``) without ROS.

    range-image projection + windows (Loader, :137-160)  ->  SPCTReg forward (:163)  ->  MSE / R2 (:167-170)
    ->  calculate_metrics with prediction and ground truth thresholded at epsilon_1 (:178-182)
    ->  epsilon filter, keep (x, y, z, score) rows with score <= epsilon_1 (:196)

Every cell of the image is a point, empty cells included (zero points): they are scored, counted in the metrics and
kept by the filter when their score is <= epsilon_1, as in the reference.  ``submit()`` issues the whole frame on the
caller's stream without a host synchronisation (projection, forward, metric sums and the two compactions are
stream-ordered native calls; the row counts stay on the device); ``PendingLTS.result()`` is the one synchronisation
and raises IndexError for a frame with a point outside the image rows (or a NaN coordinate).  ``epsilon_0`` of the node
is read there and never used: it is not a parameter here.
"""
from __future__ import annotations

import time
from dataclasses import dataclass

import torch

from . import _native
from .models.models import _require_device_tensor, get_context, metrics_from_sums


@dataclass
class LTSResult:
    filtered: torch.Tensor     # [m, 4] (x, y, z, score) of the cells with score <= epsilon_1, window-major cell order
    scores: torch.Tensor       # [num_windows * N] score of every cell
    points: torch.Tensor       # [num_windows * N, 3] the cells' points (zeros for empty cells)
    labels: torch.Tensor       # [num_windows * N] the cells' s values
    loss: float                # nn.MSELoss(scores, labels)
    r2: float                  # torchmetrics R2Score
    dIoU: float
    precision: float
    recall: float
    F1: float
    accuracy: float
    counts: dict               # count, tp, fp, fn, tn
    t_total: float             # seconds: host wall time submit -> result
    t_project: float           # GPU seconds (hipEvents): projection
    t_infer: float             # GPU seconds: forward
    t_filter: float            # GPU seconds: metrics + epsilon filter


class PendingLTS:
    def __init__(self, owner, rows, scores, kept_xyz, kept_s, counts, sums, counts_host, sums_host, ev, stream, t0):
        self._o, self._rows, self._scores, self._kx, self._ks = owner, rows, scores, kept_xyz, kept_s
        self._counts, self._sums, self._counts_host, self._sums_host = counts, sums, counts_host, sums_host
        self._ev, self._stream, self._t0 = ev, stream, t0

    def result(self) -> LTSResult:
        self._stream.synchronize()                                           # the one host synchronisation
        self._o.handle.check_errors(self._stream.cuda_stream)                # IndexError of the reference
        n_keep = int(self._counts_host[0])
        assert n_keep == int(self._counts_host[1]) and 0 <= n_keep <= self._scores.numel()
        m = metrics_from_sums(self._sums_host.tolist())
        filtered = torch.cat([self._kx[:n_keep], self._ks[:n_keep, None]], dim=1)
        e = self._ev
        return LTSResult(filtered, self._scores, self._rows[:, 1:4], self._rows[:, 5], m["loss"], m["r2"], m["dIoU"],
                         m["precision"], m["recall"], m["f1"], m["accuracy"],
                         {k: m[k] for k in ("count", "tp", "fp", "fn", "tn")}, time.time() - self._t0,
                         e[0].elapsed_time(e[1]) * 1e-3, e[1].elapsed_time(e[2]) * 1e-3, e[2].elapsed_time(e[3]) * 1e-3)


class LTSFilter:
    def __init__(self, model, lidar: str = 'hdl-32', epsilon_1: float = 0.84, device="cuda"):
        assert lidar in {'vlp-16', 'hdl-32'}, 'lidar type should be \'vlp-16\' or \'hdl-32\''
        self.model, self.lidar, self.epsilon_1 = model, lidar, float(epsilon_1)
        self.device = torch.device(device if torch.device(device).index is not None else f"cuda:{torch.cuda.current_device()}")
        self.beams, self.window_size, self.num_windows = _native.lts_lidar_info(lidar)
        self.N = self.beams * self.window_size
        with torch.cuda.device(self.device):
            self.stream = torch.cuda.current_stream()
            self.ctx = get_context(self.device.index, self.stream.cuda_stream)    # sps_metrics_dev / sps_compact_stable
            self.handle = model.handle(self.device.index)

    @torch.no_grad()
    def submit(self, points) -> PendingLTS:
        t0 = time.time()
        pts = torch.as_tensor(points)
        _require_device_tensor(pts, "LTSFilter input")
        if pts.dim() != 2 or pts.shape[1] < 4:
            raise ValueError(f"points must be [n, >=4] (x, y, z, intensity), got {tuple(pts.shape)}")
        pts = pts.to(torch.float32)
        if pts.stride(1) != 1:
            pts = pts.contiguous()
        B, N, dev = self.num_windows, self.N, self.device
        M = B * N
        eps = self.epsilon_1
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream()
            if st.cuda_stream != self.stream.cuda_stream:
                raise RuntimeError("LTSFilter must be called on the stream it was created on")
            self.handle = self.model.handle(dev.index)
            s = st.cuda_stream
            frame = torch.empty((self.beams, 1024, 4), dtype=torch.float32, device=dev)
            x = torch.empty((B, 3, N), dtype=torch.float32, device=dev)
            rows = torch.empty((M, 6), dtype=torch.float32, device=dev)
            scores = torch.empty(M, dtype=torch.float32, device=dev)
            kept_xyz = torch.empty((M, 3), dtype=torch.float32, device=dev)
            kept_s = torch.empty(M, dtype=torch.float32, device=dev)
            counts = torch.zeros(2, dtype=torch.int32, device=dev)
            sums = torch.zeros(8, dtype=torch.float64, device=dev)
            counts_host = torch.empty(2, dtype=torch.int32).pin_memory()
            sums_host = torch.empty(8, dtype=torch.float64).pin_memory()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record(st)
            self.handle.project(pts.data_ptr(), pts.stride(0), pts.shape[0], _native.LTS_LIDARS[self.lidar],
                                frame.data_ptr(), x.data_ptr(), rows.data_ptr(), s)
            ev[1].record(st)
            self.handle.forward(x.data_ptr(), B, N, scores.data_ptr(), s)
            ev[2].record(st)
            self.ctx.metrics_dev(scores.data_ptr(), rows.data_ptr(), 6, M, eps, 1, sums.data_ptr(), s)
            self.ctx.compact_stable(scores.data_ptr(), rows.data_ptr() + 4, 6, 3, M, eps, kept_xyz.data_ptr(),
                                    counts.data_ptr(), s)
            self.ctx.compact_stable(scores.data_ptr(), scores.data_ptr(), 1, 1, M, eps, kept_s.data_ptr(),
                                    counts.data_ptr() + 4, s)
            ev[3].record(st)
            counts_host.copy_(counts, non_blocking=True)
            sums_host.copy_(sums, non_blocking=True)
        return PendingLTS(self, rows, scores, kept_xyz, kept_s, counts, sums, counts_host, sums_host, ev, st, t0)

    def __call__(self, points) -> LTSResult:
        return self.submit(points).result()
