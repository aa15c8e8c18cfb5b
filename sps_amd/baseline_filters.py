"""Online 4DMOS, MapMOS and mask filters: the per-frame bodies of the reference's other scan filters without ROS
(the filters its localisation experiment puts in front of hdl_localization next to sps_node / stability_filter).

    MOS4DFilter   c_ws/src/mos4d/scripts/mos4d_node.py:80-147
        pose transform (:97) -> stamp with the scan index, append to the window, drop the oldest (:98-110)
        -> MOS4DNet over the window oldest -> newest (:113-117) -> labels of the newest scan, keep label 0 (:121-127)
        -> calculate_metrics against s < 0.84 (:83, :131-133)
    MapMOSFilter  c_ws/src/mapmos/scripts/mapmos_node.py:70-112
        30 m crop of the map around the pose origin (:63-68, :79-80) -> pose transform (:89) -> MapMOSNet.predict on
        scan + crop (:91-95) -> to_label, keep label 0 (:97-101)
    MaskFilter    c_ws/src/sps_filter/scripts/mask.py:86-147
        pose transform (:101) -> variant-B submap (:109-114) -> inverse transform of the submap rows (:118-123)

Same pattern as pipeline.StableFilter and lts_filter.LTSFilter: ``submit()`` issues the whole frame on the caller's stream
and never synchronises with the host (the row counts -- window length, crop size, kept rows -- stay on the device);
``Pending*.result()`` is the one synchronisation and raises ``SpsError`` for a frame that met an unrepresentable
coordinate (or, MapMOS, a crop larger than its capacity); the next frame is clean again.  Every tensor of a result belongs
to its frame: later submits allocate their own buffers.  The native pieces are the entry points of the "online baseline
filters" section of include/sps_hip.h.
"""
from __future__ import annotations

import math
import re
import time
from dataclasses import dataclass

import numpy as np
import torch

from . import _native
from .models.baselines import T_MAX, T_MIN, MapMOSNet, MOS4DNet
from .models.models import get_context, metrics_from_sums

SPS_MAX_POINTS = 1 << 23          # include/sps_hip.h


def window_t_base(indices) -> float:
    """baselines._t_base for a window of scan indices, from the host-side counter (no device read): 0 when every index
    already lies in the key's t range [-16, 15], else the oldest index."""
    if len(indices) == 0:
        return 0.0
    lo, hi = min(indices), max(indices)
    if T_MIN <= lo and hi <= T_MAX:
        return 0.0
    return float(lo)


class ScanWindow:
    """mos4d_node.py:98-110: every scan gets the next index of an ever-growing counter; the window holds the last
    ``buffer_size`` entries (append, then drop the oldest)."""

    def __init__(self, buffer_size: int, first_index: int = 0):
        self.buffer_size, self.next_index = int(buffer_size), int(first_index)
        self.entries = []                               # [(index, payload)], oldest first

    def push(self, payload=None) -> int:
        idx = self.next_index
        self.next_index += 1
        self.entries.append((idx, payload))
        if len(self.entries) > self.buffer_size:
            self.entries.pop(0)
        return idx

    def discard(self, index: int) -> None:
        self.entries = [e for e in self.entries if e[0] != index]

    @property
    def indices(self):
        return [i for i, _ in self.entries]

    @property
    def t_base(self) -> float:
        return window_t_base(self.indices)


def buffer_size_from_path(path: str) -> int:
    """mos4d_node.py:31-40: the window length is the integer of ``<k>_scans.ckpt`` in the checkpoint's file name."""
    m = re.search(r'(\d+)_scans\.ckpt', str(path))
    if not m:
        raise ValueError(f"buffer size not found in the path {path!r} (expected '<k>_scans.ckpt')")
    return int(m.group(1))


def load_state_dict(path, prefix: str) -> dict:
    """load_model of the nodes (mos4d_node.py:63-68, mapmos_node.py:46-52): strip ``prefix``, drop the MOSLoss keys."""
    sd = torch.load(path, map_location="cpu")["state_dict"]
    sd = {k.replace(prefix, ""): v for k, v in sd.items()}
    return {k: v for k, v in sd.items() if "MOSLoss" not in k}


def _pose(pose):
    T = None if pose is None else np.asarray(pose, dtype=np.float64)
    if T is not None and T.shape != (4, 4):
        raise ValueError("pose must be a 4x4 matrix")
    return T


def _device_of(device):
    return torch.device(device if torch.device(device).index is not None else f"cuda:{torch.cuda.current_device()}")


def _scan_input(scan, device, name):
    """The scan on the device in its own dtype (float32 / float64) plus its float32 (x, y, z[, s]) rows."""
    raw = torch.as_tensor(scan)
    if raw.dtype not in (torch.float32, torch.float64):
        raw = raw.to(torch.float32)
    raw = raw.to(device, non_blocking=True)
    if raw.dim() != 2 or raw.shape[1] < 3:
        raise ValueError(f"{name}: scan must be [n, >=3], got {tuple(raw.shape)}")
    if raw.shape[0] == 0:                              # (an empty tensor may report any row stride)
        raw = torch.empty((0, raw.shape[1]), dtype=raw.dtype, device=raw.device)
    if raw.stride(1) != 1:
        raw = raw.contiguous()
    raw32 = raw if raw.dtype == torch.float32 else raw[:, :4].to(torch.float32)
    return raw, raw32


def _check_stream(owner, name):
    st = torch.cuda.current_stream()
    if st.cuda_stream != owner.stream.cuda_stream:
        raise RuntimeError(f"{name} must be called on the stream it was created on")
    return st


def _elapsed(ev):
    return [ev[i].elapsed_time(ev[i + 1]) * 1e-3 for i in range(len(ev) - 1)]


# ---- 4DMOS -----------------------------------------------------------------------------------------------------------
@dataclass
class MOS4DResult:
    logits: torch.Tensor       # [n] logits of the newest scan (column 2 of the head, mos4d.py:32)
    labels: torch.Tensor       # [n] float32 0 / 1 (logits > 0)
    filtered: torch.Tensor     # [m, 4] (x, y, z, 0) of the label-0 points, as received (mos4d_node.py:124-127)
    transformed: torch.Tensor  # [n, 3] the scan in the map frame (float32)
    scan_index: int
    window: list               # scan indices of the forward's window, oldest first
    precision: float           # util.calculate_metrics vs s < 0.84 (NaN-free zero guards of metrics_from_sums);
    recall: float              # all None when the scan has no intensity column
    F1: float
    accuracy: float
    dIoU: float
    counts: dict               # count, tp, fp, fn, tn (None without an intensity column)
    t_total: float             # seconds: host wall time submit -> result
    t_prepare: float           # GPU seconds (hipEvents): transform + window gather
    t_infer: float             # GPU seconds: forward
    t_filter: float            # GPU seconds: labels + compaction + counts


class PendingMOS4D:
    def __init__(self, owner, idx, window, n, logits, labels, filtered, rows, counts, counts_host, has_gt, ev, stream, t0):
        self._o, self.scan_index, self._window, self.n = owner, idx, window, n
        self._logits, self._labels, self._filtered, self._rows = logits, labels, filtered, rows
        self._counts, self._counts_host, self._has_gt, self._ev, self._stream, self._t0 = \
            counts, counts_host, has_gt, ev, stream, t0

    def result(self) -> MOS4DResult:
        self._stream.synchronize()                                      # the one host synchronisation of the frame
        try:
            self._o.ctx.check_errors(self._stream.cuda_stream)
        except _native.SpsError:
            self._o.window.discard(self.scan_index)                     # an unkeyable scan never enters another forward
            raise
        n_keep, tp, fp, fn, tn = (int(x) for x in self._counts_host.tolist())
        assert 0 <= n_keep <= self.n
        m = metrics_from_sums([self.n, tp, fp, fn, tn, 0, 0, 0]) if self._has_gt else None
        g = (lambda k: m[k]) if m else (lambda k: None)
        counts = {k: m[k] for k in ("count", "tp", "fp", "fn", "tn")} if m else None
        t = _elapsed(self._ev)
        return MOS4DResult(self._logits, self._labels, self._filtered[:n_keep], self._rows[:, 1:4], self.scan_index,
                           list(self._window), g("precision"), g("recall"), g("f1"), g("accuracy"), g("dIoU"), counts,
                           time.time() - self._t0, t[0], t[1], t[2])


class MOS4DFilter:
    """mos4d_node.py:80-147.  The window keeps the last ``buffer_size`` TRANSFORMED scans on the device as float32 rows
    (0, x', y', z', scan index), one tensor per scan, each transformed once; a frame gathers them oldest -> newest into its
    own batch (the rows MOS4DNet.forward gets from the node's np.vstack) and re-bases t on the host (window_t_base).
    ``buffer_size`` is at most 16: the forward's key holds t - t_base in [-16, 15] and t_base is the oldest index."""

    def __init__(self, model: MOS4DNet, buffer_size: int = 10, filter: bool = True, device="cuda", first_index: int = 0):
        if not isinstance(model, MOS4DNet):
            raise TypeError("MOS4DFilter needs a MOS4DNet")
        if int(buffer_size) != buffer_size or not 1 <= buffer_size <= T_MAX + 1:
            raise ValueError(f"buffer_size must be an integer in [1, {T_MAX + 1}] (the window must fit the t-key range), "
                             f"got {buffer_size}")
        self.model, self.filter = model, bool(filter)
        self.window = ScanWindow(int(buffer_size), first_index)
        self.device = _device_of(device)
        with torch.cuda.device(self.device):
            self.stream = torch.cuda.current_stream()
            self.ctx = get_context(self.device.index, self.stream.cuda_stream)

    @property
    def buffer_size(self) -> int:
        return self.window.buffer_size

    @classmethod
    def from_checkpoint(cls, path, filter: bool = True, device="cuda", **kw) -> "MOS4DFilter":
        """load_model (mos4d_node.py:63-76): model.MinkUNet. stripped, MOSLoss dropped, voxel 0.2; the window length
        from the file name (:31-40)."""
        buffer_size = buffer_size_from_path(path)
        model = MOS4DNet(0.2)
        model.MinkUNet.load_state_dict(load_state_dict(path, "model.MinkUNet."))
        model = model.to(_device_of(device)).eval().freeze()
        return cls(model, buffer_size=buffer_size, filter=filter, device=device, **kw)

    @torch.no_grad()
    def submit(self, scan, pose=None) -> PendingMOS4D:
        t0 = time.time()
        raw, raw32 = _scan_input(scan, self.device, "MOS4DFilter")
        T = _pose(pose)
        n, dev = raw.shape[0], self.device
        has_gt = raw.shape[1] >= 4
        with torch.cuda.device(dev):
            st = _check_stream(self, "MOS4DFilter")
            s = st.cuda_stream
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record(st)
            rows = torch.empty((n, 5), dtype=torch.float32, device=dev)
            idx = self.window.push(rows)
            self.ctx.transform_rows(raw.data_ptr(), raw.dtype == torch.float64, raw.stride(0), n, T, float(idx),
                                    rows.data_ptr(), 5, None, 0.0, s)
            window = self.window.indices
            if self.filter:
                parts = [r for _, r in self.window.entries]
                batch = parts[0] if len(parts) == 1 else torch.cat(parts)       # one gather into the frame's own batch
                N = batch.shape[0]
                ev[1].record(st)
                out = torch.empty((N, 3), dtype=torch.float32, device=dev)
                self.model._sync_weights(self.ctx)
                self.ctx.forward_head(batch.data_ptr(), 5, N, float(self.model.ds), None, self.window.t_base,
                                      out.data_ptr(), 3, 0, s)
                logits = out[N - n:, 2]                                          # the newest scan's rows come last
                lptr, ldl = out.data_ptr() + ((N - n) * 3 + 2) * 4, 3
            else:                                                                # :117: no forward, every label 0
                ev[1].record(st)
                logits = torch.zeros(n, dtype=torch.float32, device=dev)
                lptr, ldl = logits.data_ptr(), 1
            ev[2].record(st)
            labels = torch.empty(n, dtype=torch.float32, device=dev)
            filtered = torch.empty((n, 4), dtype=torch.float32, device=dev)
            counts = torch.empty(5, dtype=torch.int32, device=dev)
            gt = raw32.data_ptr() + 12 if has_gt else None
            self.ctx.label_filter(lptr, ldl, n, raw32.data_ptr(), raw32.stride(0), gt, raw32.stride(0), labels.data_ptr(),
                                  filtered.data_ptr(), counts.data_ptr(), s)
            ev[3].record(st)
            counts_host = torch.empty(5, dtype=torch.int32).pin_memory()
            counts_host.copy_(counts, non_blocking=True)
        return PendingMOS4D(self, idx, window, n, logits, labels, filtered, rows, counts, counts_host, has_gt, ev, st, t0)

    def __call__(self, scan, pose=None) -> MOS4DResult:
        return self.submit(scan, pose).result()


# ---- MapMOS ----------------------------------------------------------------------------------------------------------
@dataclass
class MapMOSResult:
    logits_scan: torch.Tensor  # [n]
    labels: torch.Tensor       # [n] float32 0 / 1 (to_label)
    filtered: torch.Tensor     # [m, 4] (x, y, z, 0) of the label-0 points, as received (mapmos_node.py:100-101)
    crop: torch.Tensor         # [n_map, 3] the map points within the radius (float32; mapmos_node.py:107 publishes them)
    logits_map: torch.Tensor   # [n_map]
    n_map: int
    t_total: float             # seconds: host wall time submit -> result
    t_prepare: float           # GPU seconds (hipEvents): transform + crop
    t_infer: float             # GPU seconds: forward
    t_filter: float            # GPU seconds: labels + compaction


class PendingMapMOS:
    def __init__(self, owner, n, batch, out, labels, filtered, counts, counts_host, ev, stream, t0):
        self._o, self.n, self._batch, self._out, self._labels, self._filtered = owner, n, batch, out, labels, filtered
        self._counts, self._counts_host, self._ev, self._stream, self._t0 = counts, counts_host, ev, stream, t0

    def result(self) -> MapMOSResult:
        self._stream.synchronize()
        self._o.ctx.check_errors(self._stream.cuda_stream)              # SPS_ERR_RANGE, SPS_ERR_ITEMCAP (crop capacity)
        c = [int(x) for x in self._counts_host.tolist()]
        n, n_map, n_keep = self.n, c[0], c[2]
        assert c[1] == n + n_map and 0 <= n_keep <= n
        t = _elapsed(self._ev)
        return MapMOSResult(self._out[:n], self._labels, self._filtered[:n_keep], self._batch[n:n + n_map, 1:4],
                            self._out[n:n + n_map], n_map, time.time() - self._t0, t[0], t[1], t[2])


class MapMOSFilter:
    """mapmos_node.py:70-112.  The map is uploaded once (float64 when given as float64, else float32).  A frame writes ONE
    batch: the scan rows (0, x', y', z', 0) with feature 1, then the crop rows (0, x, y, z, -1) with feature 2 (1 when
    the scan is empty: mapmos.py:64-71 with i_min == i_max) -- the rows and per-point features MapMOSNet.predict builds.
    The forward reads its row count (scan + crop) from the device.  ``crop_capacity`` bounds the crop rows a frame
    reserves (the forward sizes its arena for scan + capacity rows); default min(map size, SPS_MAX_POINTS - scan size).
    A crop larger than the capacity is reported by result() (SpsError, SPS_ERR_ITEMCAP); the next frame is clean."""

    def __init__(self, model: MapMOSNet, map_points, radius: float = 30.0, crop_capacity=None, device="cuda"):
        if not isinstance(model, MapMOSNet):
            raise TypeError("MapMOSFilter needs a MapMOSNet")
        if not (math.isfinite(radius) and radius >= 0):
            raise ValueError(f"radius must be finite and >= 0, got {radius}")
        if crop_capacity is not None and not 0 <= int(crop_capacity) <= SPS_MAX_POINTS:
            raise ValueError(f"crop_capacity must be in [0, {SPS_MAX_POINTS}], got {crop_capacity}")
        self.model, self.radius = model, float(radius)
        self.crop_capacity = None if crop_capacity is None else int(crop_capacity)
        mp = torch.as_tensor(map_points)
        if mp.dim() != 2 or mp.shape[1] < 3:
            raise ValueError(f"map_points must be [m, >=3], got {tuple(mp.shape)}")
        if mp.shape[0] > SPS_MAX_POINTS:
            raise ValueError(f"the map has {mp.shape[0]} points (limit {SPS_MAX_POINTS})")
        self.device = _device_of(device)
        mp = mp[:, :3].to(torch.float64 if mp.dtype == torch.float64 else torch.float32)
        self.map = mp.to(self.device).contiguous()                       # mapmos_node.py:40, once
        with torch.cuda.device(self.device):
            self.stream = torch.cuda.current_stream()
            self.ctx = get_context(self.device.index, self.stream.cuda_stream)
            self.scratch = torch.empty(max(1, -(-len(self.map) // _native.CROP_BLOCK)), dtype=torch.int32, device=self.device)

    @classmethod
    def from_checkpoint(cls, path, map_points, device="cuda", **kw) -> "MapMOSFilter":
        """load_model (mapmos_node.py:46-56): mos.MinkUNet. stripped, MOSLoss dropped, voxel 0.1."""
        model = MapMOSNet(0.1)
        model.MinkUNet.load_state_dict(load_state_dict(path, "mos.MinkUNet."))
        model = model.to(_device_of(device)).eval().freeze()
        return cls(model, map_points, device=device, **kw)

    def capacity(self, n_scan: int) -> int:
        m = len(self.map)
        cap = min(m, SPS_MAX_POINTS - n_scan) if self.crop_capacity is None else self.crop_capacity
        if n_scan + cap > SPS_MAX_POINTS:
            raise ValueError(f"scan ({n_scan}) + crop capacity ({cap}) exceed {SPS_MAX_POINTS} rows")
        return cap

    @torch.no_grad()
    def submit(self, scan, pose=None) -> PendingMapMOS:
        t0 = time.time()
        raw, raw32 = _scan_input(scan, self.device, "MapMOSFilter")
        T = _pose(pose)
        n, dev = raw.shape[0], self.device
        cap = self.capacity(n)
        with torch.cuda.device(dev):
            st = _check_stream(self, "MapMOSFilter")
            s = st.cuda_stream
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record(st)
            batch = torch.empty((n + cap, 5), dtype=torch.float32, device=dev)
            feats = torch.empty(n + cap, dtype=torch.float32, device=dev)
            out = torch.empty(n + cap, dtype=torch.float32, device=dev)
            counts = torch.empty(8, dtype=torch.int32, device=dev)   # [n_map, n + n_map, kept, tp, fp, fn, tn, -]
            self.ctx.transform_rows(raw.data_ptr(), raw.dtype == torch.float64, raw.stride(0), n, T, 0.0, batch.data_ptr(), 5,
                                    feats.data_ptr(), 1.0, s)
            self.ctx.radius_crop(self.map.data_ptr(), self.map.dtype == torch.float64, 3, len(self.map), T, self.radius,
                                 self.scratch.data_ptr(), n, batch.data_ptr(), 5, cap, feats.data_ptr(),
                                 2.0 if n else 1.0, counts.data_ptr(), s)
            ev[1].record(st)
            self.model._sync_weights(self.ctx)
            self.ctx.forward_head_n(batch.data_ptr(), 5, n + cap, counts.data_ptr() + 4, float(self.model.voxel_size),
                                    feats.data_ptr(), 0.0, out.data_ptr(), 1, 0, s)
            ev[2].record(st)
            labels = torch.empty(n, dtype=torch.float32, device=dev)
            filtered = torch.empty((n, 4), dtype=torch.float32, device=dev)
            self.ctx.label_filter(out.data_ptr(), 1, n, raw32.data_ptr(), raw32.stride(0), None, 1, labels.data_ptr(),
                                  filtered.data_ptr(), counts.data_ptr() + 8, s)
            ev[3].record(st)
            counts_host = torch.empty(8, dtype=torch.int32).pin_memory()
            counts_host.copy_(counts, non_blocking=True)
        return PendingMapMOS(self, n, batch, out, labels, filtered, counts, counts_host, ev, st, t0)

    def __call__(self, scan, pose=None) -> MapMOSResult:
        return self.submit(scan, pose).result()


# ---- mask ------------------------------------------------------------------------------------------------------------
@dataclass
class MaskResult:
    filtered: torch.Tensor     # [m, 4] (x', y', z', 1): the submap voxel corners back in the sensor frame (mask.py:118-123)
    submap: torch.Tensor       # [m, 3] the submap in the map frame
    n_scan_voxels: int         # S of the node's log line
    n_submap_voxels: int       # M
    t_total: float             # seconds: host wall time submit -> result
    t_prune: float             # GPU seconds (hipEvents): transform + submap
    t_inverse: float           # GPU seconds: inverse transform


class PendingMask:
    def __init__(self, owner, n, batch, filtered, counts, counts_host, ev, stream, t0):
        self._o, self.n, self._batch, self._filtered = owner, n, batch, filtered
        self._counts, self._counts_host, self._ev, self._stream, self._t0 = counts, counts_host, ev, stream, t0

    def result(self) -> MaskResult:
        self._stream.synchronize()
        self._o.ctx.check_errors(self._stream.cuda_stream)
        n_sub, n_scan_vox = (int(x) for x in self._counts_host.tolist()[:2])
        assert 0 <= n_sub <= self.n
        t = _elapsed(self._ev)
        return MaskResult(self._filtered[:n_sub], self._batch[self.n:self.n + n_sub, 1:4], n_scan_vox, n_sub,
                          time.time() - self._t0, t[0], t[1])


class MaskFilter:
    """mask.py:86-147: no network.  The map's voxel hash lives in a native context of the filter's own (the shared
    per-stream context keeps whatever map a StableFilter on the same stream uploaded)."""

    def __init__(self, map_points, voxel_size: float = 0.1, device="cuda"):
        if not voxel_size > 0:
            raise ValueError(f"voxel_size must be > 0, got {voxel_size}")
        self.ds = float(voxel_size)
        self.device = _device_of(device)
        self.map_xyz = torch.as_tensor(map_points)[:, :3].to(torch.float32).to(self.device).contiguous()
        with torch.cuda.device(self.device):
            self.stream = torch.cuda.current_stream()
            self.ctx = _native.Context(self.device.index)
            self.ctx.map_upload(self.map_xyz.data_ptr(), 3, len(self.map_xyz), self.ds, self.stream.cuda_stream)

    @torch.no_grad()
    def submit(self, scan, pose=None) -> PendingMask:
        t0 = time.time()
        raw, _ = _scan_input(scan, self.device, "MaskFilter")
        T = _pose(pose)
        Tinv = None if T is None else np.linalg.inv(T)                   # util.inverse_transform_point_cloud
        n, dev = raw.shape[0], self.device
        with torch.cuda.device(dev):
            st = _check_stream(self, "MaskFilter")
            s = st.cuda_stream
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record(st)
            batch = torch.empty((2 * max(n, 1), 5), dtype=torch.float32, device=dev)
            counts = torch.zeros(4, dtype=torch.int32, device=dev)
            self.ctx.filter_prepare(raw.data_ptr(), raw.dtype == torch.float64, raw.stride(0), n, T, batch.data_ptr(),
                                    counts.data_ptr(), s)
            ev[1].record(st)
            filtered = torch.ones((max(n, 1), 4), dtype=torch.float32, device=dev)   # column 3: the label 1 (:119-120)
            self.ctx.transform_points_n(batch.data_ptr() + (5 * n + 1) * 4, False, 5, n, counts.data_ptr(), Tinv,
                                        filtered.data_ptr(), False, 4, s)
            ev[2].record(st)
            counts_host = torch.empty(4, dtype=torch.int32).pin_memory()
            counts_host.copy_(counts, non_blocking=True)
        return PendingMask(self, n, batch, filtered, counts, counts_host, ev, st, t0)

    def __call__(self, scan, pose=None) -> MaskResult:
        return self.submit(scan, pose).result()
