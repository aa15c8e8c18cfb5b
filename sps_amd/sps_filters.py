"""Node-complete online SPS filters: everything the reference's two SPS nodes publish and log per frame, without ROS.

    SPSFilter      c_ws/src/sps_filter/scripts/sps_node.py:88-176
        pose transform (:103) -> variant-B submap (:111-115) -> infer (:120) -> loss / R2 (:123-126) -> pred / gt and
        calculate_metrics (:131-134) -> the kept rows AS RECEIVED, score <= eps (:148) -> debug clouds (:152-161)
        -> the two log lines (:136-142, :168-175)
    SPSCVMFilter   c_ws/src/sps_filter/scripts/sps_node_cvm.py:116-199
        the same body for a scan that comes without a pose: the pose is predicted by a constant-velocity model over the
        corrected poses received so far (ConstantVelocityModel, :83-114), the submap is pruned at 0.2 m (:60) while the
        network still quantises at its own voxel size, and the kept rows are those with pred == 0, score < eps (:171)

``pipeline.StableFilter`` stays the lean form (scores + three kept columns).  Same pattern as it and as
baseline_filters: ``submit()`` issues the whole frame on the caller's stream -- sps_filter_prepare, sps_forward_n,
sps_filter_finish and two small copies -- and never synchronises with the host; ``PendingSPS.result()`` is the one
synchronisation and raises ``SpsError`` for a frame that met an unrepresentable coordinate; the next frame is clean.
Every tensor of a result belongs to its frame.  A filter owns a native context (its map hash), so filters with
different prune sizes can share a stream.
"""
from __future__ import annotations

import time
from dataclasses import dataclass

import numpy as np
import torch

from . import _native
from .baseline_filters import _check_stream, _device_of, _elapsed, _pose, _scan_input
from .models.models import metrics_from_sums

LABEL_COLUMN = 3                                     # sps_node.py:107: self.scan[:, 3]
CVM_PRUNE_VOXEL_SIZE = 0.2                           # sps_node_cvm.py:60: self.ds = 0.2 #cfg["MODEL"]["VOXEL_SIZE"]


def hz(t):
    return 1 / t if t else 0                          # sps_node.py:166


def node_metrics(sums) -> dict:
    """The frame's published numbers from the accumulator row [count, TP, FP, FN, TN, sum (s-g)^2, sum g, sum g^2]:
    nn.MSELoss and R2Score (sps_node.py:123-124) and util.calculate_metrics (util.py:285-299: zero guards on precision,
    recall and f1 only).  A thin name for models.metrics_from_sums, which holds the arithmetic."""
    return metrics_from_sums(sums)


@dataclass
class SPSResult:
    filtered: torch.Tensor     # [m, cols] the kept rows, whole, as received (float32)
    scores: torch.Tensor       # [n] stability score of every scan point
    labels: torch.Tensor       # [n] int32 pred = score < eps ? 0 : 1
    cloud_tr: torch.Tensor     # [n, 4] (x', y', z', pred): debug/raw_cloud_tr
    submap: torch.Tensor       # [M, 4] (vx, vy, vz, 1): debug/cloud_submap
    n_scan_voxels: int         # S of the log line
    n_submap_voxels: int       # M
    loss: float                # None for a scan without a label column, like the six below
    r2: float
    dIoU: float
    accuracy: float
    precision: float
    recall: float
    f1: float
    counts: dict               # count, tp, fp, fn, tn
    pose: np.ndarray           # the 4x4 the scan was transformed by (the predicted one for SPSCVMFilter); None = identity
    t_total: float             # seconds: host wall time submit -> result
    t_prune: float             # GPU seconds (hipEvents): transform + submap
    t_infer: float             # GPU seconds: forward
    t_finish: float            # GPU seconds: sps_filter_finish

    def log_lines(self):
        """The node's two log strings (sps_node.py:136-142 and :168-175), trailing blanks included."""
        nan = float("nan")
        v = lambda x: nan if x is None else x
        metrics = (f"dIoU: {v(self.dIoU):.3f} "
                   f"accuracy: {v(self.accuracy):.3f} "
                   f"precision: {v(self.precision):.3f} "
                   f"recall: {v(self.recall):.3f} "
                   f"f1: {v(self.f1):.3f} ")
        timing = (f"T: {self.t_total:.3f} [{hz(self.t_total):.2f} Hz] "
                  f"P: {self.t_prune:.3f} [{hz(self.t_prune):.2f} Hz] "
                  f"I: {self.t_infer:.3f} [{hz(self.t_infer):.2f} Hz] "
                  f"L: {v(self.loss):.3f} r2: {v(self.r2):.3f} "
                  f"N: {len(self.scores):d} n: {len(self.filtered):d} "
                  f"S: {self.n_scan_voxels:d} M: {self.n_submap_voxels:d} ")
        return metrics, timing


class PendingSPS:
    """A frame whose work has been issued; everything lives on the device until result()."""

    def __init__(self, owner, n, has_gt, T, scores, labels, filtered, cloud_tr, submap, counts_host, sums_host, ev, stream, t0):
        self._o, self.n, self._has_gt, self._T = owner, n, has_gt, T
        self._scores, self._labels, self._filtered, self._cloud_tr, self._submap = scores, labels, filtered, cloud_tr, submap
        self._counts_host, self._sums_host, self._ev, self._stream, self._t0 = counts_host, sums_host, ev, stream, t0

    @property
    def count_dev(self) -> torch.Tensor:
        """int32 [1] on the device: the number of kept rows, valid in stream order (for a stage that follows the filter
        without waiting for result(), e.g. localiser.ScanToMapLocaliser.submit_filtered)."""
        return self._keep[3][3:4]

    def result(self) -> SPSResult:
        self._stream.synchronize()                                   # the one host synchronisation of the frame
        self._o.ctx.check_errors(self._stream.cuda_stream)           # SPS_ERR_RANGE etc.
        n_sub, n_scan_vox, _, n_keep = (int(x) for x in self._counts_host.tolist())
        n = self.n
        # sps_node.py:147 (same message): one score per scan point as received
        assert len(self._scores[:n]) == n, f"Predicted scans labels len ({len(self._scores[:n])}) does not equal scan len ({n})"
        assert 0 <= n_keep <= n and 0 <= n_sub <= n
        m = node_metrics(self._sums_host.tolist()) if self._has_gt else None
        g = (lambda k: m[k]) if m else (lambda k: None)
        counts = {k: m[k] for k in ("count", "tp", "fp", "fn", "tn")} if m else None
        t = _elapsed(self._ev)
        return SPSResult(self._filtered[:n_keep], self._scores[:n], self._labels[:n], self._cloud_tr[:n], self._submap[:n_sub],
                         n_scan_vox, n_sub, g("loss"), g("r2"), g("dIoU"), g("accuracy"), g("precision"), g("recall"), g("f1"),
                         counts, self._T, time.time() - self._t0, t[0], t[1], t[2])


class SPSFilter:
    """sps_node.py:88-176.  ``submit(scan, pose)`` takes [n, 3] rows or [n, >= 4] rows whose column 3 is the label
    (:107); the kept rows come back whole, every column, in float32.  ``keep_strict`` selects the second node's rule
    (see SPSCVMFilter); ``prune_voxel_size`` is the grid of the submap when it differs from the network's."""

    keep_strict = False

    def __init__(self, model, map_points, voxel_size: float = 0.1, epsilon: float = 0.84, device="cuda",
                 prune_voxel_size: float = None):
        self.model, self.ds, self.epsilon = model, float(voxel_size), float(epsilon)
        self.prune_ds = self.ds if prune_voxel_size is None else float(prune_voxel_size)
        if not (self.ds > 0 and self.prune_ds > 0):
            raise ValueError("voxel sizes must be > 0")
        self.device = _device_of(device)
        self.map_xyz = torch.as_tensor(map_points)[:, :3].to(torch.float32).to(self.device).contiguous()   # sps_node.py:69-74
        with torch.cuda.device(self.device):
            self.stream = torch.cuda.current_stream()
            self.ctx = _native.Context(self.device.index)
            self.ctx.map_upload(self.map_xyz.data_ptr(), 3, len(self.map_xyz), self.prune_ds, self.stream.cuda_stream)

    @classmethod
    def from_checkpoint(cls, cfg, weights_pth, map_points, device="cuda", **kw):
        """The node's constructor (sps_node.py:55-63): util.load_model on the Lightning checkpoint, the voxel size of
        the config; epsilon defaults to the node's parameter default 0.84."""
        from .datasets import util
        model = util.load_model(cfg, weights_pth, device=_device_of(device))
        return cls(model, map_points, voxel_size=cfg["MODEL"]["VOXEL_SIZE"], device=device, **kw)

    def _frame_pose(self, pose):
        return _pose(pose)

    @torch.no_grad()
    def submit(self, scan, pose=None) -> PendingSPS:
        t0 = time.time()
        raw, _ = _scan_input(scan, self.device, type(self).__name__)
        T = self._frame_pose(pose)
        n, cols, dev = raw.shape[0], raw.shape[1], self.device
        has_gt = cols > LABEL_COLUMN
        raw32 = raw if raw.dtype == torch.float32 else raw.to(torch.float32)     # the rows the node publishes are float32
        m = max(n, 1)
        with torch.cuda.device(dev):
            st = _check_stream(self, type(self).__name__)
            s = st.cuda_stream
            net = self.model.model
            net._sync_weights(self.ctx)
            batch = torch.empty((2 * m, 5), dtype=torch.float32, device=dev)
            scores = torch.empty(2 * m, dtype=torch.float32, device=dev)
            filtered = torch.empty((m, cols), dtype=torch.float32, device=dev)
            labels = torch.empty(m, dtype=torch.int32, device=dev)
            cloud_tr = torch.empty((m, 4), dtype=torch.float32, device=dev)
            submap = torch.empty((m, 4), dtype=torch.float32, device=dev)
            counts = torch.zeros(4, dtype=torch.int32, device=dev)       # n_sub, n_scan_vox, n + n_sub, kept
            sums = torch.zeros(8, dtype=torch.float64, device=dev)
            counts_host = torch.empty(4, dtype=torch.int32).pin_memory()
            sums_host = torch.empty(8, dtype=torch.float64).pin_memory()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record(st)
            # :103 transform, :111-115 submap (on the prune grid), util.py:166-176 tensor assembly
            self.ctx.filter_prepare(raw.data_ptr(), raw.dtype == torch.float64, raw.stride(0), n, T, batch.data_ptr(),
                                    counts.data_ptr(), s)
            ev[1].record(st)
            # :120 infer (on the network's grid): the row count n + n_sub is read from counts[2] on the device
            self.ctx.forward_n(batch.data_ptr(), 5, 2 * n, counts.data_ptr() + 8, float(net.voxel_size), scores.data_ptr(), s)
            ev[2].record(st)
            # :123-161 metric sums, pred, kept rows, debug clouds
            self.ctx.filter_finish(scores.data_ptr(), n, raw32.data_ptr(), raw32.stride(0), cols,
                                   LABEL_COLUMN if has_gt else -1, batch.data_ptr(), counts.data_ptr(), self.epsilon,
                                   self.keep_strict, filtered.data_ptr(), counts.data_ptr() + 12, labels.data_ptr(),
                                   cloud_tr.data_ptr(), submap.data_ptr(), sums.data_ptr(), s)
            ev[3].record(st)
            counts_host.copy_(counts, non_blocking=True)
            sums_host.copy_(sums, non_blocking=True)
        pend = PendingSPS(self, n, has_gt, T, scores, labels, filtered, cloud_tr, submap, counts_host, sums_host, ev, st, t0)
        pend._keep = (raw, raw32, batch, counts, sums)                 # inputs of work that may still be in flight
        return pend

    def __call__(self, scan, pose=None) -> SPSResult:
        return self.submit(scan, pose).result()


class ConstantVelocityModel:
    """The pose list and get_prediction_model of sps_node_cvm.py:83-114, in float64 on the host, as written there:

      * the list starts as [I] (:83), so the first corrected pose is the SECOND entry;
      * below four entries the prediction is the identity (:91-92);
      * the model averages 3 relative motions up to 10 entries and 9 after that (:94);
      * relative motion i is inv(poses[-i]) @ poses[-i + 1] for i = 2 .. (:97-98), newest first, so predictions[-1]
        (:105), whose rotation the result keeps, is the OLDEST of them;
      * the whole fourth column of that matrix, its last element included, is replaced by the mean's (:106);
      * the result is poses[-1] @ that matrix (:108)."""

    def __init__(self):
        self.poses = [np.eye(4)]

    def add_pose(self, T) -> None:
        T = np.array(T, dtype=np.float64)
        if T.shape != (4, 4):
            raise ValueError("pose must be a 4x4 matrix")
        self.poses.append(T)

    def predict(self) -> np.ndarray:
        num_poses = len(self.poses)
        if num_poses < 4:
            return np.eye(4)
        num_predictions = 3 if num_poses <= 10 else 9
        inverse_poses = [np.linalg.inv(self.poses[num_poses - i]) for i in range(2, 2 + num_predictions)]
        predictions = [np.dot(inverse_poses[i - 2], self.poses[num_poses - i + 1]) for i in range(2, 2 + num_predictions)]
        mean_prediction = np.mean(predictions, axis=0)
        prediction = predictions[-1]
        prediction[:, 3] = mean_prediction[:, 3]
        return np.dot(self.poses[-1], prediction)


class SPSCVMFilter(SPSFilter):
    """sps_node_cvm.py:116-199: ``add_pose(T)`` is the odometry callback (:112-114), ``submit(scan)`` the cloud
    callback, which transforms by the predicted pose (:122-125).  The node's two quirks:

      * it prunes the submap at 0.2 m whatever the configured voxel size (:60) while SPSModel still quantises at the
        configured one -- ``prune_voxel_size`` (default 0.2) and ``voxel_size`` are independent here too;
      * it keeps ``scan[pred == 0]`` (:171), i.e. score < eps, where sps_node.py keeps score <= eps (:148): a point
        whose score is exactly eps is kept by SPSFilter and dropped here."""

    keep_strict = True

    def __init__(self, model, map_points, voxel_size: float = 0.1, epsilon: float = 0.84, device="cuda",
                 prune_voxel_size: float = CVM_PRUNE_VOXEL_SIZE):
        super().__init__(model, map_points, voxel_size, epsilon, device, prune_voxel_size)
        self.cvm = ConstantVelocityModel()

    def add_pose(self, T) -> None:
        self.cvm.add_pose(T)

    def _frame_pose(self, pose):
        if pose is not None:
            raise ValueError("SPSCVMFilter predicts the pose of a scan itself: feed corrected poses through add_pose()")
        return self.cvm.predict()
