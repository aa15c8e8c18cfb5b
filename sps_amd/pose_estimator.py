"""Device pose estimator: an unscented Kalman filter over position, velocity, orientation and the IMU biases, predicted
by the gyroscope (or by time alone) and corrected by a registered pose (C ABI: the "pose estimator" section of
include/sps_hip.h; the specification is tests/ukf_reference.py).

It plays the role of hdl_localization's pose estimator beside ``NDTLocaliser``; it is a restatement of that filter's
published pose system, not a port of the package.  The state lives in one small device buffer.  Every call is one
launch on the caller's current stream and none synchronises but ``state()``:

    est = PoseEstimator(T0, "cuda", initial_velocity=(5, 0, 0))
    est.predict_imu(samples)                      # [M, 7] rows (dt, ax, ay, az, gx, gy, gz); or est.predict(dt)
    pend = ndt.submit_from_device(rows, count, est.pose_dev)    # the alignment starts from the predicted pose
    est.correct_from(pend)                        # gated on the device by the alignment's status

The velocity is constant in the world frame and the acceleration is read and left out, as in the package: on a curve the
prediction drifts (DESIGN.md 8j has figures)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _native
from .baseline_filters import _device_of, _pose

DONE, GATE_CLOSED, SINGULAR = 0, 2, 3
STATUS_NAMES = {DONE: "done", GATE_CLOSED: "gate closed", SINGULAR: "singular"}
N_STATE, N_MEAS = 16, 7
MAX_IMU = _native.UKF_MAX_IMU
PROCESS_NOISE = (1.0,) * 3 + (1.0,) * 3 + (0.5,) * 4 + (1e-6,) * 3 + (1e-6,) * 3     # pos, vel, quat, acc bias, gyro bias
MEASUREMENT_NOISE = (0.01,) * 3 + (0.001,) * 4                                        # pos, quat


@dataclass
class EstimatorState:
    mean: np.ndarray           # [16] p, v, q (w, x, y, z), accelerometer bias, gyroscope bias
    covariance: np.ndarray     # [16, 16], symmetric bit for bit
    pose: np.ndarray           # [4, 4] the pose of the mean
    status: int                # of the last correction: 0 done, 2 gate closed, 3 singular (0 before the first)
    predict_status: int        # of the last prediction: 0 done, 3 singular
    predict_samples: int       # samples the last prediction ran
    predict_failed: int        # index of the sample that ended the last prediction, -1 where none did
    n_predict: int             # prediction steps done since the start
    n_correct: int             # corrections done since the start
    innovation: np.ndarray     # [7] z - zbar of the last correction (zeros unless its status is 0)


def _diag(values, n, default, what):
    v = np.array(default if values is None else values, dtype=np.float64)
    if v.ndim == 0:
        v = np.full(n, float(v))
    if v.shape != (n,) or not (np.isfinite(v).all() and (v >= 0).all()):
        raise ValueError(f"{what} must be a finite scalar or [{n}] vector, >= 0")
    return (C.c_double * n)(*v.tolist())


def checked_imu(samples) -> np.ndarray:
    """[M, 7] float64 rows (dt, ax, ay, az, gx, gy, gz), finite, dt > 0"""
    s = np.ascontiguousarray(np.asarray(samples, dtype=np.float64))
    if s.size == 0:
        return np.zeros((0, 7))
    if s.ndim != 2 or s.shape[1] != 7:
        raise ValueError(f"IMU samples must be [M, 7] rows (dt, ax, ay, az, gx, gy, gz), got {s.shape}")
    if not np.isfinite(s).all() or not (s[:, 0] > 0).all():
        raise ValueError("IMU samples must be finite with dt > 0")
    return s


class PoseEstimator:
    """``initial_cov``, ``process_noise`` (per second) and ``measurement_noise`` are diagonals: a scalar or a vector of
    16, 16 and 7 entries; the defaults are the package's."""

    def __init__(self, initial_pose, device="cuda", initial_velocity=(0.0, 0.0, 0.0), initial_cov=0.01, process_noise=None,
                 measurement_noise=None):
        T = _pose(initial_pose)
        v = np.asarray(initial_velocity, dtype=np.float64)
        if T is None or not np.isfinite(T).all() or v.shape != (3,) or not np.isfinite(v).all():
            raise ValueError("initial_pose must be a finite 4x4 matrix and initial_velocity three finite numbers")
        self._Q = _diag(process_noise, N_STATE, PROCESS_NOISE, "process_noise")
        self._R = _diag(measurement_noise, N_MEAS, MEASUREMENT_NOISE, "measurement_noise")
        p0 = _diag(initial_cov, N_STATE, 0.01, "initial_cov")
        self.device = _device_of(device)
        words = int(_native.lib.sps_ukf_state_bytes()) // 8
        with torch.cuda.device(self.device):
            # one buffer: the state block | T_pred[16] | predict info int32[4] | correct info [8]
            self._buf = torch.zeros(words + 16 + 2 + 8, dtype=torch.float64, device=self.device)
            self._words = words
            base = self._buf.data_ptr()
            self._state_ptr, self._pred_ptr = base, base + words * 8
            self._pinfo_ptr, self._cinfo_ptr = base + (words + 16) * 8, base + (words + 18) * 8
        self._p0 = p0
        self._init(T, v)
        self._keep = None

    def _init(self, T, v):
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream().cuda_stream
            _native.check(_native.lib.sps_ukf_init(self._state_ptr, _native.Context._mat(T), (C.c_double * 3)(*v.tolist()), self._p0,
                                                   st))
            # the predicted pose before any prediction is the initial one (n_imu = 0 only writes the pose)
            _native.check(_native.lib.sps_ukf_predict(self._state_ptr, None, 0, self._Q, self._pred_ptr, self._pinfo_ptr, st))

    def reset(self, pose, velocity=(0.0, 0.0, 0.0)) -> None:
        """Start again at ``pose`` (4x4) with ``velocity``, the construction's ``initial_cov`` and zeroed biases and counters,
        behind the work issued so far on the current stream: what a new estimator built with the same noise would hold.  For a
        pose that a global search found, to which no motion leads from the state before."""
        T = _pose(pose)
        v = np.asarray(velocity, dtype=np.float64)
        if T is None or not np.isfinite(T).all() or v.shape != (3,) or not np.isfinite(v).all():
            raise ValueError("pose must be a finite 4x4 matrix and velocity three finite numbers")
        self._init(T, v)

    @property
    def state_dev(self) -> torch.Tensor:
        """the state block: x[16] | P[16][16] | T[16] | int32 counters, as float64 words on the device"""
        return self._buf[:self._words]

    @property
    def pose_dev(self) -> torch.Tensor:
        """[4, 4] float64 on the device: the pose after the last prediction (the initial pose before the first)"""
        return self._buf[self._words:self._words + 16].view(4, 4)

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def predict(self, dt: float) -> None:
        """the IMU-less step over ``dt`` seconds"""
        with torch.cuda.device(self.device):
            _native.check(_native.lib.sps_ukf_predict_dt(self._state_ptr, float(dt), self._Q, self._pred_ptr, self._pinfo_ptr,
                                                         self._stream()))

    def predict_imu(self, samples) -> None:
        """one step per row of ``samples`` [M, 7] (dt, ax, ay, az, gx, gy, gz), uploaded pinned and non-blocking; one launch
        per 256 rows.  M = 0 only refreshes ``pose_dev``."""
        s = checked_imu(samples)
        with torch.cuda.device(self.device):
            st = self._stream()
            if len(s) == 0:
                _native.check(_native.lib.sps_ukf_predict(self._state_ptr, None, 0, self._Q, self._pred_ptr, self._pinfo_ptr, st))
                return
            host = torch.from_numpy(s).pin_memory()
            dev = host.to(self.device, non_blocking=True)
            self._keep = (host, dev)
            for at in range(0, len(s), MAX_IMU):
                n = min(MAX_IMU, len(s) - at)
                _native.check(_native.lib.sps_ukf_predict(self._state_ptr, dev.data_ptr() + at * 56, n, self._Q, self._pred_ptr,
                                                          self._pinfo_ptr, st))

    def _correct(self, T_ptr, gate_ptr):
        with torch.cuda.device(self.device):
            _native.check(_native.lib.sps_ukf_correct(self._state_ptr, T_ptr, gate_ptr, self._R, self._cinfo_ptr, self._stream()))

    def correct(self, pose) -> None:
        """the correction with a 4 x 4 pose: a host matrix (ungated) or a float64 device tensor of 16 entries"""
        if torch.is_tensor(pose) and pose.is_cuda:
            if pose.dtype != torch.float64 or pose.numel() != 16 or not pose.is_contiguous() or pose.device != self.device:
                raise TypeError("a device pose must be 16 contiguous float64 entries on the estimator's device")
            self._keep_pose = pose
            return self._correct(pose.data_ptr(), None)
        T = _pose(pose.numpy() if torch.is_tensor(pose) else pose)
        if T is None or not np.isfinite(T).all():
            raise ValueError("pose must be a finite 4x4 matrix")
        with torch.cuda.device(self.device):
            host = torch.from_numpy(np.ascontiguousarray(T)).pin_memory()
            dev = host.to(self.device, non_blocking=True)
        self._keep_pose = (host, dev)
        self._correct(dev.data_ptr(), None)

    def correct_from(self, pending) -> None:
        """the correction with the pose of a pending registration, read from its device buffer and gated by its status on
        the device: ``T_out`` / status of a PendingPose, ``T_best`` / ``best[1]`` of a PendingPoses or a
        PendingRelocalisation -- the gate of the map update and the carve.  A failed registration leaves the state alone."""
        from .localiser import PendingPose, PendingPoses, PendingRelocalisation
        if not isinstance(pending, (PendingPose, PendingPoses, PendingRelocalisation)):
            raise TypeError("correct_from needs a PendingPose, PendingPoses or PendingRelocalisation")
        out, T_ptr, gate_ptr = pending._pose_on_device()
        if out.device != self.device:
            raise ValueError("the pending registration lives on another device")
        self._keep_pose = out
        self._correct(T_ptr, gate_ptr)

    def _parse(self, h) -> EstimatorState:
        w = self._words
        cnt = h[w - 2:w].view(np.int32)
        pinfo = h[w + 16:w + 18].view(np.int32)
        cstat = int(h[w + 18:w + 19].view(np.int32)[0])
        return EstimatorState(h[:16].copy(), h[16:272].reshape(16, 16).copy(), h[272:288].reshape(4, 4).copy(), cstat,
                              int(pinfo[0]), int(pinfo[1]), int(pinfo[2]), int(cnt[0]), int(cnt[1]), h[w + 19:w + 26].copy())

    def snapshot(self):
        """everything ``state()`` tells, copied to a pinned host buffer behind the work issued so far, without
        synchronising -> a callable that waits for the copy and returns (EstimatorState, predicted pose [4, 4])"""
        with torch.cuda.device(self.device):
            host = torch.empty(self._buf.numel(), dtype=torch.float64).pin_memory()
            host.copy_(self._buf, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())

        def wait():
            ev.synchronize()
            h = host.numpy()
            return self._parse(h), h[self._words:self._words + 16].reshape(4, 4).copy()
        return wait

    def state(self) -> EstimatorState:
        """synchronises: everything about the filter after the work issued so far"""
        return self.snapshot()()[0]
