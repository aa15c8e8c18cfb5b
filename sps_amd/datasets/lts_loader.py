"""The LTS baseline's range-image loader: a drop-in for the reference's ``loader.Loader``
(c_ws/src/inference_model/lts_filter/scripts/loader.py).

The projection runs on the device (sps_lts_project, one launch sequence and one synchronisation); the reference's
attributes and indexing are kept: ``num_slices``, ``window_size``, ``num_windows``, ``.frame`` (numpy f32
[beams, 1024, 4]), ``loader[w] -> (points[N, 3], labels[N])`` with N = beams x window_size, beam-major.  Per cell the
lexicographically largest (x, y, z, s) row wins (np.unique + last write); rows with s == -1 are dropped; a point
outside the image rows (or with a NaN coordinate) raises IndexError for the whole frame, as in the reference.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _native

_PROJECTORS = {}


def projector(device_index: int) -> _native.LtsHandle:
    """A weight-less sps_lts handle of the device (projection only), one per process and device."""
    h = _PROJECTORS.get(device_index)
    if h is None:
        h = _PROJECTORS[device_index] = _native.LtsHandle(device_index, None, 0)
    return h


class Loader:
    def __init__(self, data, lidar: str = 'vlp-16', device=None) -> None:
        assert lidar in {'vlp-16', 'hdl-32'}, 'lidar type should be \'vlp-16\' or \'hdl-32\''
        self.lidar = lidar
        beams, self.window_size, self.num_windows = _native.lts_lidar_info(lidar)
        self.num_slices = 1024
        self.num_beams = beams
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        pts = torch.as_tensor(data)
        if pts.dim() != 2 or pts.shape[1] < 4:
            raise ValueError(f"data must be [n, >=4] (x, y, z, s), got {tuple(pts.shape)}")
        pts = pts[:, :4].to(device=dev, dtype=torch.float32).contiguous()
        N = beams * self.window_size
        self.frame_dev = torch.empty((beams, self.num_slices, 4), dtype=torch.float32, device=dev)
        self.x_dev = torch.empty((self.num_windows, 3, N), dtype=torch.float32, device=dev)
        h = projector(dev.index)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream().cuda_stream
            h.project(pts.data_ptr(), 4, pts.shape[0], _native.LTS_LIDARS[lidar], self.frame_dev.data_ptr(),
                      self.x_dev.data_ptr(), None, st)
            h.check_errors(st)
        self.frame = self.frame_dev.cpu().numpy()

    def __getitem__(self, idx: int):
        w_s = idx * self.window_size
        frame = self.frame[:, w_s: w_s + self.window_size, :].reshape(-1, self.frame.shape[-1])
        return frame[:, :3], frame[:, 3]

    def __len__(self) -> int:
        return self.num_windows
