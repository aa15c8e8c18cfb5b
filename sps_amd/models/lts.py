"""The LTS baseline's regressor on the MI355X: a drop-in for the reference's ``transformer.SPCTReg``
(c_ws/src/inference_model/lts_filter/scripts/transformer.py).

``SPCTReg`` holds its parameters under the reference's state_dict keys and shapes (so
``model.load_state_dict(torch.load(p)['model_state_dict'])`` works unchanged) and runs ``forward(x[B, 3, N]) ->
[B, 1, N]`` (sigmoid applied) through the HIP kernels of libsps_hip.so (sps_lts_forward): BatchNorm in eval mode,
dropout = identity.  As in the reference, ``sa*.q_conv.weight`` IS ``sa*.k_conv.weight`` (one Parameter): a
state_dict with two different values loads the ``k_conv`` one.  No CPU fallback: a CPU tensor raises.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from .. import _native
from .models import _require_device_tensor

TAPS = ("embedding", "sa1", "sa2", "sa3", "sa4", "max", "mean")


class _Embedding(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv1d(3, 128, 1, bias=False)
        self.conv2 = nn.Conv1d(128, 128, 1, bias=False)
        self.bn1 = nn.BatchNorm1d(128)
        self.bn2 = nn.BatchNorm1d(128)


class _OA(nn.Module):
    def __init__(self, c=128):
        super().__init__()
        self.q_conv = nn.Conv1d(c, c // 4, 1, bias=False)
        self.k_conv = nn.Conv1d(c, c // 4, 1, bias=False)
        self.q_conv.weight = self.k_conv.weight           # shared, as in the reference
        self.v_conv = nn.Conv1d(c, c, 1)
        self.trans_conv = nn.Conv1d(c, c, 1)
        self.after_norm = nn.BatchNorm1d(c)


class SPCTReg(nn.Module):
    def __init__(self):
        super().__init__()
        self.embedding = _Embedding()
        self.sa1, self.sa2, self.sa3, self.sa4 = _OA(), _OA(), _OA(), _OA()
        self.linear1 = nn.Sequential(nn.Conv1d(512, 2048, 1, bias=False), nn.BatchNorm1d(2048), nn.LeakyReLU(0.2))
        self.linear2 = nn.Sequential(nn.Conv1d(2048 * 3, 512, 1), nn.BatchNorm1d(512), nn.SiLU(), nn.Dropout(0.2))
        self.linear3 = nn.Sequential(nn.Conv1d(512, 256, 1), nn.BatchNorm1d(256), nn.SiLU(), nn.Dropout(0.2))
        self.convs = nn.Conv1d(256, 1, 1)
        self.sigmoid = nn.Sigmoid()
        self._handles = {}       # device index -> (state key, _native.LtsHandle)

    # ---- parameters -> native handle -------------------------------------------------------------------------------
    def _state_key(self, sd):
        return tuple((k, v.data_ptr(), v._version) for k, v in sd.items())

    def pack(self) -> np.ndarray:
        """The native weight blob (sps_lts_tensor_info order) of the current parameters."""
        sd = self.state_dict()
        blob = np.zeros(_native.lib.sps_lts_numel(), dtype=np.float32)
        for name, off, numel, shape in _native.lts_layout():
            t = sd[name].detach().to("cpu", torch.float32).reshape(-1)
            if t.numel() != numel:
                raise ValueError(f"{name}: {t.numel()} values, the native layout expects {numel} {shape}")
            blob[off: off + numel] = t.numpy()
        return blob

    def handle(self, device_index: int) -> _native.LtsHandle:
        sd = self.state_dict()
        key = self._state_key(sd)
        cached = self._handles.get(device_index)
        if cached is not None and cached[0] == key:
            return cached[1]
        blob = self.pack()
        with torch.cuda.device(device_index):
            torch.cuda.current_stream().synchronize()     # a forward in flight may still read the old handle
            h = _native.LtsHandle(device_index, blob.ctypes.data, blob.size)
        self._handles[device_index] = (key, h)
        return h

    def _apply(self, fn, *args, **kwargs):
        self._handles = {}
        return super()._apply(fn, *args, **kwargs)

    # ---- forward ---------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, x: torch.Tensor, taps: dict | None = None) -> torch.Tensor:
        _require_device_tensor(x, "SPCTReg input")
        if x.dim() != 3 or x.shape[1] != 3:
            raise ValueError(f"SPCTReg expects [B, 3, N], got {tuple(x.shape)}")
        B, _, N = x.shape
        x = x.to(torch.float32).contiguous()
        dev = x.device.index if x.device.index is not None else torch.cuda.current_device()
        h = self.handle(dev)
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream().cuda_stream
            scores = torch.empty((B, 1, N), dtype=torch.float32, device=x.device)
            h.forward(x.data_ptr(), B, N, scores.data_ptr(), st)
            if taps is not None:
                for i, name in enumerate(TAPS):
                    r, c = h.tap_shape(i)
                    t = torch.empty((r, c), dtype=torch.float32, device=x.device)
                    h.tap(i, t.data_ptr(), st)
                    taps[name] = t.view(B, N, c).permute(0, 2, 1) if i < 5 else t
        return scores
