"""Shoebox room impulse responses generated on the device (image-source method, csrc/al_ism.h; DESIGN.md "Shoebox IRs").

``shoebox_irs_device`` makes the one call of the C ABI (``al_ism_shoebox``): the (C, N, ir_len) tensor of a rectangular room is
born in HBM in the layout ``Renderer.prepare(plan, clips, irs, ir_strides)`` reads and never crosses PCIe.  ``DeviceIRTensor`` wraps
it as a lazy array: the render path takes its buffer (``result()``), a host consumer downloads it once.  Omnidirectional point
capsules, frequency-independent walls, no diffuse tail, no air absorption.  Without ``max_order`` the cost grows as
``ir_len**3 / (Lx * Ly * Lz)`` per (capsule, source) pair.
"""
from __future__ import annotations

import ctypes as ct
from typing import Optional, Sequence, Tuple

import numpy as np

SPEED_OF_SOUND = 343.0
MIN_DISTANCE = 0.01     # metres between a source and a capsule


def betas_from_absorption(alpha) -> np.ndarray:
    """Reflection coefficients ``sqrt(1 - alpha)`` of energy absorption coefficients in [0, 1]."""
    alpha = np.asarray(alpha, dtype=np.float64)
    if not np.all(np.isfinite(alpha)) or np.any(alpha < 0.0) or np.any(alpha > 1.0):
        raise ValueError("absorption coefficients must be in [0, 1]")
    return np.sqrt(1.0 - alpha)


def _room(room) -> np.ndarray:
    room = np.asarray(room, dtype=np.float64)
    if room.shape != (3,) or not np.all(np.isfinite(room)) or np.any(room <= 0.0):
        raise ValueError("room must be three finite positive dimensions (Lx, Ly, Lz) in metres")
    return room


def betas_from_rt60(room, rt60: float, c: float = SPEED_OF_SOUND) -> np.ndarray:
    """Six equal reflection coefficients for a reverberation time, by Sabine's law read backwards:
    ``alpha = 24 ln(10) V / (c S rt60)``.  Raises when the room cannot be that dry (``alpha > 1``)."""
    room = _room(room)
    if not (np.isfinite(rt60) and rt60 > 0.0 and np.isfinite(c) and c > 0.0):
        raise ValueError("rt60 and c must be finite and positive")
    volume = float(np.prod(room))
    surface = 2.0 * float(room[0] * room[1] + room[0] * room[2] + room[1] * room[2])
    alpha = 24.0 * np.log(10.0) * volume / (c * surface * float(rt60))
    if alpha > 1.0:
        raise ValueError(f"rt60 = {rt60} s needs an absorption coefficient of {alpha:.3f} > 1 in this room (Sabine)")
    return np.full(6, np.sqrt(1.0 - alpha))


def _points(points, room: np.ndarray, what: str) -> np.ndarray:
    points = np.ascontiguousarray(points, dtype=np.float64)
    if points.ndim != 2 or points.shape[1] != 3 or points.shape[0] < 1:
        raise ValueError(f"{what} must have shape (n >= 1, 3)")
    if not np.all(np.isfinite(points)):
        raise ValueError(f"{what} must be finite")
    if np.any(points <= 0.0) or np.any(points >= room[None, :]):
        raise ValueError(f"every point of {what} must lie strictly inside the room")
    return points


def pitch_of(ir_len: int) -> int:
    return (int(ir_len) + 3) // 4 * 4


def check_arguments(room, betas, sources, capsules, ir_len, sample_rate, c=SPEED_OF_SOUND, max_order=None):
    """The host-side validation of ``shoebox_irs_device`` (ValueError); returns the arguments as the call takes them."""
    room = _room(room)
    betas = np.ascontiguousarray(betas, dtype=np.float64)
    if betas.shape != (6,) or not np.all(np.isfinite(betas)) or np.any(betas < 0.0) or np.any(betas > 1.0):
        raise ValueError("betas must be six reflection coefficients (x0, x1, y0, y1, z0, z1) in [0, 1]")
    sources, capsules = _points(sources, room, "sources"), _points(capsules, room, "capsules")
    if int(ir_len) != ir_len or ir_len < 1:
        raise ValueError("ir_len must be an integer >= 1")
    if not (np.isfinite(sample_rate) and sample_rate > 0.0 and np.isfinite(c) and c > 0.0):
        raise ValueError("sample_rate and c must be finite and positive")
    if max_order is not None and (int(max_order) != max_order or max_order < 0):
        raise ValueError("max_order must be None or an integer >= 0")
    gap = np.sqrt(((capsules[:, None, :] - sources[None, :, :]) ** 2).sum(axis=2))
    if gap.min() < MIN_DISTANCE:
        raise ValueError(f"every source must be at least {MIN_DISTANCE} m from every capsule (closest: {gap.min():.4g} m)")
    return room, betas, sources, capsules, int(ir_len), float(sample_rate), float(c), -1 if max_order is None else int(max_order)


def shoebox_irs_device(renderer, room, betas, sources, capsules, ir_len: int, sample_rate: float, c: float = SPEED_OF_SOUND,
                       max_order: Optional[int] = None):
    """The IRs of ``sources`` (N, 3) at ``capsules`` (C, 3) in the room ``(Lx, Ly, Lz)`` with wall reflection coefficients
    ``betas = (x0, x1, y0, y1, z0, z1)``: ``(device buffer, (stride_c, stride_n), ir_len)`` as ``ingest.pack_ragged_irs`` returns
    it, enqueued on the renderer's stream.  The two coordinate tables are all that is uploaded."""
    room, betas, sources, capsules, ir_len, fs, c, order = check_arguments(room, betas, sources, capsules, ir_len, sample_rate, c,
                                                                          max_order)
    mem, lib = renderer.mem, renderer.lib
    n, n_cap, pitch = len(sources), len(capsules), pitch_of(ir_len)
    src_dev, cap_dev = mem.upload(sources.reshape(-1)), mem.upload(capsules.reshape(-1))
    out = mem.empty(n_cap * n * pitch)
    lib.call("al_ism_shoebox", mem.ptr(src_dev), n, mem.ptr(cap_dev), n_cap, room.ctypes.data_as(ct.POINTER(ct.c_double)),
             betas.ctypes.data_as(ct.POINTER(ct.c_double)), c, fs, order, ir_len, pitch, mem.ptr(out), mem.stream())
    return out, (n * pitch, pitch), ir_len


class DeviceIRTensor:
    """A (C, N, ir_len) float32 IR tensor that lives in HBM with rows of ``pitch`` floats.  ``result()`` hands the render path the
    buffer and its strides (``Renderer.prepare`` accepts anything with ``result()``); ``np.asarray(t)`` and ``t[...]`` download
    it once and keep the host copy.  ``ready``: an event recorded behind the generating launch (torch memory provider) for a
    consumer on another stream, else None."""

    dtype = np.dtype(np.float32)
    ndim = 3

    def __init__(self, renderer, buffer, strides: Tuple[int, int], shape: Tuple[int, int, int]):
        self.renderer, self.buffer, self.strides_floats = renderer, buffer, (int(strides[0]), int(strides[1]))
        self.shape = tuple(int(v) for v in shape)
        self._host = None
        mem = renderer.mem
        self.ready = None
        if hasattr(mem, "torch"):
            self.ready = mem.torch.cuda.Event()
            self.ready.record(mem.torch.cuda.current_stream(mem.device))

    @property
    def size(self) -> int:
        return self.shape[0] * self.shape[1] * self.shape[2]

    @property
    def nbytes(self) -> int:
        return 4 * self.size

    def __len__(self) -> int:
        return self.shape[0]

    def result(self):
        return self.buffer, self.strides_floats

    def host(self) -> np.ndarray:
        if self._host is None:
            c, n, l = self.shape
            pitch = self.strides_floats[1]
            flat = np.asarray(self.renderer.mem.download(self.buffer))[: c * n * pitch]
            host = np.ascontiguousarray(flat.reshape(c, n, pitch)[:, :, :l])
            host.flags.writeable = False
            self._host = host
        return self._host

    def __array__(self, dtype=None, copy=None):
        host = self.host()
        return host if dtype is None or np.dtype(dtype) == host.dtype else host.astype(dtype)

    def __getitem__(self, key):
        return self.host()[key]


def concatenate_sources(tensors: Sequence) -> object:
    """Several IR tensors with equal capsule count and length joined along the source axis (``batch.merge_jobs``): on the device
    when every one is a ``DeviceIRTensor`` of one renderer and pitch, else as a float32 host array."""
    if len(tensors) == 1 and isinstance(tensors[0], DeviceIRTensor):
        return tensors[0]
    first = tensors[0]
    if all(isinstance(t, DeviceIRTensor) and t.renderer is first.renderer and t.strides_floats[1] == first.strides_floats[1]
           and t.strides_floats[0] == t.shape[1] * t.strides_floats[1] for t in tensors):
        c, l, pitch = first.shape[0], first.shape[2], first.strides_floats[1]
        torch = getattr(first.renderer.mem, "torch", None)
        views = [t.buffer[: c * t.shape[1] * pitch].reshape(c, t.shape[1], pitch) for t in tensors]
        if torch is not None:
            cur = torch.cuda.current_stream(first.renderer.mem.device)
            for t in tensors:
                if t.ready is not None:
                    cur.wait_event(t.ready)
            joined = torch.cat(views, dim=1).reshape(-1)
        else:
            joined = np.concatenate(views, axis=1).reshape(-1)
        n = sum(t.shape[1] for t in tensors)
        return DeviceIRTensor(first.renderer, joined, (n * pitch, pitch), (c, n, l))
    return np.concatenate([np.asarray(t, dtype=np.float32) for t in tensors], axis=1)
