"""Room-acoustic metrics of impulse-response tensors, measured where the tensors lie (DESIGN.md "IR metrics").

``ir_metrics`` runs ``al_ir_metrics`` (csrc/al_irmetrics.h) over a ``DeviceIRTensor`` in place -- the tensor a ``ShoeboxIRState``
generated, or one ``Renderer.upload_irs`` put into HBM -- and downloads one ``(rows, 16)`` float64 table: per row the Schroeder
energy-decay curve's reverberation times (EDT, T20, T30), the direct-to-reverberant ratio, the clarities C50 / C80, D50, the centre
time and the decay the row has room for.  The definition is the header comment of ``al_ir_metrics`` in
include/audiblelight_hip.h.  No noise-floor compensation is applied (no Lundeby truncation, no subtraction): a measured IR with a
noise floor reads long, and ``dyn_db`` -- the level of the curve's last sample under its level at the direct sound -- says how much
decay the row had room for.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

COLUMNS = ("bad", "energy", "t0", "peak", "drr_db", "c50_db", "c80_db", "d50", "ts", "edt", "t20", "t30", "n_edt", "n_t20", "n_t30",
           "dyn_db")
INTEGER_COLUMNS = ("bad", "t0", "n_edt", "n_t20", "n_t30")       # whole numbers (NaN where the row has none): integers in to_dict()
KNOT_SPACING = 256                                                # samples between two knots of the curve (shoebox.KNOT_SPACING)


def n_knots_of(ir_len: int) -> int:
    return (int(ir_len) - 1) // KNOT_SPACING + 2


def _plain(values: np.ndarray, integer: bool):
    """A float64 array as nested lists that survive strict JSON: non-finite values as None, whole-number columns as integers."""
    flat = [None if not np.isfinite(v) else (int(v) if integer else float(v)) for v in values.reshape(-1)]
    return np.array(flat, dtype=object).reshape(values.shape).tolist()


def _array(nested) -> np.ndarray:
    """The inverse of ``_plain`` up to the kind of non-finite value: None comes back as NaN."""
    a = np.array(nested, dtype=object)
    out = np.full(a.shape, np.nan)
    keep = np.not_equal(a, None)
    out[keep] = a[keep].astype(np.float64)
    return out


@dataclass
class IRMetrics:
    """One ``(C, N)`` float64 array per column of ``al_ir_metrics`` (``COLUMNS``), ``edc_knots`` ``(C, N, n_knots)`` -- E at every
    256th sample, the last knot 0 -- or None, and the sample rate.  Times are seconds, levels dB."""
    bad: np.ndarray
    energy: np.ndarray
    t0: np.ndarray
    peak: np.ndarray
    drr_db: np.ndarray
    c50_db: np.ndarray
    c80_db: np.ndarray
    d50: np.ndarray
    ts: np.ndarray
    edt: np.ndarray
    t20: np.ndarray
    t30: np.ndarray
    n_edt: np.ndarray
    n_t20: np.ndarray
    n_t30: np.ndarray
    dyn_db: np.ndarray
    sample_rate: float
    edc_knots: Optional[np.ndarray] = None

    @classmethod
    def from_table(cls, table: np.ndarray, shape, sample_rate: float, edc_knots: Optional[np.ndarray] = None) -> "IRMetrics":
        table = np.asarray(table, dtype=np.float64).reshape(shape[0], shape[1], len(COLUMNS))
        return cls(**{name: np.ascontiguousarray(table[:, :, i]) for i, name in enumerate(COLUMNS)}, sample_rate=float(sample_rate),
                   edc_knots=edc_knots)

    def table(self) -> np.ndarray:
        """The ``(C, N, 16)`` table the columns came from."""
        return np.stack([getattr(self, name) for name in COLUMNS], axis=-1)

    def to_dict(self) -> dict:
        """Plain lists; non-finite values (the NaN of a fit the row has no room for, the +inf of a window past the row's end) are
        written as None, so the dictionary survives ``json.dumps(..., allow_nan=False)``."""
        d = {name: _plain(getattr(self, name), name in INTEGER_COLUMNS) for name in COLUMNS}
        d["sample_rate"] = self.sample_rate
        d["edc_knots"] = None if self.edc_knots is None else _plain(self.edc_knots, False)
        return d

    @classmethod
    def from_dict(cls, d: dict) -> "IRMetrics":
        """``to_dict`` read back: every None is NaN (the dictionary does not keep which non-finite value it was)."""
        knots = d.get("edc_knots")
        return cls(**{name: _array(d[name]) for name in COLUMNS}, sample_rate=float(d["sample_rate"]),
                   edc_knots=None if knots is None else _array(knots))


def check_rate(sample_rate) -> float:
    if isinstance(sample_rate, (bool, np.bool_)) or not isinstance(sample_rate, (int, float, np.integer, np.floating)):
        raise ValueError("sample_rate must be a number")
    fs = float(sample_rate)
    if not (np.isfinite(fs) and fs > 0.0):
        raise ValueError("sample_rate must be finite and positive")
    return fs


def metrics_device(renderer, irs_ptr: int, n_capsules: int, n_sources: int, stride_c: int, pitch: int, ir_len: int, sample_rate: float,
                   edc: bool = False):
    """``al_ir_metrics`` over the tensor at device address ``irs_ptr``: (table buffer (rows * 16 float64), knots buffer or None),
    both on the device, enqueued on the renderer's stream.  No synchronisation."""
    mem, lib = renderer.mem, renderer.lib
    rows = int(n_capsules) * int(n_sources)
    nbytes = lib.call("al_ir_metrics_workspace_bytes", n_capsules, n_sources, ir_len)
    workspace = mem.empty((nbytes + 7) // 8, np.float64)
    out = mem.empty(rows * len(COLUMNS), np.float64)
    knots = mem.empty(rows * n_knots_of(ir_len), np.float64) if edc else None
    lib.call("al_ir_metrics", irs_ptr, n_capsules, n_sources, stride_c, pitch, ir_len, float(sample_rate), mem.ptr(workspace), nbytes,
             mem.ptr(out), mem.ptr(knots) if edc else None, mem.stream())
    return out, knots


def ir_metrics(irs, sample_rate, renderer=None, edc: bool = False) -> IRMetrics:
    """The metrics of every row of ``irs``: a ``shoebox.DeviceIRTensor`` (measured in place: no copy, and the tensor is not
    downloaded), or a host ``(C, N, L)`` float32 / float64 array (uploaded by ``Renderer.upload_irs``).  One download of the
    ``(rows, 16)`` table -- and of the ``(rows, n_knots)`` curve with ``edc=True`` -- is the call's only synchronisation."""
    from . import shoebox, synthesize

    fs = check_rate(sample_rate)
    if isinstance(irs, shoebox.DeviceIRTensor):
        r = renderer or irs.renderer
        if r is not irs.renderer and r.mem is not irs.renderer.mem:
            raise ValueError("the tensor lives in another renderer's memory")
        shape = irs.shape
        if len(shape) != 3:
            raise ValueError(f"irs must have shape (C, N, L), got {shape}")
        if min(shape) < 1:
            raise ValueError(f"irs must not be empty, got shape {shape}")
        buf, (stride_c, pitch) = irs.result()
        if irs.ready is not None and hasattr(r.mem, "torch"):     # generated on another stream, perhaps
            r.mem.torch.cuda.current_stream(r.mem.device).wait_event(irs.ready)
    else:
        host = np.asarray(irs)
        if host.ndim != 3:
            raise ValueError(f"irs must have shape (C, N, L), got {host.shape}")
        if host.size == 0:
            raise ValueError(f"irs must not be empty, got shape {host.shape}")
        if host.dtype not in (np.float32, np.float64):
            raise ValueError(f"irs must be float32 or float64, got {host.dtype}")
        r = renderer or synthesize.get_renderer()
        shape = host.shape
        buf, (stride_c, pitch) = r.upload_irs(host)
    c, n, length = (int(v) for v in shape)
    out, knots = metrics_device(r, r.mem.ptr(buf), c, n, stride_c, pitch, length, fs, edc)
    table = np.asarray(r.mem.download(out))[: c * n * len(COLUMNS)]
    curve = None
    if edc:
        k = n_knots_of(length)
        curve = np.array(np.asarray(r.mem.download(knots))[: c * n * k].reshape(c, n, k))
    return IRMetrics.from_table(table, (c, n), fs, curve)


def state_metrics(state, sample_rate, alias=None, edc: bool = False, renderer=None) -> dict:
    """``{alias: IRMetrics}`` of a state's IR tensors as they lie (``state.irs``: a ``ShoeboxIRState`` raises before ``simulate()``)."""
    irs = state.irs
    if alias is not None and alias not in irs:
        raise KeyError(f"no microphone with alias {alias}")
    renderer = renderer or getattr(state, "renderer", None)
    return {k: ir_metrics(v, sample_rate, renderer, edc) for k, v in irs.items() if alias is None or k == alias}


# ----------------------------------------------------------------------------- what the room was asked for
def _absorption(room, betas):
    room = np.asarray(room, dtype=np.float64)
    betas = np.asarray(betas, dtype=np.float64)
    lx, ly, lz = room
    areas = np.array([ly * lz, ly * lz, lx * lz, lx * lz, lx * ly, lx * ly])
    alpha = 1.0 - betas ** 2
    return float(np.prod(room)), float(areas.sum()), float((areas * alpha).sum())


def sabine_rt60(room, betas, c: float = 343.0) -> float:
    """Sabine's reverberation time of a rectangular room with six broadband reflection coefficients: 24 ln(10) V / (c A)."""
    volume, _, absorbed = _absorption(room, betas)
    return 24.0 * np.log(10.0) * volume / (c * absorbed) if absorbed > 0.0 else float("inf")


def eyring_rt60(room, betas, c: float = 343.0) -> float:
    """Eyring's: 24 ln(10) V / (-c S ln(1 - mean alpha))."""
    volume, surface, absorbed = _absorption(room, betas)
    mean = absorbed / surface
    if mean <= 0.0:
        return float("inf")
    return 0.0 if mean >= 1.0 else 24.0 * np.log(10.0) * volume / (-c * surface * np.log1p(-mean))
