"""Room-acoustic metrics of impulse-response tensors, measured where the tensors lie (DESIGN.md "IR metrics").

``ir_metrics`` runs ``al_ir_metrics`` (csrc/al_irmetrics.h) over a ``DeviceIRTensor`` in place -- the tensor a ``ShoeboxIRState``
generated, or one ``Renderer.upload_irs`` put into HBM -- and downloads one ``(rows, 16)`` float64 table: per row the Schroeder
energy-decay curve's reverberation times (EDT, T20, T30), the direct-to-reverberant ratio, the clarities C50 / C80, D50, the centre
time and the decay the row has room for.  The definition is the header comment of ``al_ir_metrics`` in
include/audiblelight_hip.h.  No noise-floor compensation is applied (no Lundeby truncation, no subtraction): a measured IR with a
noise floor reads long, and ``dyn_db`` -- the level of the curve's last sample under its level at the direct sound -- says how much
decay the row had room for.

``ir_band_metrics`` gives the same per OCTAVE BAND (DESIGN.md "IR metrics: octave bands"): ``al_ir_band_metrics`` splits every row into
the bands of ``shoebox.band_filters`` on the device and measures every band row; ``ir_band_rows`` downloads the band rows themselves.
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


def _view(irs, renderer):
    """``(renderer, buffer, stride_c, pitch, (C, N, L))`` of a ``shoebox.DeviceIRTensor`` as it lies, or of a host ``(C, N, L)`` float32 /
    float64 array uploaded by ``Renderer.upload_irs``."""
    from . import shoebox, synthesize

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
    return r, buf, stride_c, pitch, tuple(int(v) for v in shape)


def ir_metrics(irs, sample_rate, renderer=None, edc: bool = False) -> IRMetrics:
    """The metrics of every row of ``irs``: a ``shoebox.DeviceIRTensor`` (measured in place: no copy, and the tensor is not
    downloaded), or a host ``(C, N, L)`` float32 / float64 array (uploaded by ``Renderer.upload_irs``).  One download of the
    ``(rows, 16)`` table -- and of the ``(rows, n_knots)`` curve with ``edc=True`` -- is the call's only synchronisation."""
    fs = check_rate(sample_rate)
    r, buf, stride_c, pitch, (c, n, length) = _view(irs, renderer)
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


# ----------------------------------------------------------------------------- per octave band
@dataclass
class IRBandMetrics:
    """``IRMetrics`` per band: one ``(C, N, B)`` float64 array per column of ``al_ir_metrics`` (``COLUMNS``), ``edc_knots``
    ``(C, N, B, n_knots)`` or None, the band ``centres`` in Hz, the half length ``half`` of the band filters and the sample rate.  ``t0``
    of a band is the peak of the band row: a zero-phase filter rings before the direct sound."""
    centres: tuple
    half: int
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
    def from_table(cls, table: np.ndarray, shape, bands, sample_rate: float, edc_knots: Optional[np.ndarray] = None) -> "IRBandMetrics":
        table = np.asarray(table, dtype=np.float64).reshape(shape[0], shape[1], len(bands.centres), len(COLUMNS))
        return cls(**{name: np.ascontiguousarray(table[..., i]) for i, name in enumerate(COLUMNS)}, centres=tuple(bands.centres),
                   half=int(bands.half), sample_rate=float(sample_rate), edc_knots=edc_knots)

    def table(self) -> np.ndarray:
        """The ``(C, N, B, 16)`` table the columns came from."""
        return np.stack([getattr(self, name) for name in COLUMNS], axis=-1)

    def band(self, b: int) -> IRMetrics:
        """Band ``b`` alone, as the ``IRMetrics`` of its band rows."""
        if isinstance(b, (bool, np.bool_)) or not isinstance(b, (int, np.integer)) or not 0 <= b < len(self.centres):
            raise IndexError(f"band {b!r} of {len(self.centres)}")
        return IRMetrics(**{name: np.ascontiguousarray(getattr(self, name)[:, :, b]) for name in COLUMNS}, sample_rate=self.sample_rate,
                         edc_knots=None if self.edc_knots is None else np.ascontiguousarray(self.edc_knots[:, :, b]))

    def to_dict(self) -> dict:
        """As ``IRMetrics.to_dict``: plain lists, None for what is not finite, integers in the whole-number columns."""
        d = {name: _plain(getattr(self, name), name in INTEGER_COLUMNS) for name in COLUMNS}
        d.update(centres=[float(v) for v in self.centres], half=int(self.half), sample_rate=self.sample_rate,
                 edc_knots=None if self.edc_knots is None else _plain(self.edc_knots, False))
        return d

    @classmethod
    def from_dict(cls, d: dict) -> "IRBandMetrics":
        knots = d.get("edc_knots")
        return cls(**{name: _array(d[name]) for name in COLUMNS}, centres=tuple(float(v) for v in d["centres"]), half=int(d["half"]),
                   sample_rate=float(d["sample_rate"]), edc_knots=None if knots is None else _array(knots))


def check_measure_bands(bands, sample_rate: float):
    """``bands`` of ``ir_band_metrics`` as a ``shoebox.ShoeboxBands`` (None: the six octave centres, ``half`` 512), its centres and
    ``half`` held against the sample rate by the generator's checks (ValueError)."""
    from . import shoebox

    if bands is None:
        bands = shoebox.ShoeboxBands()
    elif isinstance(bands, dict):
        try:
            bands = shoebox.ShoeboxBands.from_dict(bands)
        except (TypeError, ValueError):
            raise ValueError("bands: centres must be numbers")
    if not isinstance(bands, shoebox.ShoeboxBands):
        raise ValueError("bands must be a ShoeboxBands, its dictionary or None")
    shoebox._centres(bands.centres, sample_rate)
    shoebox._half(bands.half)
    return bands


def _filters_device(renderer, bands, sample_rate: float):
    from . import shoebox

    return renderer.mem.upload(shoebox.band_filters(bands.centres, sample_rate, bands.half).reshape(-1))


def band_metrics_device(renderer, irs_ptr: int, n_capsules: int, n_sources: int, stride_c: int, pitch: int, ir_len: int,
                        sample_rate: float, filters, n_bands: int, half: int, edc: bool = False, workspace_cap: int = 1 << 30):
    """``al_ir_band_metrics`` over the tensor at device address ``irs_ptr`` with the device filter table ``filters``: (table buffer
    (rows * n_bands * 16 float64), knots buffer or None), on the device, enqueued on the renderer's stream.  The workspace is allocated
    here: what all rows need, at most ``workspace_cap`` bytes and at least one row's.  No synchronisation."""
    mem, lib = renderer.mem, renderer.lib
    rows = int(n_capsules) * int(n_sources)
    per_row = lib.call("al_ir_band_metrics_workspace_bytes", n_bands, ir_len)
    if per_row <= 0:
        raise ValueError(f"al_ir_band_metrics_workspace_bytes refused {n_bands} bands, ir_len = {ir_len}")
    nbytes = max(1, min(rows, int(workspace_cap) // per_row)) * per_row
    workspace = mem.empty(nbytes // 8, np.float64)
    out = mem.empty(rows * n_bands * len(COLUMNS), np.float64)
    knots = mem.empty(rows * n_bands * n_knots_of(ir_len), np.float64) if edc else None
    lib.call("al_ir_band_metrics", irs_ptr, n_capsules, n_sources, stride_c, pitch, ir_len, float(sample_rate), mem.ptr(filters), n_bands,
             half, mem.ptr(workspace), nbytes, mem.ptr(out), mem.ptr(knots) if edc else None, mem.stream())
    return out, knots


def ir_band_metrics(irs, sample_rate, bands=None, renderer=None, edc: bool = False, workspace_cap: int = 1 << 30) -> IRBandMetrics:
    """The metrics of every row of ``irs`` in every band of ``bands`` (a ``shoebox.ShoeboxBands`` or its dictionary; None: the six
    octave centres at ``half`` 512).  ``irs`` as ``ir_metrics`` takes it: a ``DeviceIRTensor`` is split and measured where it lies.
    The band filters are ``shoebox.band_filters`` at the sample rate, uploaded per call; ``workspace_cap`` bounds the bytes of band
    rows held at a time (the rows are walked in passes; never less than one row's share).  The tables are the only download."""
    from . import shoebox

    fs = check_rate(sample_rate)
    bands = check_measure_bands(bands, fs)
    shoebox._check_workspace_cap(workspace_cap)
    r, buf, stride_c, pitch, (c, n, length) = _view(irs, renderer)
    n_bands = len(bands.centres)
    out, knots = band_metrics_device(r, r.mem.ptr(buf), c, n, stride_c, pitch, length, fs, _filters_device(r, bands, fs), n_bands,
                                     bands.half, edc, workspace_cap)
    table = np.asarray(r.mem.download(out))[: c * n * n_bands * len(COLUMNS)]
    curve = None
    if edc:
        k = n_knots_of(length)
        curve = np.array(np.asarray(r.mem.download(knots))[: c * n * n_bands * k].reshape(c, n, n_bands, k))
    return IRBandMetrics.from_table(table, (c, n), bands, fs, curve)


def ir_band_rows(irs, sample_rate, bands=None, renderer=None) -> np.ndarray:
    """The band rows ``al_ir_band_split`` makes of ``irs`` (as ``ir_band_metrics`` takes it), downloaded: ``(C, N, B, L)`` float32, for
    plots and tests.  B times the tensor's bytes come to the host."""
    fs = check_rate(sample_rate)
    bands = check_measure_bands(bands, fs)
    r, buf, stride_c, pitch, (c, n, length) = _view(irs, renderer)
    n_bands, out_pitch = len(bands.centres), (length + 3) // 4 * 4
    out = r.mem.empty(c * n * n_bands * out_pitch, np.float32)
    r.lib.call("al_ir_band_split", r.mem.ptr(buf), c, n, stride_c, pitch, length, r.mem.ptr(_filters_device(r, bands, fs)), n_bands,
               bands.half, r.mem.ptr(out), out_pitch, r.mem.stream())
    flat = np.asarray(r.mem.download(out))[: c * n * n_bands * out_pitch]
    return np.ascontiguousarray(flat.reshape(c, n, n_bands, out_pitch)[..., :length])


def state_band_metrics(state, sample_rate, alias=None, bands=None, edc: bool = False, renderer=None) -> dict:
    """``{alias: IRBandMetrics}`` of a state's IR tensors as they lie."""
    irs = state.irs
    if alias is not None and alias not in irs:
        raise KeyError(f"no microphone with alias {alias}")
    renderer = renderer or getattr(state, "renderer", None)
    return {k: ir_band_metrics(v, sample_rate, bands, renderer, edc) for k, v in irs.items() if alias is None or k == alias}


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


def _absorption_bands(room, betas, air):
    from . import shoebox

    betas = np.asarray(betas, dtype=np.float64)
    if betas.ndim != 2 or betas.shape[0] != 6:
        raise ValueError(f"betas must have shape (6, bands), not {betas.shape}")
    air = np.zeros(betas.shape[1]) if air is None else shoebox.check_air(air, betas.shape[1])
    parts = [_absorption(room, betas[:, b]) for b in range(betas.shape[1])]
    return parts, air


def sabine_rt60_bands(room, betas, c: float = 343.0, air=None) -> np.ndarray:
    """Sabine's time per band, ``(B,)``, of a room with reflection coefficients ``betas`` ``(6, B)``: 24 ln(10) V / (c (A_b + 8 m_b V)),
    ``air`` the amplitude attenuation ``m_b`` of the air in Np/m (a number or one per band; None: 0)."""
    parts, air = _absorption_bands(room, betas, air)
    with np.errstate(divide="ignore"):
        return np.array([24.0 * np.log(10.0) * v / np.float64(c * (a + 8.0 * m * v)) for (v, _, a), m in zip(parts, air)])


def eyring_rt60_bands(room, betas, c: float = 343.0, air=None) -> np.ndarray:
    """Eyring's per band: 24 ln(10) V / (c (-S ln(1 - mean alpha_b) + 8 m_b V)); a band whose mean absorption is 1 gives 0."""
    parts, air = _absorption_bands(room, betas, air)
    out = []
    for (v, surface, a), m in zip(parts, air):
        mean = a / surface
        with np.errstate(divide="ignore"):
            out.append(0.0 if mean >= 1.0 else 24.0 * np.log(10.0) * v / np.float64(c * (-surface * np.log1p(-max(mean, 0.0)) + 8.0 * m * v)))
    return np.array(out)
