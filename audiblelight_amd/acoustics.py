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

``ir_pair_metrics`` measures PAIRS of rows (DESIGN.md "IR metrics: channel pairs"): ``al_ir_pair_metrics`` correlates the two rows of
every (capsule pair, emitter) over lags of +-``max_lag`` samples in the early 80 ms, the late remainder and the whole response, and
gives the inter-aural cross-correlation coefficients of ISO 3382-1 Annex B, the lag of the peak (ITD / TDOA) and the level
difference; ``ir_pair_band_metrics`` the same per octave band.
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


# ----------------------------------------------------------------------------- pairs of rows: IACC, ITD, ILD
PAIR_WINDOWS = ("e", "l", "a")                                    # early [T0, T0 + 80 ms), late (from there on), all
PAIR_COLUMNS = ("bad", "t0") + tuple(f"{name}_{w}" for w in PAIR_WINDOWS for name in ("peak", "lag", "ild_db", "exx", "eyy"))
PAIR_INTEGER_COLUMNS = ("bad", "t0", "lag_e", "lag_l", "lag_a")
MAX_PAIR_LAG = 1024                                               # csrc/al_irmetrics.h IRP_MAX_LAG
_PAIR_TILE = 1024                                                 # csrc/al_irmetrics.h IRP_TILE


@dataclass
class IRPairMetrics:
    """One ``(P, N)`` float64 array per column of ``al_ir_pair_metrics`` (``PAIR_COLUMNS``) -- ``(P, N, B)`` from
    ``ir_pair_band_metrics``, which also sets ``centres`` and ``half`` --, the ``(P, 2)`` capsule ``pairs``, ``max_lag`` in samples and
    the sample rate.  ``peak_*`` is the signed peak of the normalised cross-correlation of the window (early, late, all), ``lag_*`` its
    lag in samples (positive: the sound reaches the pair's first capsule first), ``ild_db_*`` the level of the first capsule over the
    second.  ``xcorr``: ``(P, N, 2, 2 max_lag + 1)`` (``(P, N, B, 2, ...)`` per band), the unnormalised early and late curves, or None."""
    pairs: np.ndarray
    sample_rate: float
    max_lag: int
    bad: np.ndarray
    t0: np.ndarray
    peak_e: np.ndarray
    lag_e: np.ndarray
    ild_db_e: np.ndarray
    exx_e: np.ndarray
    eyy_e: np.ndarray
    peak_l: np.ndarray
    lag_l: np.ndarray
    ild_db_l: np.ndarray
    exx_l: np.ndarray
    eyy_l: np.ndarray
    peak_a: np.ndarray
    lag_a: np.ndarray
    ild_db_a: np.ndarray
    exx_a: np.ndarray
    eyy_a: np.ndarray
    xcorr: Optional[np.ndarray] = None
    centres: Optional[tuple] = None
    half: Optional[int] = None

    @classmethod
    def from_table(cls, table: np.ndarray, pairs, sample_rate: float, max_lag: int, xcorr: Optional[np.ndarray] = None,
                   bands=None) -> "IRPairMetrics":
        """``table``: ``(P, N, 17)``, or ``(P, N, B, 17)`` with ``bands``."""
        table = np.asarray(table, dtype=np.float64)
        return cls(**{name: np.ascontiguousarray(table[..., i]) for i, name in enumerate(PAIR_COLUMNS)},
                   pairs=np.array(pairs, dtype=np.int32).reshape(-1, 2), sample_rate=float(sample_rate), max_lag=int(max_lag), xcorr=xcorr,
                   centres=None if bands is None else tuple(bands.centres), half=None if bands is None else int(bands.half))

    def table(self) -> np.ndarray:
        """The ``(P, N, 17)`` (per band ``(P, N, B, 17)``) table the columns came from."""
        return np.stack([getattr(self, name) for name in PAIR_COLUMNS], axis=-1)

    iacc_e = property(lambda self: np.abs(self.peak_e), doc="IACC of the early window (ISO 3382-1 Annex B)")
    iacc_l = property(lambda self: np.abs(self.peak_l), doc="IACC of the late window")
    iacc_a = property(lambda self: np.abs(self.peak_a), doc="IACC of the whole response")
    itd_e = property(lambda self: self.lag_e / self.sample_rate, doc="lag of the early peak in seconds")
    itd_l = property(lambda self: self.lag_l / self.sample_rate, doc="lag of the late peak in seconds")
    itd_a = property(lambda self: self.lag_a / self.sample_rate, doc="lag of the peak of the whole response in seconds")

    def to_dict(self) -> dict:
        """As ``IRMetrics.to_dict``: plain lists, None for what is not finite, integers in ``bad``, ``t0`` and the lags."""
        d = {name: _plain(getattr(self, name), name in PAIR_INTEGER_COLUMNS) for name in PAIR_COLUMNS}
        d.update(pairs=self.pairs.tolist(), sample_rate=self.sample_rate, max_lag=int(self.max_lag),
                 xcorr=None if self.xcorr is None else _plain(self.xcorr, False))
        if self.centres is not None:
            d.update(centres=[float(v) for v in self.centres], half=int(self.half))
        return d

    @classmethod
    def from_dict(cls, d: dict) -> "IRPairMetrics":
        xcorr = d.get("xcorr")
        return cls(**{name: _array(d[name]) for name in PAIR_COLUMNS}, pairs=np.array(d["pairs"], dtype=np.int32).reshape(-1, 2),
                   sample_rate=float(d["sample_rate"]), max_lag=int(d["max_lag"]), xcorr=None if xcorr is None else _array(xcorr),
                   centres=tuple(float(v) for v in d["centres"]) if "centres" in d else None, half=int(d["half"]) if "half" in d else None)


def _shape_of(irs) -> tuple:
    """``(C, N, L)`` of what ``_view`` takes, refused as ``_view`` refuses it, before anything is uploaded."""
    shape = tuple(int(v) for v in np.shape(irs))
    if len(shape) != 3:
        raise ValueError(f"irs must have shape (C, N, L), got {shape}")
    if min(shape) < 1:
        raise ValueError(f"irs must not be empty, got shape {shape}")
    return shape


def check_pairs(pairs, n_capsules: int) -> np.ndarray:
    """``pairs`` of ``ir_pair_metrics`` as an int32 ``(P, 2)`` array: None is (0, 1), (2, 3), ... (the binaural layout; ValueError for an
    odd capsule count), ``"all"`` every a < b, else an integer ``(P, 2)`` array of capsule indices in ``[0, n_capsules)``."""
    if pairs is None:
        if n_capsules % 2:
            raise ValueError(f"pairs=None pairs consecutive capsules, and {n_capsules} is odd: give pairs")
        return np.arange(n_capsules, dtype=np.int32).reshape(-1, 2)
    if isinstance(pairs, str):
        if pairs != "all":
            raise ValueError(f"pairs must be None, 'all' or an integer (P, 2) array, not {pairs!r}")
        if n_capsules < 2:
            raise ValueError("pairs='all' needs two capsules at least")
        return np.array([(a, b) for a in range(n_capsules) for b in range(a + 1, n_capsules)], dtype=np.int32)
    try:
        table = np.asarray(pairs)
    except (TypeError, ValueError):
        raise ValueError("pairs must be None, 'all' or an integer (P, 2) array")
    if table.dtype.kind not in "iu" or table.ndim != 2 or table.shape[1] != 2 or table.shape[0] < 1:
        raise ValueError(f"pairs must be an integer (P, 2) array with P >= 1, got {table.dtype} {table.shape}")
    if table.min() < 0 or table.max() >= n_capsules:
        raise ValueError(f"pairs holds a capsule index outside 0 .. {n_capsules - 1}")
    return np.ascontiguousarray(table, dtype=np.int32)


def check_max_lag(max_lag, sample_rate: float) -> int:
    """``max_lag`` in samples; None: ``rint(0.001 fs)``, the +-1 ms of ISO 3382-1."""
    if max_lag is None:
        max_lag = int(np.rint(0.001 * sample_rate))
    if isinstance(max_lag, (bool, np.bool_)) or not isinstance(max_lag, (int, np.integer)) or not 0 <= max_lag <= MAX_PAIR_LAG:
        raise ValueError(f"max_lag must be an integer in 0 .. {MAX_PAIR_LAG} (samples), not {max_lag!r}")
    return int(max_lag)


def pair_metrics_device(renderer, irs_ptr: int, n_capsules: int, n_sources: int, stride_c: int, pitch: int, ir_len: int,
                        sample_rate: float, pairs: np.ndarray, max_lag: int, curves: bool = False, workspace_cap: int = 1 << 30):
    """``al_ir_metrics`` for the rows table, then ``al_ir_pair_metrics`` over the tensor at device address ``irs_ptr``: (table buffer
    (P * n_sources * 17 float64), curve buffer (P * n_sources * 2 * (2 max_lag + 1)) or None), on the device, enqueued on the renderer's
    stream.  Where the workspace of all pairs would pass ``workspace_cap`` bytes the pair list is walked in several calls (one pair at
    the least); a line's bits do not depend on the call it fell into.  No synchronisation."""
    mem, lib = renderer.mem, renderer.lib
    n_pairs, n_lags = len(pairs), 2 * max_lag + 1
    rows, _ = metrics_device(renderer, irs_ptr, n_capsules, n_sources, stride_c, pitch, ir_len, sample_rate)
    one = lib.call("al_ir_pair_metrics_workspace_bytes", 1, n_sources, ir_len, max_lag)
    if one <= 0:
        raise ValueError(f"al_ir_pair_metrics_workspace_bytes refused {n_sources} sources, ir_len = {ir_len}, max_lag = {max_lag}")
    groups_of_one = n_sources * (-(-ir_len // _PAIR_TILE))                              # workgroups of one pair: below 2^31 per call
    per_call = max(1, min(n_pairs, int(workspace_cap) // one, (2 ** 31 - 1) // groups_of_one))
    workspace = mem.empty(per_call * one // 8, np.float64)
    table = mem.upload(pairs.reshape(-1))
    out = mem.empty(n_pairs * n_sources * len(PAIR_COLUMNS), np.float64)
    xcorr = mem.empty(n_pairs * n_sources * 2 * n_lags, np.float64) if curves else None
    for p0 in range(0, n_pairs, per_call):
        count = min(per_call, n_pairs - p0)
        lib.call("al_ir_pair_metrics", irs_ptr, n_capsules, n_sources, stride_c, pitch, ir_len, float(sample_rate), mem.ptr(rows),
                 mem.ptr(table) + 8 * p0, count, max_lag, mem.ptr(workspace), per_call * one,
                 mem.ptr(out) + 8 * p0 * n_sources * len(PAIR_COLUMNS),
                 mem.ptr(xcorr) + 8 * p0 * n_sources * 2 * n_lags if curves else None, mem.stream())
    return out, xcorr


def ir_pair_metrics(irs, sample_rate, pairs=None, max_lag=None, renderer=None, curves: bool = False,
                    workspace_cap: int = 1 << 30) -> IRPairMetrics:
    """Inter-aural (inter-capsule) measures of ``irs`` per (pair, source): the peak of the normalised cross-correlation over lags of
    ``+-max_lag`` samples (None: 1 ms) in the early, the late and the whole window, its lag and the level difference (the header
    comment of ``al_ir_pair_metrics``).  ``irs`` as ``ir_metrics`` takes it: a ``DeviceIRTensor`` is measured where it lies.
    ``pairs``: None for consecutive capsules (0, 1), (2, 3), ..., ``"all"`` for every a < b, or an integer ``(P, 2)`` array.
    ``curves=True`` also downloads the unnormalised curves.  ``workspace_cap`` bounds the bytes of workspace per call (the pair list
    is split; never less than one pair's share)."""
    from . import shoebox

    fs = check_rate(sample_rate)
    shoebox._check_workspace_cap(workspace_cap)
    pairs = check_pairs(pairs, _shape_of(irs)[0])
    lag = check_max_lag(max_lag, fs)
    r, buf, stride_c, pitch, (c, n, length) = _view(irs, renderer)
    out, xcorr = pair_metrics_device(r, r.mem.ptr(buf), c, n, stride_c, pitch, length, fs, pairs, lag, curves, workspace_cap)
    p = len(pairs)
    table = np.asarray(r.mem.download(out))[: p * n * len(PAIR_COLUMNS)].reshape(p, n, len(PAIR_COLUMNS))
    curve = None
    if curves:
        curve = np.array(np.asarray(r.mem.download(xcorr))[: p * n * 2 * (2 * lag + 1)].reshape(p, n, 2, 2 * lag + 1))
    return IRPairMetrics.from_table(table, pairs, fs, lag, curve)


def ir_pair_band_metrics(irs, sample_rate, bands=None, pairs=None, max_lag=None, renderer=None, curves: bool = False,
                         workspace_cap: int = 1 << 30) -> IRPairMetrics:
    """``ir_pair_metrics`` per octave band, columns ``(P, N, B)``: a composition of ``al_ir_band_split``, ``al_ir_metrics`` over the band
    rows and ``al_ir_pair_metrics`` over them as a tensor of ``N B`` sources.  THE CONTRACT: (pair, n, b) carries the bits
    ``al_ir_pair_metrics`` gives for the pair at source ``n B + b`` of the tensor ``ir_band_rows`` returns.  The sources are walked in
    passes whose band rows stay under ``workspace_cap`` bytes (one source at the least); ``bands`` as ``ir_band_metrics`` takes them."""
    from . import shoebox

    fs = check_rate(sample_rate)
    bands = check_measure_bands(bands, fs)
    shoebox._check_workspace_cap(workspace_cap)
    pairs = check_pairs(pairs, _shape_of(irs)[0])
    lag = check_max_lag(max_lag, fs)
    r, buf, stride_c, pitch, (c, n, length) = _view(irs, renderer)
    mem = r.mem
    p, n_bands, n_lags, out_pitch = len(pairs), len(bands.centres), 2 * lag + 1, (length + 3) // 4 * 4
    filters = _filters_device(r, bands, fs)
    in_pass = max(1, min(n, int(workspace_cap) // (c * n_bands * out_pitch * 4)))
    rows = mem.empty(c * in_pass * n_bands * out_pitch, np.float32)
    table = np.empty((p, n, n_bands, len(PAIR_COLUMNS)))
    curve = np.empty((p, n, n_bands, 2, n_lags)) if curves else None
    for n0 in range(0, n, in_pass):
        m = min(in_pass, n - n0)
        r.lib.call("al_ir_band_split", mem.ptr(buf) + 4 * n0 * pitch, c, m, stride_c, pitch, length, mem.ptr(filters), n_bands, bands.half,
                   mem.ptr(rows), out_pitch, mem.stream())
        out, xcorr = pair_metrics_device(r, mem.ptr(rows), c, m * n_bands, m * n_bands * out_pitch, out_pitch, length, fs, pairs, lag, curves,
                                         workspace_cap)
        table[:, n0: n0 + m] = np.asarray(mem.download(out))[: p * m * n_bands * len(PAIR_COLUMNS)].reshape(p, m, n_bands, -1)
        if curves:
            curve[:, n0: n0 + m] = np.asarray(mem.download(xcorr))[: p * m * n_bands * 2 * n_lags].reshape(p, m, n_bands, 2, n_lags)
    return IRPairMetrics.from_table(table, pairs, fs, lag, curve, bands)


def state_pair_metrics(state, sample_rate, alias=None, pairs=None, max_lag=None, bands=None, curves: bool = False, renderer=None) -> dict:
    """``{alias: IRPairMetrics}`` of a state's IR tensors as they lie; with ``bands`` per octave band."""
    irs = state.irs
    if alias is not None and alias not in irs:
        raise KeyError(f"no microphone with alias {alias}")
    renderer = renderer or getattr(state, "renderer", None)
    if bands is None:
        return {k: ir_pair_metrics(v, sample_rate, pairs, max_lag, renderer, curves) for k, v in irs.items() if alias is None or k == alias}
    return {k: ir_pair_band_metrics(v, sample_rate, bands, pairs, max_lag, renderer, curves) for k, v in irs.items()
            if alias is None or k == alias}


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
