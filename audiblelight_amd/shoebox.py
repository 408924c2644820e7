"""Shoebox room impulse responses generated on the device (image-source method, csrc/al_ism.h; DESIGN.md "Shoebox IRs").

``shoebox_irs_device`` makes the one call of the C ABI (``al_ism_shoebox``): the (C, N, ir_len) tensor of a rectangular room is
born in HBM in the layout ``Renderer.prepare(plan, clips, irs, ir_strides)`` reads and never crosses PCIe.  ``DeviceIRTensor`` wraps
it as a lazy array: the render path takes its buffer (``result()``), a host consumer downloads it once.  Point capsules,
omnidirectional or with first-order patterns (``patterns=``: ``omni``, ``first_order``, ``cardioid``, ``foa_patterns``; the channels
of a point share one image search, ``al_ism_shoebox_dir``).  Walls are one broadband coefficient each, or, with
``bands=`` (a ``ShoeboxBands``), a column of coefficients per octave band, from a material table if wanted (``load_materials``,
``material_betas``, ``al_ism_shoebox_bands``; DESIGN.md "Shoebox IRs: frequency-dependent walls").  Without ``max_order`` the cost grows as
``ir_len**3 / (Lx * Ly * Lz)`` per (capsule, source) pair; with a ``ShoeboxTail`` the exact image sum ends a fade after the mixing
time and the row continues as seeded Gaussian noise under an envelope that matches the image field in level and decay
(``al_ism_shoebox_tail``, ``tail_envelope``; DESIGN.md "Shoebox IRs: the diffuse tail"), so a row of seconds costs a write of its bytes.
Sources are omnidirectional, or carry a first-order pattern each (``source_patterns=``, the same ``(w, vx, vy, vz)`` as a capsule's,
applied to the direction in which the image's ray leaves the source), and the air may absorb (``air=`` in Np/m, one coefficient or one
per band; ``air_absorption`` gives ISO 9613-1's): ``al_ism_shoebox_src``, ``al_ism_shoebox_bands_src``; DESIGN.md "Shoebox IRs:
directional sources and air".
Capsules may sit on a rigid sphere, an array or a spherical head (``shoebox_sphere_irs_device``, ``sphere_filters``,
``sphere_diffuse_filter``, ``binaural_directions``; ``al_ism_shoebox_sphere``, DESIGN.md "Shoebox IRs: rigid-sphere receivers").
"""
from __future__ import annotations

import ctypes as ct
import json
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

SPEED_OF_SOUND = 343.0
MIN_DISTANCE = 0.01     # metres between a source and a capsule
KNOT_SPACING = 256      # samples between two knots of the tail's envelope table (the kernel's tile)
MIXED_ECHO_DENSITY = 1.0e4   # echoes per second at which a field is heard as diffuse (Griesinger's figure): default_mix_time
ENVELOPE_QUADRATURE = 64     # Gauss-Legendre points per variable of tail_envelope's direction average
OCTAVE_CENTRES = (125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0)     # the band centres of the usual absorption tables, Hz
MAX_BANDS = 8           # bands of al_ism_shoebox_bands
MAX_BAND_HALF = 4096    # its cap on the half length of a band filter
MAX_BAND_TAIL_HALF = 1024     # the cap of al_ism_shoebox_bands_tail
BAND_WORKSPACE_CAP = 1 << 30     # bytes of band-sum workspace shoebox_irs_device allocates at most (never less than one pair's)


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


_REAL = (int, float, np.integer, np.floating)


@dataclass(frozen=True)
class ShoeboxTail:
    """The diffuse tail of a shoebox IR: the image sum is exact up to ``mix_time`` seconds (None: ``default_mix_time``), cross-faded
    over ``fade_time`` seconds (None: a quarter of the mix time; at least one sample) into seeded Gaussian noise.  The noise decays
    as the image-source field of the room does (``tail_envelope``), or, with ``rt60`` given, exponentially at that reverberation
    time from the image field's level at the mixing time.  ``seed``: 64 bits; a row's noise is a function of the seed and of its
    source and capsule numbers alone.  ``coherent``: the rows of one call (one microphone of a state) share their noise as a
    diffuse field does: ``n_waves`` plane waves (even, 2 .. 256) from ``diffuse_directions``, each heard by a row with the delay of
    its position through ``2 half_taps`` interpolation taps and the weight of its pattern (``coherent_tail_tables``,
    ``al_ism_shoebox_coherent``; DESIGN.md "Shoebox IRs: the coherent tail").  Validated by ``check_arguments``."""

    mix_time: Optional[float] = None
    fade_time: Optional[float] = None
    rt60: Optional[float] = None
    seed: int = 0
    coherent: bool = False
    n_waves: int = 64
    half_taps: int = 4

    def to_dict(self) -> dict:
        d = dict(mix_time=self.mix_time, fade_time=self.fade_time, rt60=self.rt60, seed=int(self.seed))
        if self.coherent:      # a tail without it keeps the dictionary it always had
            d.update(coherent=True, n_waves=int(self.n_waves), half_taps=int(self.half_taps))
        return d

    @classmethod
    def from_dict(cls, d) -> "ShoeboxTail":
        if isinstance(d, cls):
            return d
        return cls(mix_time=d.get("mix_time"), fade_time=d.get("fade_time"), rt60=d.get("rt60"), seed=d.get("seed", 0),
                   coherent=d.get("coherent", False), n_waves=d.get("n_waves", 64), half_taps=d.get("half_taps", 4))


def default_mix_time(room, c: float = SPEED_OF_SOUND) -> float:
    """Seconds after which the echo density ``4 pi c^3 tau^2 / V`` of the room reaches ``MIXED_ECHO_DENSITY`` per second:
    ``sqrt(MIXED_ECHO_DENSITY V / (4 pi c^3))``, 42 ms in a 6 x 5 x 3 m room."""
    room = _room(room)
    if not (np.isfinite(c) and c > 0.0):
        raise ValueError("c must be finite and positive")
    return float(np.sqrt(MIXED_ECHO_DENSITY * float(np.prod(room)) / (4.0 * np.pi * float(c) ** 3)))


def n_knots_of(ir_len: int) -> int:
    return (int(ir_len) - 1) // KNOT_SPACING + 2


def _check_tail(tail, betas: np.ndarray) -> None:
    if not isinstance(tail, ShoeboxTail):
        raise ValueError("tail must be a ShoeboxTail or None")
    if np.any(betas == 0.0):
        raise ValueError("a diffuse tail needs every reflection coefficient > 0: a wall of beta = 0 leaves an image lattice of "
                         "lower dimension, whose decay the envelope law does not describe")
    for name in ("mix_time", "fade_time"):
        v = getattr(tail, name)
        if v is not None and not (isinstance(v, _REAL) and not isinstance(v, bool) and np.isfinite(v) and v >= 0.0):
            raise ValueError(f"tail.{name} must be None or a finite time >= 0 in seconds")
    if tail.rt60 is not None and not (isinstance(tail.rt60, _REAL) and not isinstance(tail.rt60, bool) and np.isfinite(tail.rt60)
                                      and tail.rt60 > 0.0):
        raise ValueError("tail.rt60 must be None or a finite reverberation time > 0 in seconds")
    if isinstance(tail.seed, (bool, np.bool_)) or not isinstance(tail.seed, (int, np.integer)) or not 0 <= int(tail.seed) < 1 << 64:
        raise ValueError("tail.seed must be an integer in [0, 2^64)")
    if not isinstance(tail.coherent, (bool, np.bool_)):
        raise ValueError("tail.coherent must be True or False")
    _check_waves(tail.n_waves, tail.half_taps)


MAX_WAVES = 256          # plane waves of al_ism_shoebox_coherent
MAX_HALF_TAPS = 16       # its 32 taps per plane wave, two per half
COHERENT_REACH = 256     # samples a tap of its tables may lie before or after the sample it serves


def _check_waves(n_waves, half_taps) -> None:
    if isinstance(n_waves, (bool, np.bool_)) or not isinstance(n_waves, (int, np.integer)) or not 2 <= int(n_waves) <= MAX_WAVES or int(n_waves) % 2:
        raise ValueError(f"n_waves must be an even integer in 2 .. {MAX_WAVES}")
    if isinstance(half_taps, (bool, np.bool_)) or not isinstance(half_taps, (int, np.integer)) or not 1 <= int(half_taps) <= MAX_HALF_TAPS:
        raise ValueError(f"half_taps must be an integer in 1 .. {MAX_HALF_TAPS}")


def diffuse_directions(n_waves: int) -> np.ndarray:
    """The ``n_waves`` (even) unit vectors ``(P, 3)`` the coherent tail's plane waves arrive from: THE TABLE THIS RETURNS IS THE
    DEFINITION.  With ``h = P / 2`` and ``i = k + 0.5`` for ``k < h``: ``z = 1 - 2 i / h``, ``phi = pi (1 + sqrt 5) i``,
    ``u_k = (sqrt(1 - z^2) cos phi, sqrt(1 - z^2) sin phi, z)`` (a Fibonacci spiral over the sphere) and ``u_{k+h} = -u_k``: the set
    is antipodal, so the model's cross-spectrum between two omnidirectional capsules is real."""
    _check_waves(n_waves, 1)
    h = int(n_waves) // 2
    i = np.arange(h, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / h
    phi = np.pi * (1.0 + np.sqrt(5.0)) * i
    rho = np.sqrt(1.0 - z * z)
    u = np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1)
    return np.ascontiguousarray(np.concatenate([u, -u], axis=0))


def coherent_tail_tables(positions, patterns=None, origin=None, sample_rate: float = 48000.0, c: float = SPEED_OF_SOUND,
                         n_waves: int = 64, half_taps: int = 4) -> Tuple[np.ndarray, np.ndarray]:
    """``(taps, delays)`` of ``al_ism_shoebox_coherent`` for rows at ``positions`` (rows, 3) with the first-order patterns
    ``patterns`` (rows, 4) in room axes (None: omni): float64 ``(rows, P, J)`` and int32 ``(rows, P)``, ``P = n_waves``,
    ``J = 2 half_taps``.  THE TABLES THIS RETURNS ARE THE DEFINITION the kernels are handed.

    Plane wave ``p`` arrives from ``u_p = diffuse_directions(P)[p]`` and reaches row ``c`` at ``delta = -(r_c - origin) . u_p fs / c``
    samples (``origin``: a point, default the centroid of the positions).  With ``D0 = floor(delta)``, ``f = delta - D0`` and
    ``H = half_taps``: ``k_j = sinc(x) 0.5 (1 + cos(pi x / H))`` at ``x = j - (H - 1) - f``, zero for ``|x| >= H``, divided by
    ``sqrt(sum_j k_j^2)``; ``delays[c, p] = D0 - (H - 1)`` and ``taps[c, p, j] = a_cp k_j`` with
    ``a_cp = w_c(u_p) / sqrt(sum_p w_c(u_p)^2)``, ``w_c(u) = w + v . u`` (1 for an omni).  Every plane wave is unit white noise, so
    ``Var g = 1`` for every row and the envelope keeps its meaning.  ValueError: a row whose weights all vanish; a delay outside
    what the entry takes (every tap within 256 samples of the sample it serves)."""
    _check_waves(n_waves, half_taps)
    if not (isinstance(sample_rate, _REAL) and np.isfinite(sample_rate) and sample_rate > 0.0 and isinstance(c, _REAL) and np.isfinite(c)
            and c > 0.0):
        raise ValueError("sample_rate and c must be finite and positive")
    positions = np.ascontiguousarray(positions, dtype=np.float64)
    if positions.ndim != 2 or positions.shape[1] != 3 or len(positions) < 1 or not np.all(np.isfinite(positions)):
        raise ValueError("positions must be finite with shape (rows >= 1, 3)")
    rows, P, H = len(positions), int(n_waves), int(half_taps)
    if patterns is None:
        patterns = np.tile(omni(), (rows, 1))
    patterns = np.asarray(patterns, dtype=np.float64)
    if patterns.shape != (rows, 4) or not np.all(np.isfinite(patterns)):
        raise ValueError(f"patterns must be None or finite with shape ({rows} rows, 4)")
    origin = positions.mean(axis=0) if origin is None else np.asarray(origin, dtype=np.float64)
    if origin.shape != (3,) or not np.all(np.isfinite(origin)):
        raise ValueError("origin must be three finite numbers")
    u = diffuse_directions(P)
    weight = patterns[:, :1] + patterns[:, 1:] @ u.T      # (rows, P)
    norm = np.sqrt((weight * weight).sum(axis=1))
    if np.any(norm == 0.0):
        raise ValueError("a row's pattern is zero towards every plane wave: it has no diffuse tail")
    delta = -((positions - origin[None, :]) @ u.T) * (float(sample_rate) / float(c))
    d0 = np.floor(delta)
    limit = COHERENT_REACH - H
    if np.any(d0 - (H - 1) < -COHERENT_REACH) or np.any(d0 + H > COHERENT_REACH):
        raise ValueError(f"a capsule lies {np.abs(delta).max():.1f} samples from the origin along a plane wave: with half_taps = {H} the "
                         f"coherent tail takes at most {limit}, an array within {limit * float(c) / float(sample_rate):.3g} m of its "
                         f"origin at this sample rate")
    x = np.arange(2 * H, dtype=np.float64)[None, None, :] - (H - 1) - (delta - d0)[:, :, None]
    k = np.where(np.abs(x) < H, np.sinc(x) * 0.5 * (1.0 + np.cos(np.pi * x / H)), 0.0)
    k = k / np.sqrt((k * k).sum(axis=2))[:, :, None]
    taps = (weight / norm[:, None])[:, :, None] * k
    return np.ascontiguousarray(taps), np.ascontiguousarray((d0 - (H - 1)).astype(np.int32))


def tail_samples(tail: ShoeboxTail, room, sample_rate: float, c: float = SPEED_OF_SOUND) -> Tuple[int, int]:
    """``(M, F)``: the mixing sample and the fade length of a tail at this sample rate."""
    mix_time = default_mix_time(room, c) if tail.mix_time is None else float(tail.mix_time)
    fade_time = 0.25 * mix_time if tail.fade_time is None else float(tail.fade_time)
    return int(round(mix_time * sample_rate)), max(1, int(round(fade_time * sample_rate)))


MAX_CHANNELS = 4        # channels per receiver position of al_ism_shoebox_dir
_FOA_AXES = {"w": (1.0, 0.0, 0.0, 0.0), "x": (0.0, 1.0, 0.0, 0.0), "y": (0.0, 0.0, 1.0, 0.0), "z": (0.0, 0.0, 0.0, 1.0)}


def omni() -> np.ndarray:
    """The pattern ``(w, vx, vy, vz) = (1, 0, 0, 0)``: a channel's amplitude is ``a (w + v . u)``, ``u`` the unit vector towards the
    image, in room axes."""
    return np.array([1.0, 0.0, 0.0, 0.0])


def first_order(alpha: float, direction) -> np.ndarray:
    """``(alpha, (1 - alpha) direction / |direction|)``: ``alpha + (1 - alpha) cos(angle to direction)``.  1: omni, 0.5: cardioid,
    0.25: hypercardioid, 0: figure of eight."""
    direction = np.asarray(direction, dtype=np.float64)
    if not (isinstance(alpha, _REAL) and not isinstance(alpha, bool) and np.isfinite(alpha)):
        raise ValueError("alpha must be a finite number")
    if direction.shape != (3,) or not np.all(np.isfinite(direction)):
        raise ValueError("direction must be three finite numbers")
    norm = float(np.sqrt((direction * direction).sum()))
    if not norm > 0.0:
        raise ValueError("direction must not be the zero vector")
    return np.concatenate([[float(alpha)], (1.0 - float(alpha)) * direction / norm])


def cardioid(direction) -> np.ndarray:
    return first_order(0.5, direction)


def foa_patterns(order: str = "wyzx") -> np.ndarray:
    """The four patterns (4, 4) of a first-order ambisonic listener with SN3D weights (W = 1, the dipoles of unit peak), in the
    channel order ``order``, any permutation of the letters w, x, y, z.  ``"wyzx"`` is AmbiX (ACN order)."""
    if not isinstance(order, str) or sorted(order.lower()) != ["w", "x", "y", "z"]:
        raise ValueError("order must be a permutation of the letters w, x, y, z")
    return np.array([_FOA_AXES[ch] for ch in order.lower()], dtype=np.float64)


def _pattern(pattern) -> np.ndarray:
    pattern = np.asarray(pattern, dtype=np.float64)
    if pattern.shape != (4,) or not np.all(np.isfinite(pattern)):
        raise ValueError("a pattern is four finite numbers (w, vx, vy, vz)")
    if not np.any(pattern != 0.0):
        raise ValueError("a pattern must not be all zero")
    return pattern


def check_patterns(patterns, n_positions: int) -> np.ndarray:
    """The pattern table of ``shoebox_irs_device`` as float64 ``(n_positions, K, 4)``, ``K`` in 1 .. 4, finite, no channel all zero
    (ValueError)."""
    try:
        patterns = np.ascontiguousarray(patterns, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("patterns must be an array of shape (positions, channels, 4)")
    if patterns.ndim != 3 or patterns.shape[0] != n_positions or patterns.shape[2] != 4:
        raise ValueError(f"patterns must have shape ({n_positions} positions, channels, 4), not {patterns.shape}")
    if not 1 <= patterns.shape[1] <= MAX_CHANNELS:
        raise ValueError(f"a position takes 1 to {MAX_CHANNELS} channels, not {patterns.shape[1]}")
    if not np.all(np.isfinite(patterns)):
        raise ValueError("patterns must be finite")
    if np.any(np.all(patterns == 0.0, axis=2)):
        raise ValueError("a channel's pattern must not be all zero")
    return patterns


def check_source_patterns(source_patterns, n_sources: int) -> np.ndarray:
    """The source patterns of ``shoebox_irs_device`` as float64 ``(n_sources, 4)``: one pattern ``(4,)`` for every source or a row
    per source, finite, none all zero (ValueError)."""
    try:
        source_patterns = np.asarray(source_patterns, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("source_patterns must be an array of shape (4,) or (sources, 4)")
    if source_patterns.shape == (4,):
        source_patterns = np.tile(source_patterns, (n_sources, 1))
    if source_patterns.shape != (n_sources, 4):
        raise ValueError(f"source_patterns must have shape (4,) or ({n_sources} sources, 4), not {source_patterns.shape}")
    if not np.all(np.isfinite(source_patterns)):
        raise ValueError("source_patterns must be finite")
    if np.any(np.all(source_patterns == 0.0, axis=1)):
        raise ValueError("a source's pattern must not be all zero")
    return np.ascontiguousarray(source_patterns)


def check_air(air, n_bands: Optional[int] = None) -> np.ndarray:
    """The air coefficients of ``shoebox_irs_device`` in Np/m as a float64 array: ``(1,)`` without bands (``n_bands`` None), else
    ``(n_bands,)`` from a number or a vector of that length; finite and >= 0 (ValueError)."""
    try:
        air = np.asarray(air, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("air must be a number (Np/m), or one per band")
    if n_bands is None:
        if air.ndim != 0:
            raise ValueError("without bands air is one number (Np/m)")
        air = air.reshape(1)
    elif air.ndim == 0:
        air = np.full(n_bands, float(air))
    elif air.shape != (n_bands,):
        raise ValueError(f"with {n_bands} bands air is one number or has shape ({n_bands},), not {air.shape}")
    if not np.all(np.isfinite(air)) or np.any(air < 0.0):
        raise ValueError("air must be finite and >= 0 (Np/m)")
    return np.ascontiguousarray(air)


def air_absorption(freqs, temperature_c: float = 20.0, humidity: float = 50.0, pressure_pa: float = 101325.0) -> np.ndarray:
    """The amplitude attenuation of air in Np/m at the frequencies ``freqs`` (Hz) by ISO 9613-1, at ``temperature_c`` degrees
    Celsius, ``humidity`` per cent relative humidity and ``pressure_pa`` pascal: what ``air=`` of ``shoebox_irs_device`` takes.

    With ``T = temperature_c + 273.15``, ``T0 = 293.15``, ``T01 = 273.16``, ``pr = 101325`` and ``pa = pressure_pa``:
    ``psat / pr = 10^(-6.8346 (T01 / T)^1.261 + 4.6151)``, ``h = humidity (psat / pr) / (pa / pr)``,
    ``frO = (pa / pr) (24 + 4.04e4 h (0.02 + h) / (0.391 + h))``,
    ``frN = (pa / pr) (T / T0)^(-1/2) (9 + 280 h exp(-4.170 ((T / T0)^(-1/3) - 1)))``,
    ``alpha = 8.686 f^2 (1.84e-11 (pr / pa) (T / T0)^(1/2) + (T / T0)^(-5/2) (0.01275 exp(-2239.1 / T) / (frO + f^2 / frO)
    + 0.1068 exp(-3352 / T) / (frN + f^2 / frN)))`` in dB/m and ``m = alpha ln(10) / 20``.

    A band of ``ShoeboxBands`` holds everything between its neighbours' centres, and the TOP band everything above its centre:
    the attenuation grows about as ``f^2``, so a coefficient read at the top band's centre understates what that band loses."""
    try:
        f = np.asarray(freqs, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("freqs must be numbers (Hz)")
    if not np.all(np.isfinite(f)) or np.any(f < 0.0):
        raise ValueError("freqs must be finite and >= 0 (Hz)")
    for name, v in (("temperature_c", temperature_c), ("humidity", humidity), ("pressure_pa", pressure_pa)):
        if not (isinstance(v, _REAL) and not isinstance(v, bool) and np.isfinite(v)):
            raise ValueError(f"{name} must be a finite number")
    T = float(temperature_c) + 273.15
    if not (T > 0.0 and 0.0 <= humidity <= 100.0 and pressure_pa > 0.0):
        raise ValueError("temperature above absolute zero, humidity in 0 .. 100 per cent, pressure > 0")
    T0, T01, pr = 293.15, 273.16, 101325.0
    pa_r, Tr = float(pressure_pa) / pr, T / T0
    psat_r = 10.0 ** (-6.8346 * (T01 / T) ** 1.261 + 4.6151)
    h = float(humidity) * psat_r / pa_r
    frO = pa_r * (24.0 + 4.04e4 * h * (0.02 + h) / (0.391 + h))
    frN = pa_r * Tr ** -0.5 * (9.0 + 280.0 * h * np.exp(-4.170 * (Tr ** (-1.0 / 3.0) - 1.0)))
    f2 = f * f
    alpha_db = 8.686 * f2 * (1.84e-11 / pa_r * np.sqrt(Tr) + Tr ** -2.5 * (0.01275 * np.exp(-2239.1 / T) / (frO + f2 / frO)
                                                                         + 0.1068 * np.exp(-3352.0 / T) / (frN + f2 / frN)))
    return alpha_db * (np.log(10.0) / 20.0)


def _centres(centres, sample_rate: float) -> np.ndarray:
    try:
        centres = np.asarray(centres, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("band centres must be numbers")
    if centres.ndim != 1 or not 1 <= len(centres) <= MAX_BANDS:
        raise ValueError(f"1 to {MAX_BANDS} band centres, not an array of shape {centres.shape}")
    if not (np.isfinite(sample_rate) and sample_rate > 0.0):
        raise ValueError("sample_rate must be finite and positive")
    if not np.all(np.isfinite(centres)) or np.any(centres <= 0.0) or np.any(np.diff(centres) <= 0.0) or centres[-1] >= 0.5 * sample_rate:
        raise ValueError("band centres must be positive, strictly increasing and strictly below sample_rate / 2")
    return centres


def _half(half) -> int:
    if isinstance(half, (bool, np.bool_)) or not isinstance(half, (int, np.integer)) or not 1 <= int(half) <= MAX_BAND_HALF:
        raise ValueError(f"half must be an integer in 1 .. {MAX_BAND_HALF}")
    return int(half)


def band_filters(centres=OCTAVE_CENTRES, sample_rate: float = 48000.0, half: int = 512) -> np.ndarray:
    """The float64 table ``phi`` of shape ``(B, 2 half + 1)``, ``phi[b, half + j] = phi_b[j]``, of the zero-phase band filters:
    THE TABLE THIS RETURNS IS THE DEFINITION the kernels are handed.

    On the grid ``f_k = k fs / Nf``, ``Nf = 4 half``, ``k = 0 .. Nf / 2`` the target magnitudes are ``G_0 = 1`` for ``f <= f_0``,
    ``G_{B-1} = 1`` for ``f >= f_{B-1}``, and between two centres, with ``x = log2(f / f_b) / log2(f_{b+1} / f_b)``,
    ``G_b = cos^2(pi x / 2)`` and ``G_{b+1} = sin^2(pi x / 2)``, every other band 0: ``sum_b G_b = 1`` at every grid point.
    ``phi_b[j]`` for ``j = 0 .. half`` is sample ``j`` of the inverse real DFT of length ``Nf`` of ``G_b``
    (``numpy.fft.irfft(G_b, Nf)``) times the window ``0.5 (1 + cos(pi j / (half + 1)))``, and ``phi_b[-j] = phi_b[j]`` is that same
    number: the table is symmetric bit for bit.  ``sum_b phi_b`` is the unit impulse to 1e-15 (the window is 1 at ``j = 0`` and the
    bands' spectra sum to 1), and one band alone is the impulse."""
    half = _half(half)
    centres = _centres(centres, sample_rate)
    n_fft, n_bands = 4 * half, len(centres)
    f = np.arange(n_fft // 2 + 1, dtype=np.float64) * float(sample_rate) / n_fft
    G = np.zeros((n_bands, len(f)))
    G[0, f <= centres[0]] = 1.0
    G[-1, f >= centres[-1]] = 1.0
    for b in range(n_bands - 1):
        between = (f >= centres[b]) & (f < centres[b + 1])     # x = 0 at the centre itself: G_b = 1, G_{b+1} = 0 exactly
        x = np.log2(f[between] / centres[b]) / np.log2(centres[b + 1] / centres[b])
        G[b, between] = np.cos(0.5 * np.pi * x) ** 2
        G[b + 1, between] = np.sin(0.5 * np.pi * x) ** 2
    j = np.arange(half + 1)
    right = np.fft.irfft(G, n_fft, axis=1)[:, : half + 1] * (0.5 * (1.0 + np.cos(np.pi * j / (half + 1.0))))[None, :]
    return np.ascontiguousarray(np.concatenate([right[:, :0:-1], right], axis=1))


@dataclass(frozen=True)
class ShoeboxBands:
    """The bands of a shoebox room with frequency-dependent walls: ``centres`` in Hz (1 to 8, increasing, below half the sample
    rate) and the half length ``half`` of the band filters (``band_filters``).  ``betas`` of such a room has shape ``(6, B)``."""

    centres: Tuple[float, ...] = OCTAVE_CENTRES
    half: int = 512

    def __post_init__(self):
        object.__setattr__(self, "centres", tuple(float(v) for v in np.ravel(np.asarray(self.centres, dtype=np.float64))))

    def to_dict(self) -> dict:
        return dict(centres=list(self.centres), half=int(self.half))

    @classmethod
    def from_dict(cls, d) -> "ShoeboxBands":
        if isinstance(d, cls):
            return d
        return cls(centres=tuple(d.get("centres", OCTAVE_CENTRES)), half=d.get("half", 512))


def load_materials(path) -> dict:
    """A material file ``{"materials": [{"name": ..., "absorption": [f0, a0, f1, a1, ...], ...}]}`` as ``name -> (freqs, alphas)``,
    two float64 arrays with the frequencies in Hz increasing.  Every other key of a material is ignored."""
    with open(path) as fh:
        data = json.load(fh)
    table = {}
    for m in data["materials"]:
        pairs = np.asarray(m["absorption"], dtype=np.float64)
        if pairs.ndim != 1 or len(pairs) < 2 or len(pairs) % 2:
            raise ValueError(f"material {m['name']!r}: absorption must be a flat list f0, a0, f1, a1, ...")
        freqs, alphas = pairs[0::2], pairs[1::2]
        if not np.all(np.isfinite(pairs)) or np.any(freqs <= 0.0) or np.any(np.diff(freqs) <= 0.0):
            raise ValueError(f"material {m['name']!r}: frequencies must be positive and increasing")
        table[str(m["name"])] = (freqs.copy(), alphas.copy())
    return table


def material_betas(table: dict, walls, centres=OCTAVE_CENTRES) -> np.ndarray:
    """Reflection coefficients ``(6, B)`` of six walls ``(x0, x1, y0, y1, z0, z1)`` named in ``table`` (``load_materials``); one
    name serves all six.  A wall's absorption is interpolated linearly in ``log2 f`` at the band centres, held at its end values
    outside the table's range, and goes through ``betas_from_absorption``.  An unknown name is a KeyError."""
    walls = [walls] * 6 if isinstance(walls, str) else list(walls)
    if len(walls) != 6:
        raise ValueError("walls must be six material names (x0, x1, y0, y1, z0, z1) or one name")
    centres = np.asarray(centres, dtype=np.float64)
    if centres.ndim != 1 or len(centres) < 1 or not np.all(np.isfinite(centres)) or np.any(centres <= 0.0):
        raise ValueError("band centres must be positive numbers")
    alphas = np.stack([np.interp(np.log2(centres), np.log2(table[name][0]), table[name][1]) for name in walls])
    return betas_from_absorption(alphas)


def check_bands(bands, betas, sample_rate: float) -> np.ndarray:
    """The band checks of ``check_arguments``: ``betas`` as float64 ``(6, B)`` for ``bands`` (ValueError)."""
    if not isinstance(bands, ShoeboxBands):
        raise ValueError("bands must be a ShoeboxBands or None")
    centres = _centres(bands.centres, sample_rate)
    _half(bands.half)
    try:
        betas = np.ascontiguousarray(betas, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("betas must be an array of shape (6, bands)")
    if betas.shape != (6, len(centres)) or not np.all(np.isfinite(betas)) or np.any(betas < 0.0) or np.any(betas > 1.0):
        raise ValueError(f"with bands, betas must have shape (6, {len(centres)}): a column of six reflection coefficients in [0, 1] per band")
    return betas


def _direction_weight(pattern, mu, phi, s):
    """ln of the octant average's weight of a first-order pattern at the quadrature nodes: ``w^2 + vx^2 s^2 cos^2 phi + vy^2 s^2
    sin^2 phi + vz^2 mu^2`` (the omni pattern: ln 1 = 0)."""
    pw, vx, vy, vz = _pattern(pattern)
    weight = (pw * pw + (vx * vx * np.cos(phi)[None, :] ** 2 + vy * vy * np.sin(phi)[None, :] ** 2) * (s * s)[:, None]
              + vz * vz * (mu * mu)[:, None])
    with np.errstate(divide="ignore"):
        return np.log(weight)


def tail_energy_law(room, betas, sample_rate: float, c: float = SPEED_OF_SOUND, pattern=None, source_pattern=None, air: float = 0.0):
    """``tau -> ln(sigma^2 D(tau))``, ``tau`` in seconds: the expected squared sample of the image-source field (``tail_envelope``
    states the law and the quadrature rule), seen through ``pattern`` (None: omni), sent through ``source_pattern`` (None: omni)
    and through air of ``air`` Np/m."""
    room = _room(room)
    betas = np.ascontiguousarray(betas, dtype=np.float64)
    if betas.shape != (6,) or not np.all(np.isfinite(betas)) or np.any(betas <= 0.0) or np.any(betas > 1.0):
        raise ValueError("the tail's envelope needs six reflection coefficients in (0, 1]")
    if not (np.isfinite(sample_rate) and sample_rate > 0.0 and np.isfinite(c) and c > 0.0):
        raise ValueError("sample_rate and c must be finite and positive")
    c = float(c)
    ln_sigma2 = np.log(c / (4.0 * np.pi * float(np.prod(room)) * float(sample_rate)))
    lam = -np.log(betas[0::2] * betas[1::2]) / room
    x, w = np.polynomial.legendre.leggauss(ENVELOPE_QUADRATURE)
    mu, w_mu = 0.5 * (x + 1.0), 0.5 * w
    phi, w_phi = 0.25 * np.pi * (x + 1.0), 0.25 * np.pi * w
    s = np.sqrt(1.0 - mu * mu)
    rate = (lam[0] * np.cos(phi)[None, :] + lam[1] * np.sin(phi)[None, :]) * s[:, None] + lam[2] * mu[:, None]     # (mu, phi)
    ln_w = np.log(w_mu[:, None] * w_phi[None, :]) + np.log(2.0 / np.pi)
    if pattern is not None:     # the direction weight of a first-order pattern, inside the log-sum (omni: ln 1 = 0, today's bits)
        ln_w = ln_w + _direction_weight(pattern, mu, phi, s)
    if source_pattern is not None:     # the source's weight multiplies the receiver's: the same quadratic form (tail_envelope)
        ln_w = ln_w + _direction_weight(source_pattern, mu, phi, s)
    if not (isinstance(air, _REAL) and not isinstance(air, bool) and np.isfinite(air) and air >= 0.0):
        raise ValueError("air must be a finite number >= 0 (Np/m)")
    air = float(air)

    def ln_energy(tau: float) -> float:
        e = ln_w - c * float(tau) * rate
        top = e.max()
        return float(ln_sigma2 + top + np.log(np.exp(e - top).sum())) - 2.0 * air * c * float(tau)

    return ln_energy


def tail_envelope(room, betas, ir_len: int, sample_rate: float, mix: int, c: float = SPEED_OF_SOUND,
                  rt60: Optional[float] = None, pattern=None, source_pattern=None, air: float = 0.0) -> np.ndarray:
    """The float64 table ``ln_env`` of ``n_knots_of(ir_len)`` log-amplitude knots of the tail, knot ``k`` at sample ``256 k``: THE
    TABLE THIS RETURNS IS THE DEFINITION the kernel is held to.

    ``sigma^2 = c / (4 pi V fs)``: images are uniform in space at density ``1 / V``, each carries ``a^2 = gain / (4 pi d)^2``, and
    ``4 pi d^2 (c / fs) / V`` of them land per sample.  An image in direction ``n`` at distance ``d`` has been reflected about
    ``d |n_i| / L_i`` times on axis ``i``, half by each wall, so with ``lambda_i = -ln(beta_i0 beta_i1) / L_i`` its energy gain
    is ``exp(-d sum_i lambda_i |n_i|)``; averaged over the directions of an octant, at ``d = c tau``,

        D(tau) = (2 / pi) int_0^1 dmu int_0^(pi/2) dphi exp(-c tau (lambda_x s cos phi + lambda_y s sin phi + lambda_z mu)),

    ``s = sqrt(1 - mu^2)``.  THE RULE: both integrals by the 64-point Gauss-Legendre rule
    (``numpy.polynomial.legendre.leggauss(64)``, nodes ``x_j`` and weights ``w_j`` on [-1, 1]) mapped linearly:
    ``mu_j = (x_j + 1) / 2`` with weight ``w_j / 2``, ``phi_j = pi (x_j + 1) / 4`` with weight ``pi w_j / 4``; the double sum is
    taken in the logarithm (the largest exponent is subtracted first), so a ``D`` below the float64 range still gives a finite
    knot.

    Model "ism" (``rt60`` None): ``ln_env[k] = 0.5 ln(sigma^2 D(256 k / fs))``.  With ``rt60 = T``:
    ``ln_env[k] = 0.5 ln(sigma^2 D(mix / fs)) - (3 ln 10 / T) (256 k - mix) / fs``: level-matched to the image field at the mixing
    sample, then exponential at the requested rate.  A ``beta`` of 0 is a ValueError.

    ``pattern = (w, vx, vy, vz)`` (a channel of a directional receiver; None: omni): the image field is symmetric under a sign flip
    of each axis, so the cross terms of ``(w + v . n)^2`` average out and the integrand carries the weight
    ``w^2 + vx^2 s^2 cos^2 phi + vy^2 s^2 sin^2 phi + vz^2 mu^2``, inside the same rule; ``rt60`` level-matches with the weighted
    law.  The omni pattern gives the bits of None.

    ``source_pattern = (w, vx, vy, vz)`` (None: omni): the ray of an image in direction ``u`` left the source along ``e``,
    ``e_i = -sigma_i u_i`` with ``sigma_i`` the parity sign of the image on axis ``i``.  To the order the law works at the parity is
    independent of the sign of ``u_i``, so ``E[gs^2 gr^2] = E[gs^2] E[gr^2]`` with every cross term gone: the integrand's weight is
    the PRODUCT of the two quadratic forms, the source's over the same ``(s cos phi, s sin phi, mu)``.  ``air = m`` in Np/m: an image at
    ``d = c tau`` has lost ``exp(-2 m c tau)`` of its energy, which leaves the integral: ``ln_env[k] -= m c 256 k / fs`` with
    ``rt60`` None.  With ``rt60`` the level is matched at the mixing sample with both factors in and the requested exponential is
    kept as it is: a measured reverberation time already contains the air.  None / omni / 0 give today's bits."""
    ln_energy = tail_energy_law(room, betas, sample_rate, c, pattern, source_pattern, air)
    if int(ir_len) != ir_len or ir_len < 1 or int(mix) != mix or mix < 0:
        raise ValueError("ir_len must be an integer >= 1 and mix an integer >= 0")
    if rt60 is not None and not (np.isfinite(rt60) and rt60 > 0.0):
        raise ValueError("rt60 must be finite and positive")
    fs = float(sample_rate)
    knots = KNOT_SPACING * np.arange(n_knots_of(ir_len), dtype=np.float64)
    if rt60 is None:
        return np.array([0.5 * ln_energy(t / fs) for t in knots], dtype=np.float64)
    return 0.5 * ln_energy(int(mix) / fs) - (3.0 * np.log(10.0) / float(rt60)) * (knots - int(mix)) / fs


def check_arguments(room, betas, sources, capsules, ir_len, sample_rate, c=SPEED_OF_SOUND, max_order=None, tail=None, patterns=None,
                    bands=None, source_patterns=None, air=None):
    """The host-side validation of ``shoebox_irs_device`` (ValueError); returns the arguments as the call takes them (the pattern
    table through ``check_patterns``, the source patterns through ``check_source_patterns``, the air through ``check_air``).  With
    ``bands`` (a ``ShoeboxBands``) ``betas`` is ``(6, B)``."""
    room = _room(room)
    if bands is not None:
        if not (np.isfinite(sample_rate) and sample_rate > 0.0):
            raise ValueError("sample_rate and c must be finite and positive")
        betas = check_bands(bands, betas, float(sample_rate))
        if patterns is not None:
            raise ValueError("bands together with patterns are not yet supported (K x B gains per image)")
        if tail is not None and bands.half > MAX_BAND_TAIL_HALF:
            raise ValueError(f"with a diffuse tail the band filters' half length is at most {MAX_BAND_TAIL_HALF}")
    else:
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
    if tail is not None:
        _check_tail(tail, betas)
    if patterns is not None:
        check_patterns(patterns, len(capsules))
    if source_patterns is not None:
        check_source_patterns(source_patterns, len(sources))
    if air is not None:
        check_air(air, None if bands is None else betas.shape[1])
    gap = np.sqrt(((capsules[:, None, :] - sources[None, :, :]) ** 2).sum(axis=2))
    if gap.min() < MIN_DISTANCE:
        raise ValueError(f"every source must be at least {MIN_DISTANCE} m from every capsule (closest: {gap.min():.4g} m)")
    return room, betas, sources, capsules, int(ir_len), float(sample_rate), float(c), -1 if max_order is None else int(max_order)


def shoebox_irs_device(renderer, room, betas, sources, capsules, ir_len: int, sample_rate: float, c: float = SPEED_OF_SOUND,
                       max_order: Optional[int] = None, tail: Optional[ShoeboxTail] = None, source_id0: int = 0,
                       capsule_id0: int = 0, patterns=None, bands: Optional[ShoeboxBands] = None,
                       workspace_cap: int = BAND_WORKSPACE_CAP, source_patterns=None, air=None, origin=None):
    """The IRs of ``sources`` (N, 3) at ``capsules`` (C, 3) in the room ``(Lx, Ly, Lz)`` with wall reflection coefficients
    ``betas = (x0, x1, y0, y1, z0, z1)``: ``(device buffer, (stride_c, stride_n), ir_len)`` as ``ingest.pack_ragged_irs`` returns
    it, enqueued on the renderer's stream.  The two coordinate tables are all that is uploaded.  With ``tail`` (a ``ShoeboxTail``)
    the rows carry a diffuse tail (``al_ism_shoebox_tail``; the envelope's knot table is uploaded too); row (c, n) draws its
    noise as source ``source_id0 + n`` at capsule ``capsule_id0 + c``, so a caller that splits a tensor over several calls gives
    each part its offsets.

    ``patterns`` (P, K, 4), K in 1 .. 4: ``capsules`` are P receiver POSITIONS with K first-order channels each, channel k of
    position p with the pattern ``(w, vx, vy, vz) = patterns[p, k]`` in room axes (``omni``, ``first_order``, ``cardioid``,
    ``foa_patterns``); the tensor has the P K rows ``c = p K + k`` (``al_ism_shoebox_dir``; DESIGN.md "Shoebox IRs: directional
    receivers"), one image search per position.  With a tail, row c draws as capsule ``capsule_id0 + c`` under the envelope of
    its own pattern.  None: omnidirectional capsules, the call above.

    ``bands`` (a ``ShoeboxBands``): frequency-dependent walls, ``betas`` of shape ``(6, B)`` with a column per band
    (``material_betas``); ``al_ism_shoebox_bands``, DESIGN.md "Shoebox IRs: frequency-dependent walls".  The band filters are
    uploaded (``band_filters``) and a float64 workspace for the band sums is allocated for the call: what all pairs need, at most
    ``workspace_cap`` bytes and at least one pair's; the entry walks the pairs in passes of what it holds, and the rows' bits do
    not depend on it.  With ``tail`` every band decays under its own envelope, ``tail_envelope`` of its column of ``betas``
    (``al_ism_shoebox_bands_tail``; every coefficient > 0).  Not yet together with ``patterns`` (ValueError).

    ``source_patterns`` ``(4,)`` or ``(N, 4)``: a first-order pattern ``(w, vx, vy, vz)`` per source in room axes (``omni``,
    ``first_order``, ``cardioid``), applied to the direction in which an image's ray leaves the source.  ``air``: amplitude
    attenuation in Np/m (``air_absorption``), one number, or ``(B,)`` with bands.  With either the call goes to
    ``al_ism_shoebox_src`` or ``al_ism_shoebox_bands_src`` (DESIGN.md "Shoebox IRs: directional sources and air"), and a tail takes
    an envelope per distinct (receiver pattern, source pattern) or (source pattern, band); with both None the calls above, bit
    for bit.

    ``tail.coherent``: the rows of the call are ONE GROUP whose tails share ``tail.n_waves`` plane waves, with
    ``group_id = capsule_id0`` (``al_ism_shoebox_coherent``; DESIGN.md "Shoebox IRs: the coherent tail"); the two tables of
    ``coherent_tail_tables`` are uploaded.  ``origin``: the point the plane waves' delays are counted from, default the centroid of
    ``capsules``; a caller that splits a microphone over several calls gives every call the same ``origin`` and ``capsule_id0``.
    A call with one row goes to the entries above, bit for bit: one row has nobody to be coherent with.  Not yet together with
    ``bands`` (ValueError)."""
    room, betas, sources, capsules, ir_len, fs, c, order = check_arguments(room, betas, sources, capsules, ir_len, sample_rate, c,
                                                                          max_order, tail, patterns, bands, source_patterns, air)
    if bands is not None:
        _check_workspace_cap(workspace_cap)
    if patterns is not None:
        patterns = check_patterns(patterns, len(capsules))
    n, n_cap, pitch = len(sources), len(capsules), pitch_of(ir_len)
    K = 1 if patterns is None else patterns.shape[1]
    n_rows = n_cap * K
    if tail is not None:
        _check_ids(source_id0, capsule_id0, n, n_rows)
    coherent = None      # the two tables of a coherent tail
    if tail is not None and tail.coherent:
        if bands is not None:
            raise ValueError("bands together with a coherent tail are not yet supported")
        if n_rows > 1:
            coherent = coherent_tail_tables(np.repeat(capsules, K, axis=0), None if patterns is None else patterns.reshape(-1, 4), origin,
                                            fs, c, tail.n_waves, tail.half_taps)
    mem, lib = renderer.mem, renderer.lib
    mix, fade = (-1, 0) if tail is None else tail_samples(tail, room, fs, c)
    # the entries with the source side take its arguments whether or not there is a tail; the others have a name per combination
    src = source_patterns is not None or air is not None or coherent is not None      # the coherent entry takes the arguments of _src
    spat = None if source_patterns is None else check_source_patterns(source_patterns, n)
    air = check_air(0.0 if air is None else air, None if bands is None else betas.shape[1])
    keep = []      # device tables, alive until the call is enqueued

    def ptr_of(table):
        if table is None:
            return 0
        keep.append(mem.upload(table.reshape(-1)))
        return mem.ptr(keep[-1])

    head = (ptr_of(sources), n) + ((ptr_of(spat),) if src else ()) + (ptr_of(capsules), n_cap)
    walls = (room.ctypes.data_as(ct.POINTER(ct.c_double)), betas.ctypes.data_as(ct.POINTER(ct.c_double)))
    sources_of = [None] * n if spat is None else list(spat)
    workspace_pair = ()
    if bands is not None:
        n_bands, half = betas.shape[1], int(bands.half)
        entry = "al_ism_shoebox_bands"
        workspace, workspace_bytes = _workspace(renderer, entry, n_bands, half, ir_len, mix, fade, n * n_cap, workspace_cap)
        workspace_pair = (mem.ptr(workspace), workspace_bytes)
        middle = walls + (n_bands, ptr_of(band_filters(bands.centres, fs, half)), half)
        middle += (air.ctypes.data_as(ct.POINTER(ct.c_double)),) if src else ()
        # a knot table per band, (1, B, n_knots), or per (source, band), (N, B, n_knots)
        keys = [[(b, None, source) for b in range(n_bands)] for source in (sources_of if src else [None])]
    else:
        entry = "al_ism_shoebox" + ("_dir" if patterns is not None and not src else "")
        middle = ((ptr_of(patterns), K) if patterns is not None or src else ()) + walls + ((float(air[0]),) if src else ())
        # one knot table, one per row, (rows, 1, n_knots), or one per (row, source), (rows, N, n_knots)
        rows = [None] * (n_rows if src else 1) if patterns is None else list(patterns.reshape(-1, 4))
        keys = [[(None, row, source) for source in (sources_of if src else [None])] for row in rows]
    tail_block = (mix, fade, 0, int(source_id0), int(capsule_id0), 0, 0) if src else ()
    if tail is not None:
        ln_env = _envelope_tables(room, betas, ir_len, fs, mix, c, tail.rt60, air, keys)
        tail_block = (mix, fade, int(tail.seed), int(source_id0), int(capsule_id0), ptr_of(ln_env), ln_env.shape[-1])
    if coherent is not None:
        taps, delays = coherent
        tail_block += (ptr_of(taps), ptr_of(delays), taps.shape[1], taps.shape[2], int(capsule_id0))
    out = mem.empty(n_rows * n * pitch)
    lib.call(entry + ("_coherent" if coherent is not None else "_src" if src else "_tail" if tail is not None else ""), *head, *middle, c, fs,
             order, ir_len, pitch, *tail_block, *workspace_pair, mem.ptr(out), mem.stream())
    return out, (n * pitch, pitch), ir_len


def _check_workspace_cap(workspace_cap) -> None:
    if isinstance(workspace_cap, (bool, np.bool_)) or not isinstance(workspace_cap, (int, np.integer)) or workspace_cap < 0:
        raise ValueError("workspace_cap must be an integer >= 0 (bytes)")


def _check_ids(source_id0, capsule_id0, n_sources: int, n_rows: int) -> None:
    """The first noise ids of a call with a tail: its sources and rows count on from them within 32 bits."""
    for name, v, count in (("source_id0", source_id0, n_sources), ("capsule_id0", capsule_id0, n_rows)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < 0 or int(v) + count > 1 << 32:
            raise ValueError(f"{name} must be an integer >= 0 with {name} + count <= 2^32")


def _workspace(renderer, entry: str, n_rows: int, half: int, ir_len: int, mix: int, fade: int, pairs: int, workspace_cap: int):
    """``(buffer, bytes)`` of a float64 workspace for the row sums of ``entry`` (the band or the sphere call), allocated for the call:
    what all ``pairs`` need, at most ``workspace_cap`` bytes and at least one pair's."""
    what = "bands" if entry.endswith("bands") else "orders"
    per_pair = renderer.lib.call(entry + "_workspace_bytes", n_rows, half, ir_len, mix, fade)
    if per_pair <= 0:
        raise ValueError(f"{entry}_workspace_bytes refused {n_rows} {what}, half = {half}, ir_len = {ir_len}")
    pairs_per_pass = max(1, min(pairs, int(workspace_cap) // per_pair))
    return renderer.mem.empty(pairs_per_pass * per_pair // 8, dtype=np.float64), pairs_per_pass * per_pair


def _envelope_tables(room, betas, ir_len, fs, mix, c, rt60, air, keys) -> np.ndarray:
    """The knot tables of a call with a tail, stacked as ``keys`` is nested.  A key is ``(band or None, receiver pattern or None,
    source pattern or None)``; band ``b`` decays under column ``b`` of ``betas`` and ``air[b]``.  One quadrature (``tail_envelope``)
    per distinct key."""
    tables = {}

    def table(key):
        if isinstance(key, list):
            return np.stack([table(k) for k in key])
        band, pattern, source = key
        name = (band, None if pattern is None else pattern.tobytes(), None if source is None else source.tobytes())
        if name not in tables:
            tables[name] = tail_envelope(room, betas if band is None else betas[:, band], ir_len, fs, mix, c, rt60, pattern, source,
                                         float(air[0 if band is None else band]))
        return tables[name]

    return table(keys)


# ----------------------------------------------------------------------------- capsules on a rigid sphere
MAX_SPHERE_ORDERS = 64     # Legendre orders of al_ism_shoebox_sphere
MIN_SPHERE_ORDERS = 4      # the fewest sphere_filters takes when asked for a number
MAX_SPHERE_HALF = 1024     # its cap on the half length of a radial filter
SPHERE_PASS_EDGE = 0.8     # the pass edge f_p of the radial filters, as a fraction of the Nyquist frequency


def spherical_hankel1(n_max: int, x) -> np.ndarray:
    """``h_l(x)``, ``l = 0 .. n_max``, the spherical Hankel functions of the first kind at the positive reals ``x``: complex
    ``(n_max + 1, len(x))``.  ``h_0 = -i e^{ix} / x``, ``h_1 = -e^{ix} (x + i) / x^2`` and upwards by
    ``h_{l+1} = (2 l + 1) / x h_l - h_{l-1}``: the stable direction for this solution (it is dominated by ``y_l``, which grows
    with ``l``).  An order that overflows float64 (a tiny ``x`` at a high order) comes out as inf or nan."""
    x = np.asarray(x, dtype=np.float64)
    h = np.zeros((int(n_max) + 1,) + x.shape, dtype=np.complex128)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        e = np.exp(1j * x)
        h[0] = -1j * e / x
        if n_max >= 1:
            h[1] = -e * (x + 1j) / (x * x)
        for l in range(1, int(n_max)):
            h[l + 1] = (2 * l + 1) / x * h[l] - h[l - 1]
    return h


def wiscombe_length(x: float) -> int:
    """``ceil(x + 4 x^(1/3) + 2) + 1``: the orders ``0 .. ceil(x + 4 x^(1/3) + 2)`` of Wiscombe's series length at size parameter ``x``."""
    return int(np.ceil(x + 4.0 * x ** (1.0 / 3.0) + 2.0)) + 1


def _sphere_plan(radius, sample_rate, c, n_orders, half):
    """(radius, fs, c, n_orders, half, f_p) of ``sphere_filters`` (ValueError)."""
    for name, v in (("radius", radius), ("sample_rate", sample_rate), ("c", c)):
        if not (isinstance(v, _REAL) and not isinstance(v, bool) and np.isfinite(v) and v > 0.0):
            raise ValueError(f"{name} must be a finite number > 0")
    a, fs, c = float(radius), float(sample_rate), float(c)
    if half is None:
        half = max(64, 2 * int(np.ceil(4.0 * a * fs / c)))
    if isinstance(half, (bool, np.bool_)) or not isinstance(half, (int, np.integer)) or not 1 <= int(half) <= MAX_SPHERE_HALF:
        raise ValueError(f"half must be an integer in 1 .. {MAX_SPHERE_HALF}")
    f_p = SPHERE_PASS_EDGE * 0.5 * fs
    x_p = 2.0 * np.pi * f_p * a / c
    if n_orders is None:
        n_orders = min(wiscombe_length(x_p), MAX_SPHERE_ORDERS)
    elif (isinstance(n_orders, (bool, np.bool_)) or not isinstance(n_orders, (int, np.integer))
          or not MIN_SPHERE_ORDERS <= int(n_orders) <= MAX_SPHERE_ORDERS):
        raise ValueError(f"n_orders must be None or an integer in {MIN_SPHERE_ORDERS} .. {MAX_SPHERE_ORDERS}")
    n_orders = int(n_orders)
    if wiscombe_length(x_p) > n_orders:     # the largest x whose series still fits: x + 4 x^(1/3) + 2 = n_orders - 1, by bisection
        lo, hi = 0.0, x_p
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if mid + 4.0 * mid ** (1.0 / 3.0) + 2.0 <= n_orders - 1.0 else (lo, mid)
        f_p = lo * c / (2.0 * np.pi * a)
    return a, fs, c, n_orders, int(half), f_p


def _sphere_spectra(a, fs, c, n_orders, half, f_p):
    """``B`` complex ``(n_orders, Nf / 2 + 1)`` of ``sphere_filters`` on the grid ``f_k = k fs / (4 half)``, taper included."""
    n_fft = 4 * half
    f = np.arange(n_fft // 2 + 1, dtype=np.float64) * fs / n_fft
    taper = np.where(f <= f_p, 1.0, np.where(f < 1.25 * f_p, np.cos(0.5 * np.pi * (f - f_p) / (0.25 * f_p)) ** 2, 0.0))
    B = np.zeros((n_orders, len(f)), dtype=np.complex128)
    B[0, 0] = 1.0
    live = np.flatnonzero(taper[1:] > 0.0) + 1
    x = 2.0 * np.pi * f[live] * a / c
    h = spherical_hankel1(n_orders, x)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for l in range(n_orders):
            dh = (l / x) * h[l] - h[l + 1]
            series = (2 * l + 1) * 1j * (-1j) ** l / (x * x * dh)
            # an order whose Hankel function has left the float64 range contributes nothing at that frequency
            B[l, live] = np.where(np.isfinite(dh.real) & np.isfinite(dh.imag), np.conj(series), 0.0) * taper[live]
    return B


def _sphere_window(half: int) -> np.ndarray:
    """``w[|j|]``, ``|j| = 0 .. half``: 1 up to ``half // 2``, then a raised cosine that reaches zero at ``half + 1``."""
    j = np.arange(half + 1, dtype=np.float64)
    flat = half // 2
    return np.where(j <= flat, 1.0, 0.5 * (1.0 + np.cos(np.pi * (j - flat) / (half + 1.0 - flat))))


def sphere_filters(radius: float, sample_rate: float, c: float = SPEED_OF_SOUND, n_orders: Optional[int] = None,
                   half: Optional[int] = None) -> np.ndarray:
    """The float64 table ``b`` of shape ``(n_orders, 2 half + 1)``, ``b[l, half + j] = b_l[j]``, of the radial filters of a rigid
    sphere of ``radius`` metres: THE TABLE THIS RETURNS IS THE DEFINITION ``al_ism_shoebox_sphere`` is handed.  A plane wave from the
    unit direction ``u`` puts ``sum_l P_l(n . u) (b_l * x)`` at the surface point of direction ``n``, with ``x`` the wave at the
    centre: time zero is the arrival at the centre, so the point facing the wave peaks at ``-radius fs / c`` samples.

    Grid ``f_k = k fs / Nf``, ``Nf = 4 half``, ``x_k = 2 pi f_k radius / c``.  Pass edge ``f_p = 0.8 fs / 2``; taper ``T(f) = 1`` up to
    ``f_p``, ``cos^2(pi / 2 (f - f_p) / (0.25 f_p))`` up to ``1.25 f_p`` (the Nyquist frequency for that ``f_p``) and 0 beyond.  For
    ``k >= 1``, ``B_l(f_k) = conj((2 l + 1) i (-i)^l / (x^2 h_l'(x))) T(f_k)`` with ``h_l`` the spherical Hankel function of the first
    kind (``spherical_hankel1``; the conjugate takes the textbook's ``e^{-i w t}`` to numpy's transform) and
    ``h_l' = (l / x) h_l - h_{l+1}``; ``B_0(0) = 1``, ``B_{l >= 1}(0) = 0``.  ``b_l[j] = irfft(B_l, Nf)[j mod Nf] w[j]``, ``w = 1`` for
    ``|j| <= half // 2`` and from there a raised cosine that reaches zero at ``|j| = half + 1``.

    ``n_orders`` None: ``ceil(x_p + 4 x_p^(1/3) + 2) + 1`` with ``x_p = 2 pi f_p radius / c`` (Wiscombe's series length).  If that
    exceeds 64, or ``n_orders`` (4 .. 64) is given and is smaller, THE PASS EDGE ``f_p`` IS LOWERED to the largest frequency whose
    Wiscombe length still fits, and the taper with it: the array is then band-limited below ``1.25 f_p``.  ``half`` None:
    ``max(64, 2 ceil(4 radius fs / c))``, 64 for a 4.2 cm array at 48 kHz, 98 for an 8.75 cm head."""
    a, fs, c, n_orders, half, f_p = _sphere_plan(radius, sample_rate, c, n_orders, half)
    n_fft = 4 * half
    time = np.fft.irfft(_sphere_spectra(a, fs, c, n_orders, half, f_p), n_fft, axis=1)
    j = np.arange(-half, half + 1)
    return np.ascontiguousarray(time[:, j % n_fft] * _sphere_window(half)[np.abs(j)][None, :])


def sphere_diffuse_filter(radius: float, sample_rate: float, c: float = SPEED_OF_SOUND, n_orders: Optional[int] = None,
                          half: Optional[int] = None) -> np.ndarray:
    """The float64 taps ``psi_d`` of shape ``(2 half + 1,)``, index ``j + half``, of the diffuse-field filter of a surface point of
    the sphere of ``sphere_filters`` (same arguments, same grid, transform and window):
    ``D(f_k) = sqrt(sum_l |B_l(f_k)|^2 / (2 l + 1))``, ``D(0) = 1``: the RMS response to plane waves from all directions, which
    tends to sqrt(2) at high ``ka``.  Zero phase, and symmetric bit for bit."""
    a, fs, c, n_orders, half, f_p = _sphere_plan(radius, sample_rate, c, n_orders, half)
    B = _sphere_spectra(a, fs, c, n_orders, half, f_p)
    D = np.sqrt((np.abs(B) ** 2 / (2.0 * np.arange(n_orders)[:, None] + 1.0)).sum(axis=0))
    D[0] = 1.0
    right = np.fft.irfft(D, 4 * half)[: half + 1] * _sphere_window(half)
    return np.ascontiguousarray(np.concatenate([right[:0:-1], right]))


UNIT_TOLERANCE = 16.0 * np.finfo(np.float64).eps     # |n|^2 within this of 1: a unit vector to rounding, taken as it is


def check_directions(directions) -> np.ndarray:
    """Capsule directions as float64 unit vectors ``(C >= 1, 3)``; a zero or non-finite direction is a ValueError.  A row that is of
    unit length to rounding (``| |n|^2 - 1 | <= 16 eps``) is TAKEN AS IT IS, every other row is divided by its length, which leaves it
    within that tolerance: the function is idempotent, so directions that went through it once (``binaural_directions``, a state's
    metadata) keep their bits however often they pass again."""
    try:
        directions = np.array(directions, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("directions must be an array of shape (capsules, 3)")
    if directions.ndim != 2 or directions.shape[1] != 3 or directions.shape[0] < 1:
        raise ValueError("directions must have shape (capsules >= 1, 3)")
    if not np.all(np.isfinite(directions)):
        raise ValueError("directions must be finite")
    largest = np.abs(directions).max(axis=1)
    if np.any(largest == 0.0):
        raise ValueError("a direction must not be the zero vector")
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        norm2 = (directions * directions).sum(axis=1)
        unit = np.abs(norm2 - 1.0) <= UNIT_TOLERANCE
        divided = directions / np.sqrt(norm2)[:, None]
    extreme = ~np.isfinite(norm2) | (norm2 < 1e-280)      # a row whose square overflows or vanishes: scaled by its largest component first
    scaled = directions / largest[:, None]
    scaled = scaled / np.sqrt((scaled * scaled).sum(axis=1))[:, None]
    return np.ascontiguousarray(np.where(unit[:, None], directions, np.where(extreme[:, None], scaled, divided)))


def check_sphere(room, centre, radius, sources=None) -> Tuple[np.ndarray, float]:
    """``(centre, radius)`` of a sphere that lies wholly inside the room, every source at least ``2 radius`` from its centre
    (ValueError): closer than that the plane-wave model of the scattering has an error of order one."""
    room = _room(room)
    if not (isinstance(radius, _REAL) and not isinstance(radius, bool) and np.isfinite(radius) and radius > 0.0):
        raise ValueError("radius must be a finite number > 0 (metres)")
    radius = float(radius)
    centre = np.asarray(centre, dtype=np.float64)
    if centre.shape != (3,) or not np.all(np.isfinite(centre)):
        raise ValueError("centre must be three finite numbers")
    if np.any(centre - radius <= 0.0) or np.any(centre + radius >= room):
        raise ValueError("the sphere must lie wholly inside the room")
    if sources is not None and len(sources):
        gap = np.sqrt(((np.asarray(sources, dtype=np.float64) - centre[None, :]) ** 2).sum(axis=1))
        if gap.min() < 2.0 * radius:
            raise ValueError(f"every source must be at least 2 radius = {2.0 * radius:.4g} m from the sphere's centre "
                             f"(closest: {gap.min():.4g} m)")
    return np.ascontiguousarray(centre), radius


def binaural_directions(forward=(1.0, 0.0, 0.0), up=(0.0, 0.0, 1.0), ear_angle_deg: float = 100.0) -> np.ndarray:
    """The two ear directions ``(2, 3)`` of a spherical head, left first: ``forward`` (made perpendicular to ``up``) turned by
    ``+ear_angle_deg`` and ``-ear_angle_deg`` about ``up``, right-handed, so that with ``up`` towards +z and ``forward`` towards
    +x the left ear points towards +y.  100 degrees puts the ears a little behind the interaural axis, as on a head."""
    forward, up = np.asarray(forward, dtype=np.float64), np.asarray(up, dtype=np.float64)
    if forward.shape != (3,) or up.shape != (3,) or not (np.all(np.isfinite(forward)) and np.all(np.isfinite(up))):
        raise ValueError("forward and up must be three finite numbers each")
    if not (isinstance(ear_angle_deg, _REAL) and not isinstance(ear_angle_deg, bool) and np.isfinite(ear_angle_deg)
            and 0.0 < ear_angle_deg < 180.0):
        raise ValueError("ear_angle_deg must be between 0 and 180 degrees")
    if not np.any(up != 0.0):
        raise ValueError("up must not be the zero vector")
    up = up / np.sqrt((up * up).sum())
    forward = forward - (forward @ up) * up
    norm = np.sqrt((forward * forward).sum())
    if not norm > 1e-12:
        raise ValueError("forward must not be parallel to up")
    forward = forward / norm
    side = np.cross(up, forward)
    angle = np.deg2rad(float(ear_angle_deg))
    return np.stack([np.cos(angle) * forward + np.sin(angle) * side, np.cos(angle) * forward - np.sin(angle) * side])


def shoebox_sphere_irs_device(renderer, room, betas, sources, centre, directions, radius: float, ir_len: int, sample_rate: float,
                              c: float = SPEED_OF_SOUND, max_order: Optional[int] = None, tail: Optional[ShoeboxTail] = None,
                              source_id0: int = 0, capsule_id0: int = 0, n_orders: Optional[int] = None, half: Optional[int] = None,
                              workspace_cap: int = BAND_WORKSPACE_CAP, source_patterns=None, air=None):
    """``shoebox_irs_device`` for the ``C`` capsules of unit directions ``directions`` (C, 3) on a RIGID SPHERE of ``radius`` metres
    at ``centre``: a rigid-sphere array or the two ears of a spherical head (``binaural_directions``); ``al_ism_shoebox_sphere``,
    DESIGN.md "Shoebox IRs: rigid-sphere receivers".  Returns what ``shoebox_irs_device`` returns, the rows in the order of
    ``directions``.  Every image reaches the sphere as a plane wave (a far-field model: the sphere lies wholly inside the room and
    every source is at least ``2 radius`` from its centre, ValueError) and is filtered per Legendre order by ``sphere_filters(radius,
    sample_rate, c, n_orders, half)``, which is uploaded with a float64 workspace as the band call's.  ``betas``: six broadband
    coefficients (not yet together with bands).  With ``tail`` the noise goes through ``sphere_diffuse_filter`` under the omni
    envelope of each source; rows are independent draws.  ``source_patterns`` and ``air`` as in ``shoebox_irs_device``."""
    room, betas, sources, _, ir_len, fs, c, order = check_arguments(room, betas, sources, np.atleast_2d(np.asarray(centre, dtype=np.float64)),
                                                                    ir_len, sample_rate, c, max_order, tail, None, None, source_patterns, air)
    centre, radius = check_sphere(room, centre, radius, sources)
    directions = check_directions(directions)
    _check_workspace_cap(workspace_cap)
    if tail is not None and tail.coherent:
        raise ValueError("a coherent tail on a rigid sphere is not yet supported (its rows are independent draws)")
    table = sphere_filters(radius, fs, c, n_orders, half)
    n_orders, half = table.shape[0], (table.shape[1] - 1) // 2
    n, n_cap, pitch = len(sources), len(directions), pitch_of(ir_len)
    if tail is not None:
        _check_ids(source_id0, capsule_id0, n, n_cap)
    mem, lib = renderer.mem, renderer.lib
    mix, fade = (-1, 0) if tail is None else tail_samples(tail, room, fs, c)
    spat = None if source_patterns is None else check_source_patterns(source_patterns, n)
    air = check_air(0.0 if air is None else air)
    workspace, workspace_bytes = _workspace(renderer, "al_ism_shoebox_sphere", n_orders, half, ir_len, mix, fade, n * n_cap, workspace_cap)
    keep = [mem.upload(sources.reshape(-1)), mem.upload(directions.reshape(-1)), mem.upload(table.reshape(-1))]
    spat_ptr = diffuse_ptr = env_ptr = 0
    n_knots = seed = 0
    if spat is not None:
        keep.append(mem.upload(spat.reshape(-1)))
        spat_ptr = mem.ptr(keep[-1])
    if tail is not None:
        keep.append(mem.upload(sphere_diffuse_filter(radius, fs, c, n_orders, half)))
        diffuse_ptr = mem.ptr(keep[-1])
        # a knot table per source, (N, n_knots): the omni law of tail_envelope
        ln_env = _envelope_tables(room, betas, ir_len, fs, mix, c, tail.rt60, air, [(None, None, source) for source in ([None] * n if spat is None else spat)])
        keep.append(mem.upload(ln_env.reshape(-1)))
        env_ptr, n_knots, seed = mem.ptr(keep[-1]), ln_env.shape[1], int(tail.seed)
    out = mem.empty(n_cap * n * pitch)
    lib.call("al_ism_shoebox_sphere", mem.ptr(keep[0]), n, spat_ptr, centre.ctypes.data_as(ct.POINTER(ct.c_double)), mem.ptr(keep[1]), n_cap,
             room.ctypes.data_as(ct.POINTER(ct.c_double)), betas.ctypes.data_as(ct.POINTER(ct.c_double)), float(air[0]), mem.ptr(keep[2]), n_orders,
             half, diffuse_ptr, c, fs, order, ir_len, pitch, mix, fade, seed, int(source_id0), int(capsule_id0), env_ptr, n_knots,
             mem.ptr(workspace), workspace_bytes, mem.ptr(out), mem.stream())
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
