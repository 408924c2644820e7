"""Sample-wise event augmentations on the GPU, with the reference's class names, ``params`` and
``to_dict`` layout (audiblelight/augmentation.py).

Covered: Gain, Invert, Reverse, Fade, Clipping, Distortion, Bitcrush, Preemphasis, Deemphasis,
TimeWarpSilence / Duplicate / Remove / Reverse, the linear time-invariant filters LowpassFilter,
HighpassFilter, LowShelfFilter, HighShelfFilter and MultibandEqualizer (cascades of second-order
sections, one ``al_fx_sos`` launch each), the delay and modulation FX Delay, Chorus and Phaser
(linear recursions with feedback, one ``al_fx_delay`` / ``al_fx_chorus`` / ``al_fx_phaser`` launch
each), the dynamics FX Compressor and Limiter (an envelope whose coefficient depends on its state: one wave walks the clip,
one ``al_fx_compressor`` / ``al_fx_limiter`` launch each), the time-stretch FX SpeedUp and PitchShift (a phase vocoder,
``al_fx_time_stretch``, and for PitchShift a Kaiser-windowed sinc resampler behind it, ``al_fx_resample_sinc``: grid-wide
launches, no job) and the peak normalisation of ``Event.load_audio``.  The FX whose
kernel runs one clip on one workgroup (the filters, Chorus with feedback, Phaser, Deemphasis, Compressor, Limiter) also
describe their launch as a job (``batch_job``), and ``run_chains`` runs the
chains of a whole scene together: the pending jobs of one kind on all clips go into ONE launch (``al_fx_batch_pack`` /
``al_fx_batch_launch``, one workgroup per clip) with the samples of the per-clip launches, bit for bit (DESIGN.md "Batched
FX launches").  The two codec emulations (GSMFullRateCompressor, MP3Compressor) are not part of this package: out of scope
(SURVEY.md section 2, row 3b).

Definitions for effects whose reference arithmetic lives in un-vendored third-party wheels
(parity unpinned): Gain = x*10^(dB/20); Clipping = clamp at +-10^(dB/20);
Distortion = tanh(x*10^(dB/20)); Bitcrush = rint(x*2^bits)/2^bits (pedalboard 0.9.17);
Preemphasis / Deemphasis = librosa 0.11 ``effects.preemphasis`` / ``deemphasis`` including their
linear-extrapolation initial state.  The filter FX: see ``_FilterFX`` (first-order low/high-pass, Audio EQ
Cookbook shelves and peaks, float64 coefficients and state, constant gains at degenerate cutoffs).  The delay and
modulation FX: see ``Delay``, ``Chorus`` and ``Phaser``.  The dynamics FX: see ``Compressor`` and ``Limiter``.  The time-stretch
FX: see ``_TimeStretchFX``.
"""
from __future__ import annotations

import ctypes as ct
import random as _random
from typing import Any, Optional

import numpy as np

from . import _hip, config
from .utils import tiny


def _renderer():
    from . import synthesize

    return synthesize.get_renderer()


def _sample(override, lo: float, hi: float) -> float:
    """Numeric override, object with ``rvs()``, or uniform(lo, hi) (Augmentation.sample_value, :62-89)."""
    if override is None:
        return float(np.random.uniform(lo, hi))
    if isinstance(override, (int, float, np.integer, np.floating)):
        return override
    if hasattr(override, "rvs"):
        return float(override.rvs())
    raise TypeError(f"Cannot handle type {type(override)}")


def _positive(x, cast=float):
    if not isinstance(x, (int, float, np.integer, np.floating)) or isinstance(x, bool):
        raise TypeError(f"Expected a numeric input, but got {type(x)}")
    if x < 0:
        raise ValueError(f"Expected a positive numeric input, but got {x}")
    return cast(x)


class DeviceClip:
    """A mono clip resident in HBM plus its length; FX ping-pong between two buffers.  A whole FX chain and the peak
    normalisation run on ONE DeviceClip: one upload, N kernel launches, at most one download.  ``device``: the samples are
    already in HBM (a view of the scene's staging arena, ``stage_clips``): nothing is uploaded here."""

    def __init__(self, renderer, host: Optional[np.ndarray] = None, device=None, n: Optional[int] = None):
        self.r = renderer
        if device is not None:
            self.n, self.buf = int(n), device
        else:
            self.n = int(host.shape[-1])
            self.buf = renderer.mem.upload(np.ascontiguousarray(host, dtype=np.float32))
        self.alt = None
        self.uploads, self.downloads = 1, 0   # PCIe crossings of the samples (tests assert the chain stays in HBM)

    def other(self, n: Optional[int] = None):
        n = self.n if n is None else n
        if self.alt is None or len(self.alt) < n:
            self.alt = self.r.mem.empty(n)
        return self.alt

    def swap(self, n: Optional[int] = None):
        self.buf, self.alt = self.alt, self.buf
        if n is not None:
            self.n = n

    def host(self, normalize: bool = False) -> np.ndarray:
        """The clip on the host; ``normalize``: peak-normalised (event.py:535-536) in a device COPY, so the resident clip
        stays as the chain left it (the renderer folds the same scalar into the clip spectra instead, ``al_clip_scales``)."""
        self.downloads += 1
        if not normalize:
            return self.r.mem.download(self.buf)[: self.n].astype(np.float32)
        r, dst = self.r, self.other()
        dst[: self.n] = self.buf[: self.n]
        scale = r.mem.empty(1)
        r.lib.call("al_peak_scale", r.mem.ptr(dst), self.n, ct.c_float(1.0), r.mem.ptr(scale), r.mem.stream())
        r.lib.call("al_scale_rows", r.mem.ptr(dst), self.n, r.mem.ptr(scale), r.mem.stream())
        return r.mem.download(dst)[: self.n].astype(np.float32)

    def peak_normalize(self) -> None:
        """``a / max(|a| + tiny(a))`` (event.py:535-536): the peak is reduced into a DEVICE scalar and applied from it
        (al_peak_scale + al_scale_rows), nothing crosses PCIe."""
        r = self.r
        scale = r.mem.empty(1)
        r.lib.call("al_peak_scale", r.mem.ptr(self.buf), self.n, ct.c_float(1.0), r.mem.ptr(scale), r.mem.stream())
        r.lib.call("al_scale_rows", r.mem.ptr(self.buf), self.n, r.mem.ptr(scale), r.mem.stream())


def stage_clips(renderer, raws) -> list:
    """Raw clips of one scene -> HBM through ONE page-locked arena and ONE asynchronous DMA (instead of a blocking pageable
    copy per event); returns one DeviceClip per clip, each a 4-float aligned view of the arena."""
    mem = renderer.mem
    if not raws:
        return []
    if not hasattr(mem, "upload_staged"):
        return [DeviceClip(renderer, raw) for raw in raws]
    offs, total = [], 0
    for raw in raws:
        offs.append(total)
        total += (len(raw) + 3) // 4 * 4

    def fill(view):
        for off, raw in zip(offs, raws):
            view[off: off + len(raw)] = raw

    arena = mem.upload_staged(total, fill)
    return [DeviceClip(renderer, device=arena[off: off + (len(raw) + 3) // 4 * 4], n=len(raw)) for off, raw in zip(offs, raws)]


def _fx(clip: DeviceClip, op: int, p0: float = 0.0, iparams=None, out_of_place: bool = False) -> None:
    r = clip.r
    pa = (ct.c_float * 1)(p0)  # host scalars: the C ABI reads them while building the launch
    ip = (ct.c_int32 * 4)(*iparams) if iparams is not None else None
    dst = clip.other() if out_of_place else clip.buf
    r.lib.call("al_fx_apply", op, r.mem.ptr(clip.buf), r.mem.ptr(dst), clip.n, ct.cast(pa, ct.c_void_p),
               ct.cast(ip, ct.c_void_p) if ip is not None else None, r.mem.stream())
    if out_of_place:
        clip.swap()


def _sos_rows(rows, gain: float) -> np.ndarray:
    """The float64 (K, 6) rows a launch is given: ``gain`` folded into the first section's numerator."""
    rows = np.array(rows, dtype=np.float64).reshape(-1, 6)
    if len(rows):
        rows[0, :3] *= gain
    return rows


def _sos(clip: DeviceClip, rows, gain: float = 1.0) -> None:
    """Filter the clip in place through float64 second-order sections ``rows`` (K x 6: b0 b1 b2 a0 a1 a2) preceded by the
    constant ``gain``: one al_fx_sos launch per AL_SOS_MAX_SECTIONS sections, the gain folded into the first section's
    numerator.  No rows: the gain alone (one pointwise launch, none at all for the identity)."""
    r = clip.r
    rows = _sos_rows(rows, gain)
    if len(rows) == 0:
        if gain != 1.0:
            _fx(clip, _hip.FX_GAIN, float(gain))
        return
    for k0 in range(0, len(rows), _hip.SOS_MAX_SECTIONS):
        part = np.ascontiguousarray(rows[k0: k0 + _hip.SOS_MAX_SECTIONS])   # a HOST array: read while the launch is built
        r.lib.call("al_fx_sos", r.mem.ptr(clip.buf), r.mem.ptr(clip.buf), clip.n, part.ctypes.data, len(part), r.mem.stream())


def peak_normalize(audio: np.ndarray) -> np.ndarray:
    """``a / max(|a| + tiny(a))`` (event.py:535-536) with the peak reduced and the scale applied on the GPU."""
    clip = DeviceClip(_renderer(), audio)
    clip.peak_normalize()
    return clip.host()


def run_chain(clip: DeviceClip, augmentations, normalize: bool = True) -> DeviceClip:
    """``for aug: a = aug(a)`` then the peak normalisation (event.py:529-536), entirely on one device-resident clip.
    Every augmentation keeps its own pad/truncate(wrap)-to-input-length contract (augmentation.py:117-123)."""
    for aug in augmentations:
        aug.process_device(clip)
    if normalize:
        clip.peak_normalize()
    return clip


def launch_batch(r, kind: int, jobs) -> None:
    """One batched launch of ``kind`` (_hip.FXB_*): ``jobs`` is a list of (src pointer, dst pointer, n, fields), ``fields`` the
    scalars of the kind's job struct (FXB_SOS: ``rows``, the float64 (K, 6) sections).  The library checks and packs the
    descriptors on the host (al_fx_batch_pack), the table goes to HBM through the memory provider, al_fx_batch_launch runs
    one workgroup per job.  The table may go once the call returns: the allocator orders its reuse behind the launch (same
    stream), like TimeWarp's row table."""
    count = len(jobs)
    arr = (_hip.FXB_JOBS[kind] * count)()
    keep = []   # the host SOS rows live until the pack has read them
    for job, (src, dst, n, fields) in zip(arr, jobs):
        job.src, job.dst, job.n = src, dst, n
        if kind == _hip.FXB_SOS:
            keep.append(np.ascontiguousarray(fields["rows"], dtype=np.float64))
            job.sos, job.n_sections = keep[-1].ctypes.data, len(keep[-1])
        else:
            for name, value in fields.items():
                setattr(job, name, value)
    table = np.zeros(count * r.lib.call("al_fx_batch_desc_bytes", kind), dtype=np.uint8)
    r.lib.call("al_fx_batch_pack", kind, ct.cast(arr, ct.c_void_p), count, table.ctypes.data)
    device_table = r.mem.upload(table)
    r.lib.call("al_fx_batch_launch", kind, r.mem.ptr(device_table), count, r.mem.stream())


def run_chains(clips, chains, normalize: bool = False) -> list:
    """``run_chain`` for every (clip, chain) pair of a scene at once, with the same samples bit for bit, in far fewer launches:
    an FX whose kernel is a one-workgroup scan describes its launch as a job (``batch_job``), and the pending jobs of one kind
    on all clips run as ONE grid, one workgroup per clip (``launch_batch``).

    Scheduling: every clip runs its FX one by one as ``run_chain`` does until its next FX has a job (or its chain ends); the
    heads now pending are grouped by kind, each kind is one pack, one upload and one launch; repeat until every chain is done.
    Everything is enqueued on the one stream, so each clip sees its FX in chain order.

    Random draws: the only draws made while a chain RUNS are TimeWarp's coin flips (Python's ``random``).  Every FX hands the
    clip on at its input length, so each event's flips depend on nothing the device computes: they are all drawn up front
    (``draw``), event 0's whole chain, then event 1's, ... -- the order the per-event loop consumes them in -- and the
    launches made from them later."""
    chains = [list(chain) for chain in chains]
    drawn = [[a.draw(clip.n) if hasattr(a, "draw") else None for a in chain] for clip, chain in zip(clips, chains)]
    pos = [0] * len(clips)
    while True:
        pending = {}    # kind -> [(clip index, fields)]
        for i, (clip, chain) in enumerate(zip(clips, chains)):
            while pos[i] < len(chain):
                aug = chain[pos[i]]
                job = aug.batch_job(clip) if hasattr(aug, "batch_job") else None
                if job is not None:
                    pending.setdefault(job[0], []).append((i, job[1]))
                    break
                if drawn[i][pos[i]] is None:
                    aug.process_device(clip)
                else:
                    aug.process_device(clip, drawn[i][pos[i]])
                pos[i] += 1
        if not pending:
            break
        for kind in sorted(pending):
            in_place = kind == _hip.FXB_SOS    # the other kinds ping-pong like _DelayModFX; every kind keeps the length
            jobs = []
            for i, fields in pending[kind]:
                clip = clips[i]
                dst = clip.buf if in_place else clip.other(clip.n)
                jobs.append((clip.r.mem.ptr(clip.buf), clip.r.mem.ptr(dst), clip.n, fields))
            launch_batch(clips[pending[kind][0][0]].r, kind, jobs)
            for i, _ in pending[kind]:
                if not in_place:
                    clips[i].swap()
                pos[i] += 1
    if normalize:
        for clip in clips:
            clip.peak_normalize()
    return list(clips)


def fold_scalars(augmentations) -> Optional[float]:
    """Product of a chain of PURE scalar FX (Gain, Invert), or None when the chain has anything else.  Such a chain
    followed by the peak normalisation is one scalar on the raw clip, ``s / (|s| max|raw| + tiny)``, which the renderer
    evaluates on the device (al_clip_scales) and folds into the clip spectra: the FX kernels are not even launched."""
    s = 1.0
    for aug in augmentations:
        k = getattr(aug, "scalar", None)
        if k is None:
            return None
        s *= float(np.float32(k))
    return s


class Augmentation:
    """Base class: callable object with ``params`` and the pad/truncate(wrap)-to-input-length contract
    of the reference's ``Augmentation.process`` (augmentation.py:91-130)."""

    def __init__(self, sample_rate: Optional[int] = config.SAMPLE_RATE):
        self.sample_rate = _positive(sample_rate, int)
        self.params: dict = dict()

    # subclasses implement this on a DeviceClip (may change clip.n)
    def apply_device(self, clip: DeviceClip) -> None:
        return None

    def draw(self, n: int):
        """Whatever ``apply_device`` would draw from a random generator for a clip of ``n`` samples, drawn now (``run_chains``
        draws a whole scene's up front); None: this FX draws nothing while it runs."""
        return None

    def batch_job(self, clip: DeviceClip):
        """(kind, fields) when this FX on ``clip`` is ONE launch of a one-workgroup scan that ``launch_batch`` can run together
        with other clips' (kind: _hip.FXB_*); None: ``process_device`` runs it."""
        return None

    def process_device(self, clip: DeviceClip, drawn=None) -> None:
        """The FX plus the wrap-pad / truncate back to the input length, on a clip that stays in HBM.  ``drawn``: what
        ``draw(clip.n)`` returned earlier (then nothing is drawn here)."""
        n_in = clip.n
        if drawn is None:
            self.apply_device(clip)
        else:
            self.apply_device(clip, drawn)
        if clip.n != n_in:
            r = clip.r
            dst = clip.other(n_in)
            r.lib.call("al_wrap_copy", r.mem.ptr(clip.buf), clip.n, r.mem.ptr(dst), n_in, r.mem.stream())
            clip.swap(n_in)

    def host_dtype(self, in_dtype: np.dtype) -> np.dtype:
        """The dtype the reference's numpy code leaves a host array of ``in_dtype`` in (most FX keep it; Fade multiplies by a
        float64 envelope, TimeWarpSilence splices float64 zeros in: augmentation.py:1554,1719)."""
        return in_dtype

    def process(self, input_array: np.ndarray) -> np.ndarray:
        arr = np.asarray(input_array)
        if arr.ndim == 2:
            return np.stack([self.process(row) for row in arr])
        clip = DeviceClip(_renderer(), arr)
        self.process_device(clip)
        return clip.host().astype(self.host_dtype(arr.dtype if np.issubdtype(arr.dtype, np.floating) else np.dtype(np.float32)))

    def __call__(self, input_array: np.ndarray) -> np.ndarray:
        return self.process(input_array)

    @property
    def name(self) -> str:
        return type(self).__name__

    def to_dict(self) -> dict[str, Any]:
        return dict(name=self.name, sample_rate=self.sample_rate, **self.params)

    @classmethod
    def from_dict(cls, input_dict: dict[str, Any]):
        d = dict(input_dict)
        name = d.pop("name", cls.__name__)
        target = globals().get(name)
        if target is None or not isinstance(target, type) or not issubclass(target, Augmentation):
            raise ValueError(f"Augmentation class {name} not found")
        return target(**d)

    def __eq__(self, other) -> bool:
        return isinstance(other, Augmentation) and self.to_dict() == other.to_dict()

    def __repr__(self) -> str:
        return f"{self.name}({self.params})"


class EventAugmentation(Augmentation):
    AUGMENTATION_TYPE = "event"


class Gain(EventAugmentation):
    MIN_GAIN, MAX_GAIN = -10, 10

    def __init__(self, sample_rate=config.SAMPLE_RATE, gain_db=None):
        super().__init__(sample_rate)
        self.gain_db = _sample(gain_db, self.MIN_GAIN, self.MAX_GAIN)
        self.params = dict(gain_db=self.gain_db)

    @property
    def linear(self) -> float:
        return float(10.0 ** (self.gain_db / 20.0))

    @property
    def scalar(self) -> float:   # pure scalar FX: foldable (fold_scalars)
        return self.linear

    def apply_device(self, clip):
        _fx(clip, _hip.FX_GAIN, self.linear)


class Invert(EventAugmentation):
    scalar = -1.0

    def apply_device(self, clip):
        _fx(clip, _hip.FX_INVERT)


class Reverse(EventAugmentation):
    def apply_device(self, clip):
        _fx(clip, _hip.FX_REVERSE, out_of_place=True)


class Clipping(EventAugmentation):
    MIN_THRESHOLD_DB, MAX_THRESHOLD_DB = -10, -1

    def __init__(self, sample_rate=config.SAMPLE_RATE, threshold_db=None):
        super().__init__(sample_rate)
        self.threshold_db = -abs(int(_sample(threshold_db, self.MIN_THRESHOLD_DB, self.MAX_THRESHOLD_DB)))
        self.params = dict(threshold_db=self.threshold_db)

    def apply_device(self, clip):
        _fx(clip, _hip.FX_CLIP, float(10.0 ** (self.threshold_db / 20.0)))


class Distortion(EventAugmentation):
    MIN_DRIVE, MAX_DRIVE = 10, 30

    def __init__(self, sample_rate=config.SAMPLE_RATE, drive_db=None):
        super().__init__(sample_rate)
        self.drive_db = _positive(_sample(drive_db, self.MIN_DRIVE, self.MAX_DRIVE))
        self.params = dict(drive_db=self.drive_db)

    def apply_device(self, clip):
        _fx(clip, _hip.FX_TANH, float(10.0 ** (self.drive_db / 20.0)))


class Bitcrush(EventAugmentation):
    MIN_DEPTH, MAX_DEPTH = 8, 32

    def __init__(self, sample_rate=config.SAMPLE_RATE, bit_depth=None):
        super().__init__(sample_rate)
        self.bit_depth = _positive(_sample(bit_depth, self.MIN_DEPTH, self.MAX_DEPTH))
        self.params = dict(bit_depth=self.bit_depth)

    def apply_device(self, clip):
        _fx(clip, _hip.FX_BITCRUSH, float(2.0 ** self.bit_depth))


class Preemphasis(EventAugmentation):
    MIN_COEF, MAX_COEF = 0.0, 1.0
    _OP = _hip.FX_PREEMPH

    def __init__(self, sample_rate=config.SAMPLE_RATE, coef=None):
        super().__init__(sample_rate)
        self.coef = _positive(_sample(coef, self.MIN_COEF, self.MAX_COEF))
        self.params = dict(coef=self.coef)

    def apply_device(self, clip):
        _fx(clip, self._OP, float(self.coef), out_of_place=True)


class Deemphasis(Preemphasis):
    _OP = _hip.FX_DEEMPH

    def batch_job(self, clip):
        if clip.n < 2:
            return None     # refused by the single-clip entry: let it say so
        return _hip.FXB_DEEMPH, dict(coef=float(self.coef))


class Fade(EventAugmentation):
    MIN_FADE, MAX_FADE = 0.0, 1.0
    FADE_SHAPES = ["linear", "exponential", "logarithmic", "quarter_sine", "half_sine", "none"]

    def __init__(self, sample_rate=config.SAMPLE_RATE, fade_in_len=None, fade_out_len=None, fade_in_shape=None,
                 fade_out_shape=None):
        super().__init__(sample_rate)
        self.fade_in_len = _positive(_sample(fade_in_len, self.MIN_FADE, self.MAX_FADE))
        self.fade_out_len = _positive(_sample(fade_out_len, self.MIN_FADE, self.MAX_FADE))
        self.fade_in_shape = self._shape(fade_in_shape)
        self.fade_out_shape = self._shape(fade_out_shape)
        self.params = dict(fade_in_len=self.fade_in_len, fade_out_len=self.fade_out_len,
                           fade_in_shape=self.fade_in_shape, fade_out_shape=self.fade_out_shape)

    def _shape(self, given):
        given = str(np.random.choice(self.FADE_SHAPES)) if given is None else given
        if given not in self.FADE_SHAPES:
            raise ValueError(f"Expected `shape` to be one of {', '.join(self.FADE_SHAPES)} but got {given}")
        return given

    def host_dtype(self, in_dtype):
        return np.result_type(in_dtype, np.float64)

    def apply_device(self, clip):
        n_in = min(int(round(self.fade_in_len * self.sample_rate)), clip.n)
        n_out = min(int(round(self.fade_out_len * self.sample_rate)), clip.n)
        _fx(clip, _hip.FX_FADE, iparams=[n_in, n_out, _hip.FADE_SHAPES[self.fade_in_shape],
                                         _hip.FADE_SHAPES[self.fade_out_shape]])


class TimeWarp(EventAugmentation):
    """Frame-shuffle family (augmentation.py:1604-1790).  The per-row coin flips use Python's ``random()``
    exactly like the reference; the shuffle itself is one gather on the GPU."""

    MIN_PROB, MAX_PROB = 0.05, 0.15
    MIN_FPS, MAX_FPS = 2, 10.0
    MODE = None  # None: identity, 1 silence, 2 reverse, "dup", "rm"

    def __init__(self, sample_rate=config.SAMPLE_RATE, fps=None, prob=None):
        super().__init__(sample_rate)
        self.fps = _positive(_sample(fps, self.MIN_FPS, self.MAX_FPS))
        if self.fps == 0.0:
            raise ValueError(f"Expected fps to be greater than 0 but got {fps}")
        self.prob = _positive(_sample(prob, self.MIN_PROB, self.MAX_PROB))
        self.params = dict(fps=self.fps, prob=self.prob)

    def row_plan(self, n: int):
        """(frame_len, row_len, [(src_row, mode)]): the reference frames with librosa.util.frame, whose
        (frame_len, n_frames) result it iterates BY ROWS (augmentation.py:1684-1692)."""
        fl = round(self.sample_rate / self.fps)
        if fl > n:
            fl_eff, row_len, n_src = n, n, 1      # a single "frame": the whole clip, contiguous
            stride = 1
        else:
            row_len, n_src, stride = 1 + (n - fl) // fl, fl, fl
            fl_eff = fl
        rows = []
        for r in range(n_src):
            hit = _random.random() < self.prob
            if self.MODE == "dup":
                rows.extend([(r, 0)] * (2 if hit else 1))
            elif self.MODE == "rm":
                if not hit:
                    rows.append((r, 0))
            else:
                rows.append((r, self.MODE if (hit and self.MODE) else 0))
        self._spliced_zeros = self.MODE == 1 and any(mode == 1 for _, mode in rows)
        return (1 if fl > n else stride), row_len, rows

    def host_dtype(self, in_dtype):
        # TimeWarpSilence replaces a hit frame by np.zeros(len(frame)) -- float64 -- and np.concatenate widens the rest to it
        return np.result_type(in_dtype, np.float64) if getattr(self, "_spliced_zeros", False) else in_dtype

    def draw(self, n):
        self._spliced_zeros = False
        return self.row_plan(n) if self.prob != 0 else None

    def apply_device(self, clip, drawn=None):
        if drawn is None:
            drawn = self.draw(clip.n)
        if drawn is None:
            return
        stride, row_len, rows = drawn
        if not rows:
            return  # every row removed: the reference falls back to the input (augmentation.py:1698-1701)
        r = clip.r
        table = r.mem.upload(np.array(rows, dtype=np.int32).reshape(-1))
        n_out = len(rows) * row_len
        dst = clip.other(max(n_out, clip.n))
        r.lib.call("al_fx_frame_shuffle", r.mem.ptr(clip.buf), r.mem.ptr(dst), n_out, stride, row_len,
                   r.mem.ptr(table), len(rows), r.mem.stream())
        clip.swap(n_out)   # `table` may go: the allocator orders its reuse behind the launch (same stream)


class TimeWarpSilence(TimeWarp):
    MODE = 1


class TimeWarpReverse(TimeWarp):
    MODE = 2


class TimeWarpDuplicate(TimeWarp):
    MODE = "dup"


class TimeWarpRemove(TimeWarp):
    MODE = "rm"


def _positive_q(q) -> float:
    q = _positive(q)
    if q == 0.0:
        raise ValueError(f"Expected q to be greater than 0 but got {q}")
    return q


def lowpass_section(fc: float, fs: float):
    """(rows, gain) of pedalboard's first-order low-pass (-3 dB at fc): with n = tan(pi fc / fs), b = [n, n],
    a = [n + 1, n - 1].  fc = 0: gain 0; fc >= fs / 2: identity."""
    if fc <= 0:
        return [], 0.0
    if fc >= fs / 2:
        return [], 1.0
    n = np.tan(np.pi * fc / fs)
    return [[n, n, 0.0, n + 1.0, n - 1.0, 0.0]], 1.0


def highpass_section(fc: float, fs: float):
    """(rows, gain) of the first-order high-pass: b = [1, -1], a = [n + 1, n - 1].  fc = 0: identity; fc >= fs / 2: 0."""
    if fc <= 0:
        return [], 1.0
    if fc >= fs / 2:
        return [], 0.0
    n = np.tan(np.pi * fc / fs)
    return [[1.0, -1.0, 0.0, n + 1.0, n - 1.0, 0.0]], 1.0


def shelf_section(fc: float, gain_db: float, q: float, fs: float, high: bool):
    """(rows, gain) of an Audio EQ Cookbook shelf (slope given by Q): A = 10^(dB/40), w = 2 pi fc / fs,
    beta = sin(w) sqrt(A) / Q.  The boosted side tends to 10^(dB/20), the other to 1: a low shelf is the identity at
    fc = 0 and 10^(dB/20) at fc >= fs / 2, a high shelf the reverse."""
    full = float(10.0 ** (gain_db / 20.0))
    if fc <= 0:
        return [], (full if high else 1.0)
    if fc >= fs / 2:
        return [], (1.0 if high else full)
    A = 10.0 ** (gain_db / 40.0)
    w = 2.0 * np.pi * fc / fs
    cw, beta = np.cos(w), np.sin(w) * np.sqrt(A) / q
    if high:
        b = [A * ((A + 1) + (A - 1) * cw + beta), -2 * A * ((A - 1) + (A + 1) * cw), A * ((A + 1) + (A - 1) * cw - beta)]
        a = [(A + 1) - (A - 1) * cw + beta, 2 * ((A - 1) - (A + 1) * cw), (A + 1) - (A - 1) * cw - beta]
    else:
        b = [A * ((A + 1) - (A - 1) * cw + beta), 2 * A * ((A - 1) - (A + 1) * cw), A * ((A + 1) - (A - 1) * cw - beta)]
        a = [(A + 1) + (A - 1) * cw + beta, -2 * ((A - 1) + (A + 1) * cw), (A + 1) + (A - 1) * cw - beta]
    return [b + a], 1.0


def peak_section(fc: float, gain_db: float, q: float, fs: float):
    """(rows, gain) of an Audio EQ Cookbook peak: alpha = sin(w) / (2Q), b = [1 + alpha A, -2 cos w, 1 - alpha A],
    a = [1 + alpha / A, -2 cos w, 1 - alpha / A].  fc = 0 and fc >= fs / 2: identity."""
    if fc <= 0 or fc >= fs / 2:
        return [], 1.0
    A = 10.0 ** (gain_db / 40.0)
    w = 2.0 * np.pi * fc / fs
    alpha, cw = np.sin(w) / (2.0 * q), np.cos(w)
    return [[1 + alpha * A, -2 * cw, 1 - alpha * A, 1 + alpha / A, -2 * cw, 1 - alpha / A]], 1.0


class _FilterFX(EventAugmentation):
    """Linear time-invariant filter FX: a cascade of second-order sections run on the device by ``al_fx_sos`` (float64
    coefficients and recursion state, zero initial state like pedalboard's ``reset=True``).  pedalboard is an un-vendored
    wheel, so the filters are defined here (parity unpinned), with w = 2 pi fc / fs and A = 10^(dB/40):

    * LowpassFilter / HighpassFilter: pedalboard's documented first-order filters, -3 dB at fc; n = tan(pi fc / fs),
      low-pass b = [n, n], high-pass b = [1, -1], both a = [n + 1, n - 1];
    * LowShelfFilter / HighShelfFilter / the bands of MultibandEqualizer: the Audio EQ Cookbook (R. Bristow-Johnson)
      shelf and peak filters, the shelf slope given by Q;
    * degenerate cutoffs (fc = 0, fc >= fs / 2) are the limit of each formula, a constant gain applied as a scalar:
      low-pass 0 / identity, high-pass identity / 0, low shelf identity / 10^(dB/20), high shelf 10^(dB/20) / identity,
      peak identity / identity.  q must be > 0.
    """

    def sections(self):
        """(rows, gain): float64 SOS rows {b0 b1 b2 a0 a1 a2} and the constant gain of the degenerate stages."""
        raise NotImplementedError

    def host_dtype(self, in_dtype):
        return np.dtype(np.float32)     # pedalboard returns float32

    def apply_device(self, clip):
        rows, gain = self.sections()
        _sos(clip, rows, gain)

    def batch_job(self, clip):
        rows = _sos_rows(*self.sections())
        if not 1 <= len(rows) <= _hip.SOS_MAX_SECTIONS:
            return None     # a constant gain (or nothing at all); a cascade that takes several launches
        return _hip.FXB_SOS, dict(rows=rows)


class _FirstOrderFilter(_FilterFX):
    MIN_FREQ, MAX_FREQ = 5512, 22050

    def __init__(self, sample_rate=config.SAMPLE_RATE, cutoff_frequency_hz=None):
        super().__init__(sample_rate)
        self.cutoff_frequency_hz = _positive(_sample(cutoff_frequency_hz, self.MIN_FREQ, self.MAX_FREQ))
        self.params = dict(cutoff_frequency_hz=self.cutoff_frequency_hz)


class LowpassFilter(_FirstOrderFilter):
    MIN_FREQ, MAX_FREQ = 5512, 22050

    def sections(self):
        return lowpass_section(self.cutoff_frequency_hz, self.sample_rate)


class HighpassFilter(_FirstOrderFilter):
    MIN_FREQ, MAX_FREQ = 32, 1024

    def sections(self):
        return highpass_section(self.cutoff_frequency_hz, self.sample_rate)


class _ShelfFilter(_FilterFX):
    MIN_FREQ, MAX_FREQ = 5512, 22050
    MIN_GAIN, MAX_GAIN = -20, 10
    MIN_Q, MAX_Q = 0.1, 1.0
    HIGH = True

    def __init__(self, sample_rate=config.SAMPLE_RATE, gain_db=None, cutoff_frequency_hz=None, q=None):
        super().__init__(sample_rate)
        self.cutoff_frequency_hz = _positive(_sample(cutoff_frequency_hz, self.MIN_FREQ, self.MAX_FREQ))
        self.gain_db = _sample(gain_db, self.MIN_GAIN, self.MAX_GAIN)
        self.q = _positive_q(_sample(q, self.MIN_Q, self.MAX_Q))
        self.params = dict(cutoff_frequency_hz=self.cutoff_frequency_hz, gain_db=self.gain_db, q=self.q)

    def sections(self):
        return shelf_section(self.cutoff_frequency_hz, self.gain_db, self.q, self.sample_rate, self.HIGH)


class HighShelfFilter(_ShelfFilter):
    MIN_FREQ, MAX_FREQ = 5512, 22050
    HIGH = True


class LowShelfFilter(_ShelfFilter):
    MIN_FREQ, MAX_FREQ = 32, 1024
    HIGH = False


class MultibandEqualizer(_FilterFX):
    """1..N Audio EQ Cookbook peak filters in series (augmentation.py:510-660): ``n_bands`` is drawn from [1, 8) and
    truncated by ``int``; each per-band parameter is a scalar (repeated), a list / ndarray of ``n_bands`` values, or a
    distribution sampled once per band."""

    MIN_BANDS, MAX_BANDS = 1, 8
    MIN_GAIN, MAX_GAIN = -20, 10
    MIN_FREQ, MAX_FREQ = 1024, 22050
    MIN_Q, MAX_Q = 0.1, 1.0

    def __init__(self, sample_rate=config.SAMPLE_RATE, n_bands=None, gain_db=None, cutoff_frequency_hz=None, q=None):
        super().__init__(sample_rate)
        self.n_bands = _positive(_sample(n_bands, self.MIN_BANDS, self.MAX_BANDS), int)
        self.gain_db = self._per_band(gain_db, self.MIN_GAIN, self.MAX_GAIN)
        self.cutoff_frequency_hz = self._per_band(cutoff_frequency_hz, self.MIN_FREQ, self.MAX_FREQ)
        self.q = self._per_band(q, self.MIN_Q, self.MAX_Q)
        self.params = dict(n_bands=self.n_bands, gain_db=self.gain_db, cutoff_frequency_hz=self.cutoff_frequency_hz, q=self.q)
        # the reference validates every band when it builds its PeakFilter objects (create_filters, :646-660)
        self._bands = [(_positive(f), g, _positive_q(q)) for g, f, q in zip(self.gain_db, self.cutoff_frequency_hz, self.q)]

    def _per_band(self, override, lo, hi) -> list:
        """sample_peak_filter_params (augmentation.py:599-644)."""
        if override is None:
            return [float(np.random.uniform(lo, hi)) for _ in range(self.n_bands)]
        if isinstance(override, (list, np.ndarray)):
            if len(override) != self.n_bands:
                raise ValueError(f"Expected {self.n_bands} values but got {len(override)}")
            return override if isinstance(override, list) else override.tolist()
        if isinstance(override, (int, float, np.integer, np.floating)):
            return [override for _ in range(self.n_bands)]
        if hasattr(override, "rvs"):
            return [float(override.rvs()) for _ in range(self.n_bands)]
        raise TypeError(f"Cannot handle type {type(override)}")

    def sections(self):
        rows, gain = [], 1.0
        for fc, g, q in self._bands:
            r, k = peak_section(fc, g, q, self.sample_rate)
            rows += r
            gain *= k
        return rows, gain


def _feedback(x) -> float:
    x = _positive(x)
    if x >= 1.0:
        raise ValueError(f"Expected feedback to be below 1 (a stable loop) but got {x}")
    return x


class _DelayModFX(EventAugmentation):
    """Delay and modulation FX: out of place on the device (``clip.other``), float32 like pedalboard's output."""

    def host_dtype(self, in_dtype):
        return np.dtype(np.float32)     # pedalboard returns float32

    def launch(self, clip, dst) -> None:
        raise NotImplementedError

    def apply_device(self, clip):
        dst = clip.other(clip.n)
        self.launch(clip, dst)
        clip.swap()


class Delay(_DelayModFX):
    """pedalboard 0.9.17's ``Delay`` (augmentation.py:1046-1102), restated by definition and not checked against a running
    pedalboard: D = trunc(delay_seconds fs), clamped to 30 fs; ``delay_seconds == 0`` is the identity; otherwise, with
    w[m] = 0 for m < 0, d[t] = w[t - D], w[t] = x[t] + feedback d[t], y = (1 - mix) x + mix d (the line is read before it
    is written: D = 0 gives d = 0).  mix is used as given.  feedback >= 1 is refused (an unstable loop)."""

    MIN_DELAY, MAX_DELAY = 0.01, 1.0
    MIN_FEEDBACK, MAX_FEEDBACK = 0.1, 0.5
    MIN_MIX, MAX_MIX = 0.1, 0.5
    MAX_DELAY_SECONDS = 30          # pedalboard's longest delay line

    def __init__(self, sample_rate=config.SAMPLE_RATE, delay_seconds=None, feedback=None, mix=None):
        super().__init__(sample_rate)
        self.delay_seconds = _positive(_sample(delay_seconds, self.MIN_DELAY, self.MAX_DELAY))
        self.feedback = _feedback(_sample(feedback, self.MIN_FEEDBACK, self.MAX_FEEDBACK))
        self.mix = _positive(_sample(mix, self.MIN_MIX, self.MAX_MIX))
        self.params = dict(delay_seconds=self.delay_seconds, feedback=self.feedback, mix=self.mix)

    @property
    def delay_samples(self) -> int:
        return min(int(self.delay_seconds * self.sample_rate), self.MAX_DELAY_SECONDS * self.sample_rate)

    def apply_device(self, clip):
        if self.delay_seconds == 0:
            return                      # pedalboard special-cases it: the identity
        super().apply_device(clip)

    def launch(self, clip, dst):
        r = clip.r
        r.lib.call("al_fx_delay", r.mem.ptr(clip.buf), r.mem.ptr(dst), clip.n, self.delay_samples, ct.c_float(self.feedback),
                   ct.c_float(self.mix), r.mem.stream())


class _Modulation(_DelayModFX):
    MIN_RATE, MAX_RATE = 0, 10
    MIN_DEPTH, MAX_DEPTH = 0.0, 1.0
    MIN_MIX, MAX_MIX = 0.1, 0.5
    MIN_FEEDBACK, MAX_FEEDBACK = 0.0, 0.9
    CENTRE = ""                     # the name of the centre parameter
    ENTRY = ""
    KIND = 0                        # _hip.FXB_* of the batched launch

    def __init__(self, sample_rate, rate_hz, depth, centre, feedback, mix):
        super().__init__(sample_rate)
        self.rate_hz = _positive(_sample(rate_hz, self.MIN_RATE, self.MAX_RATE))
        self.depth = _positive(_sample(depth, self.MIN_DEPTH, self.MAX_DEPTH))
        centre = _positive(_sample(centre, self.MIN_CENTRE, self.MAX_CENTRE))
        setattr(self, self.CENTRE, centre)
        self.feedback = _feedback(_sample(feedback, self.MIN_FEEDBACK, self.MAX_FEEDBACK))
        self.mix = _positive(_sample(mix, self.MIN_MIX, self.MAX_MIX))
        self.params = {"rate_hz": self.rate_hz, "depth": self.depth, self.CENTRE: centre, "feedback": self.feedback,
                       "mix": self.mix}

    def batch_job(self, clip):
        if self.KIND == _hip.FXB_CHORUS and self.feedback == 0:
            return None     # grid-wide already (k_fx_chorus_ff)
        return self.KIND, dict(fs=float(self.sample_rate), rate_hz=float(self.rate_hz), depth=float(self.depth),
                               centre=float(getattr(self, self.CENTRE)), feedback=float(self.feedback), mix=float(self.mix))

    def launch(self, clip, dst):
        r = clip.r
        r.lib.call(self.ENTRY, r.mem.ptr(clip.buf), r.mem.ptr(dst), clip.n, float(self.sample_rate), float(self.rate_hz),
                   float(self.depth), float(getattr(self, self.CENTRE)), float(self.feedback), float(self.mix), r.mem.stream())


class Chorus(_Modulation):
    """JUCE's ``dsp::Chorus`` as pedalboard 0.9.17 wraps it (augmentation.py:746-829), restated by definition and not checked
    against a running pedalboard.  lfo_t = sin(2 pi rate t / fs - pi) (JUCE's oscillator returns its old phase minus pi;
    the phase is exact float64 here, JUCE accumulates it in float32); tau_t = clamp(max(1, 10 depth lfo_t + centre_delay_ms)
    fs / 1000, 0, ceil(110 fs / 1000)) = i_t + f_t; with u[m] = 0 for m < 0, u[t] = x[t] - feedback v[t-1],
    v[t] = u[t - i_t] + f_t (u[t - i_t - 1] - u[t - i_t]), y = (1 - m) x + m v with m = min(mix, 1) (JUCE's DryWetMixer
    clamps it).  feedback >= 1 is refused (an unstable loop)."""

    MIN_CENTRE, MAX_CENTRE = MIN_DELAY, MAX_DELAY = 1.0, 20.0
    CENTRE = "centre_delay_ms"
    ENTRY = "al_fx_chorus"
    KIND = _hip.FXB_CHORUS

    def __init__(self, sample_rate=config.SAMPLE_RATE, rate_hz=None, depth=None, centre_delay_ms=None, feedback=None,
                 mix=None):
        super().__init__(sample_rate, rate_hz, depth, centre_delay_ms, feedback, mix)


class Phaser(_Modulation):
    """JUCE's ``dsp::Phaser`` as pedalboard 0.9.17 wraps it (augmentation.py:963-1043), restated by definition and not checked
    against a running pedalboard.  fmax = min(20000, 0.49 fs), c = log10(fc / 20) / log10(fmax / 20); the LFO ticks every 4
    samples: lfo_k = clamp(0.5 depth sin(2 pi rate 4k / fs - pi) + c, 0, 1), f_k = 20 (fmax / 20)^lfo_k; six first-order TPT
    all-passes share G = g / (1 + g), g = tan(pi f_k / fs), each {v = G (in - s), lp = v + s, s = lp + v, out = 2 lp - in};
    per sample in_0 = x - L, wet = the sixth stage's output, L = feedback wet; y = (1 - m) x + m wet, m = min(mix, 1).
    float64 LFO phase and state; feedback >= 1 is refused; 0.49 fs must exceed 20 Hz."""

    MIN_CENTRE, MAX_CENTRE = MIN_FREQ, MAX_FREQ = 260, 6500
    CENTRE = "centre_frequency_hz"
    ENTRY = "al_fx_phaser"
    KIND = _hip.FXB_PHASER

    def __init__(self, sample_rate=config.SAMPLE_RATE, rate_hz=None, depth=None, centre_frequency_hz=None, feedback=None,
                 mix=None):
        super().__init__(sample_rate, rate_hz, depth, centre_frequency_hz, feedback, mix)


class _DynamicsFX(_DelayModFX):
    """Dynamics FX: one launch of ``k_fx_dynamics`` (one wave walks the clip's envelope), out of place; as a job of a batched
    launch the clips of a scene are walked side by side."""

    ENTRY = ""
    KIND = 0                        # _hip.FXB_* of the batched launch
    MIN_THRESHOLD_DB, MAX_THRESHOLD_DB = -40, -20
    MIN_RELEASE, MAX_RELEASE = 50, 1100

    def _fields(self) -> dict:
        return dict(fs=float(self.sample_rate), **{k: float(v) for k, v in self.params.items()})

    def batch_job(self, clip):
        return self.KIND, self._fields()

    def launch(self, clip, dst):
        r = clip.r
        r.lib.call(self.ENTRY, r.mem.ptr(clip.buf), r.mem.ptr(dst), clip.n, *self._fields().values(), r.mem.stream())


class Compressor(_DynamicsFX):
    """JUCE's ``dsp::Compressor`` as pedalboard 0.9.17 wraps it (augmentation.py:663-743), restated by definition and not
    checked against a running pedalboard.  cte(ms) = 0 when ms < 1e-3, else exp(-2 pi 1000 / (ms fs)); cA = cte(attack_ms),
    cR = cte(release_ms); T = 10^(threshold_db / 20).  Per sample, with e = 0 before the clip: a = |x|, c = cA when a > e, else
    cR, e <- a + c (e - a), g = 1 when e < T, else (e / T)^(1 / ratio - 1), y = g x.  float64 arithmetic and state (JUCE:
    float32).  ``ratio`` below 1 is refused."""

    RATIOS = [4, 8, 12, 20]         # the UREI 1176's
    MIN_ATTACK, MAX_ATTACK = 1, 100
    ENTRY = "al_fx_compressor"
    KIND = _hip.FXB_COMPRESSOR

    def __init__(self, sample_rate=config.SAMPLE_RATE, threshold_db=None, ratio=None, attack_ms=None, release_ms=None):
        super().__init__(sample_rate)
        self.threshold_db = -abs(int(_sample(threshold_db, self.MIN_THRESHOLD_DB, self.MAX_THRESHOLD_DB)))
        self.ratio = int(_positive(np.random.choice(self.RATIOS) if ratio is None else _sample(ratio, 0, 0)))
        if self.ratio < 1:
            raise ValueError(f"Expected a ratio of at least 1 but got {self.ratio}")
        self.attack_ms = _positive(_sample(attack_ms, self.MIN_ATTACK, self.MAX_ATTACK))
        self.release_ms = _positive(_sample(release_ms, self.MIN_RELEASE, self.MAX_RELEASE))
        self.params = dict(threshold_db=self.threshold_db, ratio=self.ratio, attack_ms=self.attack_ms,
                           release_ms=self.release_ms)


class Limiter(_DynamicsFX):
    """JUCE's ``dsp::Limiter`` as pedalboard 0.9.17 wraps it (augmentation.py:871-924), restated by definition and not checked
    against a running pedalboard: a compressor stage (see ``Compressor``) at (-10 dB, ratio 4, 2 ms, 200 ms), a second one on
    its output at (threshold_db, ratio 1000, cA = 0, release_ms), then y = clamp(G y2, -1, 1) with
    G = 10^(10 (1 - 1/4) / 40) 10^(-threshold_db / 20).  JUCE's smoothed output gain starts at its target (no ramp)."""

    ENTRY = "al_fx_limiter"
    KIND = _hip.FXB_LIMITER

    def __init__(self, sample_rate=config.SAMPLE_RATE, threshold_db=None, release_ms=None):
        super().__init__(sample_rate)
        self.threshold_db = -abs(int(_sample(threshold_db, self.MIN_THRESHOLD_DB, self.MAX_THRESHOLD_DB)))
        self.release_ms = _positive(_sample(release_ms, self.MIN_RELEASE, self.MAX_RELEASE))
        self.params = dict(threshold_db=self.threshold_db, release_ms=self.release_ms)


class _TimeStretchFX(EventAugmentation):
    """Time-stretch FX.  The reference calls ``pedalboard.time_stretch`` (Rubber Band, an un-vendored wheel; parity unpinned,
    SURVEY.md 8c), so the effect is pinned by the definition in DESIGN.md "Time-stretch FX", restated and not checked against a
    running pedalboard or librosa: ``stretch(x, rate, n_fft, n_out)`` is librosa 0.11's ``effects.time_stretch`` (a phase
    vocoder, hop n_fft / 4, sin^2 window, float64 phase accumulator), one ``al_fx_time_stretch`` call that enqueues its kernels
    on the stream without a host synchronisation.  The launches are grid-wide already: there is no ``batch_job``."""

    N_FFT = 2048
    MIN_RATE, MAX_RATE = 0.25, 4.0      # what al_fx_time_stretch accepts

    def host_dtype(self, in_dtype):
        return np.dtype(np.float32)     # pedalboard returns float32

    @property
    def identity(self) -> bool:
        raise NotImplementedError

    def process(self, input_array):
        if self.identity:
            return input_array          # the reference's ``process`` hands the input back untouched
        return super().process(input_array)

    def stretch(self, clip: DeviceClip, rate: float, n_out: int, dst) -> None:
        """dst[:n_out] = stretch(clip, rate, N_FFT, n_out)."""
        r = clip.r
        floats = r.lib.call("al_fx_time_stretch_workspace_floats", clip.n, float(rate), self.N_FFT)
        work = r.mem.empty(floats)      # may go once the call returns: the allocator orders its reuse behind the launches
        r.lib.call("al_fx_time_stretch", r.mem.ptr(clip.buf), clip.n, r.mem.ptr(dst), n_out, float(rate), self.N_FFT,
                   r.mem.ptr(work), r.mem.stream())


class SpeedUp(_TimeStretchFX):
    """``stretch(x, stretch_factor, 2048, n_out)`` with n_out = max(1, round(n / stretch_factor)) (Python's ``round``); the clip
    then has n_out samples and ``process_device`` wrap-pads or truncates it back to n.  ``stretch_factor == 1`` is the identity:
    no launch.  A factor outside [0.25, 4] is refused."""

    MIN_SHIFT, MAX_SHIFT = 0.7, 1.5

    def __init__(self, sample_rate=config.SAMPLE_RATE, stretch_factor=None):
        super().__init__(sample_rate)
        self.stretch_factor = _positive(_sample(stretch_factor, self.MIN_SHIFT, self.MAX_SHIFT))
        if not self.MIN_RATE <= self.stretch_factor <= self.MAX_RATE:
            raise ValueError(f"Expected a stretch factor in [{self.MIN_RATE}, {self.MAX_RATE}] but got {self.stretch_factor}")
        self.params = dict(stretch_factor=self.stretch_factor)

    @property
    def identity(self) -> bool:
        return self.stretch_factor == 1.0

    def apply_device(self, clip):
        if self.identity:
            return
        n_out = max(1, int(round(clip.n / self.stretch_factor)))
        dst = clip.other(n_out)
        self.stretch(clip, self.stretch_factor, n_out, dst)
        clip.swap(n_out)


class PitchShift(_TimeStretchFX):
    """r = 2^(-semitones / 12), m = max(1, round(n / r)), y1 = stretch(x, r, 2048, m), then y1 resampled to exactly n samples by
    a Kaiser-windowed sinc (``al_fx_resample_sinc``: c = 0.95 min(1, n / m), half-width 16 / c, beta 8.6, float64 per output
    sample).  ``semitones`` is truncated by ``int``; 0 is the identity: no launch.  |semitones| > 24 is refused."""

    MIN_SEMITONES, MAX_SEMITONES = -3, 3
    SEMITONES_LIMIT = 24                # r stays in [0.25, 4]

    def __init__(self, sample_rate=config.SAMPLE_RATE, semitones=None):
        super().__init__(sample_rate)
        self.semitones = int(_sample(semitones, self.MIN_SEMITONES, self.MAX_SEMITONES))
        if abs(self.semitones) > self.SEMITONES_LIMIT:
            raise ValueError(f"Expected at most {self.SEMITONES_LIMIT} semitones either way but got {self.semitones}")
        self.params = dict(semitones=self.semitones)

    @property
    def identity(self) -> bool:
        return self.semitones == 0

    def apply_device(self, clip):
        if self.identity:
            return
        r, n = clip.r, clip.n
        rate = 2.0 ** (-self.semitones / 12.0)
        m = max(1, int(round(n / rate)))
        stretched = r.mem.empty(m)
        self.stretch(clip, rate, m, stretched)
        dst = clip.other(n)
        r.lib.call("al_fx_resample_sinc", r.mem.ptr(stretched), m, r.mem.ptr(dst), n, r.mem.stream())
        clip.swap(n)


ALL_EVENT_AUGMENTATIONS = [Gain, Invert, Reverse, Fade, Clipping, Distortion, Bitcrush, Preemphasis, Deemphasis,
                           TimeWarpSilence, TimeWarpDuplicate, TimeWarpRemove, TimeWarpReverse,
                           LowpassFilter, HighpassFilter, LowShelfFilter, HighShelfFilter, MultibandEqualizer,
                           Delay, Chorus, Phaser, Compressor, Limiter, SpeedUp, PitchShift]
