"""Minimal Scene / Event / WorldState stand-ins with the attribute surface the synthesis path uses.

The reference's ``Scene`` (audiblelight/core.py), ``Event`` (audiblelight/event.py) and ``WorldState``
(audiblelight/worldstate.py) do placement, ray tracing and file decoding, which are out of scope
here.  These classes carry exactly the attributes listed in SURVEY.md 8a A15,
so a scene can be described from arrays already in memory (clips + IR tensors) and rendered with
``Scene.generate()``; objects of the real AudibleLight classes work with the same functions.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, List, Optional, Sequence

import numpy as np

import os

from . import config
from .utils import LazyAudioDict, tiny, valid_audio

VERSION = "0.2"


class Event:
    """An audio event: a mono clip, its emitters (IR columns), timing and level (event.py:31-191)."""

    def __init__(self, alias: str, audio: np.ndarray, sample_rate: int = config.SAMPLE_RATE, snr: float = 15.0,
                 scene_start: float = 0.0, n_emitters: int = 1, is_moving: Optional[bool] = None,
                 augmentations: Sequence = (), ref_ir_channel: Optional[int] = None,
                 direct_path_time_ms: Optional[Sequence[float]] = None, class_label: Optional[str] = None,
                 class_id: Optional[int] = None, filepath: Optional[str] = None, event_start: float = 0.0,
                 duration: Optional[float] = None, metadata: Optional[dict] = None,
                 native_sample_rate: Optional[int] = None):
        audio = np.asarray(audio)
        if audio.ndim != 1:
            raise ValueError("Event audio must be mono (1-D)")
        self.alias = alias
        self.sample_rate = int(sample_rate)
        # ``audio`` is at ``native_sample_rate`` (default: the scene rate); resampling to ``sample_rate`` is the first
        # step of the device chain (librosa.load(sr=...) does it on the host, event.py:520-527)
        self.native_sample_rate = int(native_sample_rate) if native_sample_rate else self.sample_rate
        self._raw = np.ascontiguousarray(audio, dtype=np.float32)
        self.snr = float(snr)
        self.scene_start = float(scene_start)
        # the reference keeps the requested duration in seconds (event.py:131-133); the decoded clip may be a sample off
        self.duration = float(duration) if duration is not None else len(self._raw) / self.native_sample_rate
        self.scene_end = self.scene_start + self.duration
        self.n_emitters = int(n_emitters)
        self.is_moving = bool(self.n_emitters > 1 if is_moving is None else is_moving)
        self.augmentations: List = list(augmentations)
        self.ref_ir_channel = ref_ir_channel
        self.direct_path_time_ms = direct_path_time_ms
        self.class_label, self.class_id = class_label, class_id
        self.filepath, self.event_start = filepath, float(event_start)
        self.metadata = dict(metadata or {})   # reference-format keys this path does not interpret (emitter coordinates, ...)
        self.audio: Optional[np.ndarray] = None
        self.spatial_audio = LazyAudioDict()
        self._spatial_audio_padded = LazyAudioDict()
        self._spatial_audio_dry = LazyAudioDict()
        self._spatial_audio_dry_padded = LazyAudioDict()

    def __len__(self) -> int:
        return self.n_emitters

    @property
    def filename(self) -> Optional[str]:
        """Name of the audio file behind the event (event.py: ``filepath.name``): events sharing it share a DCASE source index."""
        return self.metadata.get("filename") or (os.path.basename(self.filepath) if self.filepath else self.alias)

    @property
    def emitters_relative(self) -> dict:
        """{mic: [[azimuth, elevation, distance], ...] per emitter} when the event came with positions (reference metadata)."""
        return self.metadata.get("emitters_relative") or {}

    @property
    def is_audio_loaded(self) -> bool:
        return self.audio is not None

    def register_augmentations(self, augmentations) -> None:
        """Add FX and drop every cached render (event.py:739-782)."""
        self.augmentations.extend(augmentations if isinstance(augmentations, (list, tuple)) else [augmentations])
        self.clear_audio()

    def clear_augmentations(self) -> None:
        self.augmentations = []
        self.clear_audio()

    def clear_audio(self) -> None:
        self.audio = None
        self._last_chain = None
        self.spatial_audio = LazyAudioDict()
        self._spatial_audio_padded = LazyAudioDict()
        self._spatial_audio_dry = LazyAudioDict()
        self._spatial_audio_dry_padded = LazyAudioDict()

    def _device_chain(self, normalize: bool, staged=None):
        """Raw clip -> HBM once, the whole FX chain (and, if asked, the peak normalisation) there (augmentation.run_chain).
        ``staged``: a DeviceClip already holding the raw clip (the scene's one-DMA staging arena, ``stage_event_chains``)."""
        from . import augmentation, synthesize

        from . import ingest

        device_fx = all(hasattr(a, "process_device") for a in self.augmentations)
        clip = staged if staged is not None else augmentation.DeviceClip(synthesize.get_renderer(), self._raw)
        ingest.resample_clip(clip, self.native_sample_rate, self.sample_rate)
        if not device_fx:   # foreign callables (e.g. host pedalboard FX of the reference): run them where they live
            out = clip.host() if self.native_sample_rate != self.sample_rate else self._raw.copy()
            for aug in self.augmentations:
                out = aug(out)
            clip = augmentation.DeviceClip(synthesize.get_renderer(), out)
            return augmentation.run_chain(clip, [], normalize)
        return augmentation.run_chain(clip, self.augmentations, normalize)

    def _foldable(self) -> bool:
        from . import augmentation

        return self.native_sample_rate == self.sample_rate and augmentation.fold_scalars(self.augmentations) is not None

    def _chain(self, ignore_cache: bool, staged=None):
        """The clip behind the FX chain, NOT yet peak-normalised, resident in HBM; ONE realisation per event, kept until
        ``clear_audio`` (the reference's ``load_audio`` caches ``self.audio`` the same way, event.py:507-510,538): every
        microphone, the dry path and ``load_audio`` see the same TimeWarp* coin flips, and a deterministic chain is
        uploaded and run once, not once per microphone."""
        clip = None if ignore_cache else getattr(self, "_last_chain", None)
        if clip is None:
            clip = self._device_chain(False, staged)
            self._last_chain = clip
        return clip

    @classmethod
    def from_file(cls, filepath: str, alias: str, sample_rate: int, event_start: float = 0.0,
                  duration: Optional[float] = None, **kwargs) -> "Event":
        """An event from a WAV file, the way the reference's constructor + ``load_audio`` read one
        (event.py:131-133,520-527): ``[event_start, event_start + duration)`` of the file, down-mixed to mono on the host,
        resampled to ``sample_rate`` on the device when the chain first runs."""
        from . import ingest

        audio, native = ingest.read_wav_excerpt(filepath, event_start, duration)
        return cls(alias, audio, sample_rate, filepath=filepath, event_start=event_start,
                   duration=duration if duration is not None else len(audio) / native, native_sample_rate=native, **kwargs)

    def load_audio(self, ignore_cache: Optional[bool] = False, normalize: Optional[bool] = True) -> np.ndarray:
        """Clip after the FX chain and peak normalisation (event.py:496-539); cached in ``self.audio``.
        One upload, the chain on the device, one download (no intermediate copies between FX)."""
        if self.is_audio_loaded and not ignore_cache:
            return self.audio
        out = self._chain(bool(ignore_cache)).host(normalize=bool(normalize)).astype(self.chain_dtype(), copy=False)
        valid_audio(out)
        self.audio = out
        return self.audio

    def chain_dtype(self) -> np.dtype:
        """The dtype the reference's FX chain leaves a float32 clip in (event.py:520-539 + the numpy FX of augmentation.py): float32
        unless an FX widens it -- Fade's float64 envelope, a TimeWarpSilence that spliced float64 zeros in on its last run."""
        dt = np.dtype(np.float32)
        for a in self.augmentations:
            if hasattr(a, "host_dtype"):
                dt = np.dtype(a.host_dtype(dt))
        return dt

    def clip_source(self, ignore_cache: Optional[bool] = False, chain_is_fresh: bool = False):
        """What the renderer needs of this event's clip WITHOUT bringing samples back to the host
        (engine.ClipSource): a chain of pure scalars (Gain, Invert) + peak normalisation becomes the raw clip plus
        one device-evaluated scalar; any other chain runs on the device ONCE per event (``_chain``) and is handed over in
        HBM with its peak normalisation left to the same device scalar (``al_clip_scales``: no extra pass over the clip);
        a clip somebody already loaded to the host (``self.audio``) is used as it is.  ``chain_is_fresh``: the cached chain
        was run for THIS render (``stage_event_chains``), so it is used even when ``ignore_cache`` asks for a new one."""
        from . import augmentation, engine

        if self.is_audio_loaded and not ignore_cache:
            return engine.ClipSource(host=np.ascontiguousarray(self.audio, dtype=np.float32), n=len(self.audio))
        if self._foldable():
            return engine.ClipSource(host=self._raw, n=len(self._raw), prescale=augmentation.fold_scalars(self.augmentations),
                                     normalize=True)
        clip = self._chain(bool(ignore_cache) and not chain_is_fresh)
        return engine.ClipSource(device=clip.buf, n=clip.n, prescale=1.0, normalize=True)

    def to_dict(self) -> dict:
        """The reference's Event metadata layout (event.py:568-620).  Keys this path does not compute (emitter
        coordinates, image, velocity) are carried over from ``self.metadata`` when the event was loaded from a
        reference file, else left empty."""
        m = self.metadata
        return dict(
            alias=self.alias, filename=m.get("filename", os.path.basename(self.filepath) if self.filepath else None),
            filepath=self.filepath, class_id=self.class_id, class_label=self.class_label, is_moving=self.is_moving,
            scene_start=self.scene_start, scene_end=self.scene_end, event_start=self.event_start,
            event_end=self.event_start + self.duration, duration=self.duration, snr=self.snr, sample_rate=self.sample_rate,
            image_filepath=m.get("image_filepath"), spatial_resolution=m.get("spatial_resolution"),
            spatial_velocity=m.get("spatial_velocity"), shape=m.get("shape"), num_emitters=self.n_emitters,
            emitters=m.get("emitters", []), emitters_relative=m.get("emitters_relative", {}),
            augmentations=[a.to_dict() for a in self.augmentations if hasattr(a, "to_dict")],
            ref_ir_channel=self.ref_ir_channel, direct_path_time_ms=self.direct_path_time_ms)

    @classmethod
    def from_dict(cls, input_dict: dict, audio: np.ndarray) -> "Event":
        """An event from the reference's metadata (event.py:622-698) plus its decoded clip: either exactly the
        ``[event_start, event_start + duration)`` excerpt at ``sample_rate`` (what ``librosa.load(offset, duration)``
        returns, event.py:520-527) or the whole file, from which that excerpt is cut.  Decoding / resampling files is
        out of scope here."""
        from . import augmentation as aug_mod

        for k in ("alias", "snr", "duration", "scene_start", "scene_end", "sample_rate"):
            if k not in input_dict:
                raise KeyError(f"Missing key: '{k}'")
        d = input_dict
        sr = int(d["sample_rate"])
        audio = np.asarray(audio)
        want = int(round(float(d["duration"]) * sr))
        if len(audio) > want + 1:   # whole file given: cut the excerpt
            lo = int(round(float(d.get("event_start") or 0.0) * sr))
            audio = audio[lo: lo + want]
        n_emit = d.get("num_emitters", d.get("n_emitters"))
        if n_emit is None:
            n_emit = len(d.get("emitters") or [None])
        fx = [aug_mod.Augmentation.from_dict(a) for a in d.get("augmentations", [])]
        keep = {k: d[k] for k in ("filename", "image_filepath", "spatial_resolution", "spatial_velocity", "shape", "emitters",
                                  "emitters_relative") if k in d}
        return cls(d["alias"], audio, sr, snr=d["snr"], scene_start=d["scene_start"], n_emitters=int(n_emit),
                   is_moving=d.get("is_moving"), augmentations=fx, ref_ir_channel=d.get("ref_ir_channel"),
                   direct_path_time_ms=d.get("direct_path_time_ms"), class_label=d.get("class_label"),
                   class_id=d.get("class_id"), filepath=d.get("filepath"), event_start=d.get("event_start") or 0.0,
                   duration=d["duration"], metadata=keep)


def stage_event_chains(events, ignore_cache: bool = False) -> list:
    """Before a scene is rendered: the raw clips of every event whose FX chain has to RUN on the device (not foldable into a
    scalar, no cached realisation, nothing loaded to the host) go to HBM through one page-locked arena and one asynchronous
    DMA, and their chains run there, all together (event.py:520-539 does a blocking load + host chain per event)."""
    from . import augmentation, synthesize

    todo = [ev for ev in events
            if isinstance(ev, Event) and not (ev.is_audio_loaded and not ignore_cache) and not ev._foldable()
            and (ignore_cache or getattr(ev, "_last_chain", None) is None)
            and all(hasattr(a, "process_device") for a in ev.augmentations)]
    if not todo:
        return []
    from . import ingest

    staged = augmentation.stage_clips(synthesize.get_renderer(), [ev._raw for ev in todo])
    for ev, clip in zip(todo, staged):
        ingest.resample_clip(clip, ev.native_sample_rate, ev.sample_rate)
    # all chains together: the one-workgroup scans of every event in one launch per kind (augmentation.run_chains)
    augmentation.run_chains(staged, [ev.augmentations for ev in todo])
    for ev, clip in zip(todo, staged):
        ev._last_chain = clip
    return todo


class MicArray:
    """Capsule count holder (micarrays.py:36-162): only ``n_capsules`` / ``n_listeners`` matter to the path."""

    def __init__(self, alias: str, n_capsules: int, metadata: Optional[dict] = None, n_listeners: Optional[int] = None):
        # n_listeners: points in space (an FOA listener is one point with four channels); None: one per capsule
        self.alias, self.n_capsules = alias, int(n_capsules)
        self.n_listeners = int(n_capsules) if n_listeners is None else int(n_listeners)
        self.metadata = dict(metadata or {})

    def to_dict(self) -> dict:   # micarrays.py:207-240 (coordinates only when loaded from a reference file)
        d = dict(name=self.metadata.get("name", self.alias), micarray_type=self.metadata.get("micarray_type", "MicArray"),
                 n_capsules=self.n_capsules)
        d.update({k: v for k, v in self.metadata.items() if k not in d})
        return d


class StaticIRState:
    """WorldState stand-in holding precomputed IRs: {mic: (C, N_emitters_total, L)} (worldstate.py:360-370)."""

    name = "static"

    def __init__(self, irs: Dict[str, np.ndarray], microphones: Optional[Dict[str, dict]] = None,
                 metadata: Optional[dict] = None):
        self._irs = OrderedDict((k, np.asarray(v)) for k, v in irs.items())
        mic_meta = microphones or {}
        self.microphones = OrderedDict((k, MicArray(k, v.shape[0], mic_meta.get(k))) for k, v in self._irs.items())
        self.metadata = dict(metadata or {})   # reference state keys kept for the round trip (emitters, mesh, backend)

    def to_dict(self) -> dict:   # worldstate.py:2330-2356 layout
        d = dict(backend=self.metadata.get("backend", self.name), sample_rate=self.metadata.get("sample_rate"),
                 emitters=self.metadata.get("emitters", {}),
                 microphones={k: m.to_dict() for k, m in self.microphones.items()})
        d.update({k: v for k, v in self.metadata.items() if k not in d})
        return d

    @property
    def irs(self):
        return self._irs

    @property
    def num_emitters(self) -> int:
        return next(iter(self._irs.values())).shape[1] if self._irs else 0

    def get_irs(self):
        return self._irs

    def simulate(self) -> None:  # IRs are given, nothing to trace
        return None

    def metrics(self, alias: Optional[str] = None, edc: bool = False, sample_rate: Optional[float] = None, renderer=None) -> dict:
        """``{alias: acoustics.IRMetrics}`` of the tensors as they are (acoustics.ir_metrics: reverberation times, DRR, clarity per
        row, measured on the device); ``sample_rate``: default the ``sample_rate`` of the metadata.  Not part of ``to_dict()``."""
        from . import acoustics

        rate = self.metadata.get("sample_rate") if sample_rate is None else sample_rate
        if rate is None:
            raise ValueError("this state knows no sample rate: give sample_rate")
        return acoustics.state_metrics(self, rate, alias, edc, renderer)

    def band_metrics(self, alias: Optional[str] = None, bands=None, edc: bool = False, sample_rate: Optional[float] = None,
                     renderer=None) -> dict:
        """``{alias: acoustics.IRBandMetrics}``: ``metrics()`` per octave band (acoustics.ir_band_metrics; ``bands``: a
        ``shoebox.ShoeboxBands``, its dictionary, or None for the six octave centres).  Not part of ``to_dict()``."""
        from . import acoustics

        rate = self.metadata.get("sample_rate") if sample_rate is None else sample_rate
        if rate is None:
            raise ValueError("this state knows no sample rate: give sample_rate")
        return acoustics.state_band_metrics(self, rate, alias, bands, edc, renderer)

    def pair_metrics(self, alias: Optional[str] = None, pairs=None, max_lag=None, bands=None, curves: bool = False,
                     sample_rate: Optional[float] = None, renderer=None) -> dict:
        """``{alias: acoustics.IRPairMetrics}``: IACC, ITD and ILD per (capsule pair, emitter) (acoustics.ir_pair_metrics; ``pairs``
        None: consecutive capsules).  ``bands``: None for the broadband rows, True for the six octave centres, or a
        ``shoebox.ShoeboxBands`` / its dictionary (acoustics.ir_pair_band_metrics).  Not part of ``to_dict()``."""
        from . import acoustics, shoebox

        rate = self.metadata.get("sample_rate") if sample_rate is None else sample_rate
        if rate is None:
            raise ValueError("this state knows no sample rate: give sample_rate")
        return acoustics.state_pair_metrics(self, rate, alias, pairs, max_lag, shoebox.ShoeboxBands() if bands is True else bands, curves,
                                            renderer)


class ShoeboxIRState:
    """WorldState stand-in for a rectangular room whose IRs are generated on the device by the image-source method
    (shoebox.py, DESIGN.md "Shoebox IRs"): the reference's ``WorldStateShoebox`` (worldstate.py:3105-3110) is declared and left
    empty.  ``betas``: six wall reflection coefficients (x0, x1, y0, y1, z0, z1), or ``rt60`` for one uniform coefficient by
    Sabine's law.  Microphones are sets of point capsules, omnidirectional or with a first-order pattern each
    (``add_microphone(patterns=...)``), or one point with the four channels of first-order ambisonics (``add_foa_listener``);
    emitters are IR columns in event order (a moving event contributes one row per trajectory point).  ``simulate()`` enqueues one
    generation per microphone; the tensors stay in HBM.
    ``tail``: a ``shoebox.ShoeboxTail`` (or its dictionary) gives every row a diffuse tail past the mixing time; channels are
    numbered through the microphones in their order, so no two rows of the state share noise.
    With ``tail.coherent`` every microphone of point capsules is one group whose tails are coherent as a diffuse field's are
    (DESIGN.md "Shoebox IRs: the coherent tail"); its first channel's number is the group's id.
    ``bands``: a ``shoebox.ShoeboxBands`` (or its dictionary) gives the walls a reflection coefficient per band (DESIGN.md "Shoebox
    IRs: frequency-dependent walls"): ``betas`` then has shape (6, B), or ``materials`` names six walls (or one name for all) in
    ``material_table`` (``shoebox.load_materials``), read at the band centres.  The names are kept with the betas in ``to_dict``;
    ``from_dict`` needs no material file.
    ``air``: the air's amplitude attenuation in Np/m (``shoebox.air_absorption``), one number, or one per band with ``bands``;
    ``add_emitters(patterns=...)`` gives emitters a first-order pattern each (DESIGN.md "Shoebox IRs: directional sources and
    air").  Without either the state generates what it generated before, bit for bit.
    ``add_sphere_microphone`` puts capsules on a rigid sphere and ``add_binaural_listener`` two ears on a spherical head (DESIGN.md
    "Shoebox IRs: rigid-sphere receivers"); the other microphones of the state are generated as before."""

    name = "SHOEBOX"

    def __init__(self, room, betas=None, rt60: Optional[float] = None, ir_len: int = 4096, sample_rate: int = config.SAMPLE_RATE,
                 c: float = 343.0, max_order: Optional[int] = None, renderer=None, metadata: Optional[dict] = None, tail=None,
                 bands=None, materials=None, material_table=None, air=None):
        from . import shoebox

        self.bands = shoebox.ShoeboxBands.from_dict(bands) if isinstance(bands, dict) else bands
        self.materials = None
        if materials is not None:
            if betas is not None or rt60 is not None:
                raise ValueError("give either materials, betas or rt60")
            if material_table is None:
                raise ValueError("materials needs a material_table (shoebox.load_materials)")
            if self.bands is None:
                self.bands = shoebox.ShoeboxBands()
            if not isinstance(self.bands, shoebox.ShoeboxBands):
                raise ValueError("bands must be a ShoeboxBands, its dictionary or None")
            self.materials = [materials] * 6 if isinstance(materials, str) else [str(v) for v in materials]
            betas = shoebox.material_betas(material_table, self.materials, self.bands.centres)
        if (betas is None) == (rt60 is None):
            raise ValueError("give either betas or rt60")
        if self.bands is not None and rt60 is not None:
            raise ValueError("rt60 gives one broadband coefficient: with bands give betas (6, B) or materials")
        self.room = shoebox._room(room)
        self.rt60 = None if rt60 is None else float(rt60)
        self.betas = shoebox.betas_from_rt60(self.room, rt60, c) if betas is None else np.array(betas, dtype=np.float64)
        self.ir_len, self.sample_rate, self.c = int(ir_len), int(sample_rate), float(c)
        self.max_order = None if max_order is None else int(max_order)
        self.tail = shoebox.ShoeboxTail.from_dict(tail) if isinstance(tail, dict) else tail
        self.renderer = renderer
        self.metadata = dict(metadata or {})
        self.microphones: "OrderedDict[str, MicArray]" = OrderedDict()
        self.emitters: "OrderedDict[str, np.ndarray]" = OrderedDict()
        self._emitter_patterns: "OrderedDict[str, np.ndarray]" = OrderedDict()      # (n, 4) of the aliases that have patterns
        self._capsules: "OrderedDict[str, np.ndarray]" = OrderedDict()      # receiver positions (P, 3) of each microphone
        self._patterns: "OrderedDict[str, Optional[np.ndarray]]" = OrderedDict()     # None (omni) or (P, K, 4)
        self._spheres: "OrderedDict[str, dict]" = OrderedDict()      # the microphones on a rigid sphere: centre, radius, directions, ...
        self._irs = None
        # refuse bad room parameters here, not at the first simulate()
        inside = 0.5 * self.room[None, :]
        shoebox.check_arguments(self.room, self.betas, inside, inside + 0.25 * self.room[None, :], self.ir_len, self.sample_rate,
                                self.c, self.max_order, self.tail, None, self.bands, None, air)
        self.air = None      # a number, or with bands an array (B,)
        if air is not None:
            self.air = float(shoebox.check_air(air)[0]) if self.bands is None else shoebox.check_air(air, self.betas.shape[1])

    def add_microphone(self, alias: str, capsule_positions, patterns=None, capsule_names=None) -> MicArray:
        """``capsule_positions`` (C, 3).  ``patterns`` (C, 4): one first-order pattern ``(w, vx, vy, vz)`` per capsule in room axes
        (``shoebox.omni``, ``first_order``, ``cardioid``); None: omnidirectional capsules."""
        from . import shoebox

        capsules = shoebox._points(capsule_positions, self.room, f"capsules of {alias}")
        if patterns is not None:
            patterns = np.asarray(patterns, dtype=np.float64)
            if patterns.shape != (len(capsules), 4):
                raise ValueError(f"patterns of {alias} must have shape ({len(capsules)} capsules, 4), not {patterns.shape}")
            patterns = patterns[:, None, :]
        return self._add_receivers(alias, capsules, patterns, capsule_names, {})

    def add_foa_listener(self, alias: str, position, order: str = "wyzx") -> MicArray:
        """One point with the four channels of first-order ambisonics (the reference's ``FOAListener``, micarrays.py:371-394), SN3D
        weights, channels in ``order`` ("wyzx": AmbiX), axes the room's."""
        from . import shoebox

        patterns = shoebox.foa_patterns(order)
        point = shoebox._points(np.atleast_2d(np.asarray(position, dtype=np.float64)), self.room, f"position of {alias}")
        if len(point) != 1:
            raise ValueError("an FOA listener is one point")
        return self._add_receivers(alias, point, patterns[None, :, :], list(order.lower()),
                                   dict(micarray_type="FOAListener", channel_layout_type="foa"))

    def add_sphere_microphone(self, alias: str, centre, directions, radius: float = 0.042, n_orders: Optional[int] = None,
                              half: Optional[int] = None, capsule_names=None) -> MicArray:
        """Capsules on a RIGID SPHERE of ``radius`` metres at ``centre``, capsule c at the unit direction ``directions[c]`` (C, 3; room
        axes, normalised here): an array whose body scatters (DESIGN.md "Shoebox IRs: rigid-sphere receivers").  The default radius
        is that of the 4.2 cm arrays; no array geometry is shipped, the directions are the caller's.  ``n_orders`` and ``half``: as
        ``shoebox.sphere_filters`` (None: from the radius and the sample rate).  The capsule coordinates written to the metadata
        are ``centre + radius directions``."""
        from . import shoebox

        return self._add_sphere(alias, centre, shoebox.check_directions(directions), radius, n_orders, half, capsule_names, {})

    def add_binaural_listener(self, alias: str, position, forward=(1.0, 0.0, 0.0), up=(0.0, 0.0, 1.0), radius: float = 0.0875,
                              ear_angle_deg: float = 100.0) -> MicArray:
        """A listener with a SPHERICAL HEAD of ``radius`` metres at ``position``: two channels, left then right, the ears at
        ``+-ear_angle_deg`` from ``forward`` about ``up`` (``shoebox.binaural_directions``; the reference's ``binaural`` channel
        layout).  Level and time differences come from the sphere's scattering; there is no pinna and no torso."""
        from . import shoebox

        ears = shoebox.check_directions(shoebox.binaural_directions(forward, up, ear_angle_deg))      # one policy for every path
        return self._add_sphere(alias, position, ears, radius, None, None, ["left", "right"],
                                dict(micarray_type="Binaural", channel_layout_type="binaural"))

    def _add_sphere(self, alias: str, centre, directions: np.ndarray, radius, n_orders, half, capsule_names, metadata: dict) -> MicArray:
        from . import shoebox

        if self.bands is not None:
            raise ValueError("bands together with a rigid sphere are not yet supported (B x n_orders rows per capsule)")
        if self.tail is not None and self.tail.coherent:
            raise ValueError("a coherent tail on a rigid sphere is not yet supported (its rows are independent draws)")
        centre, radius = shoebox.check_sphere(self.room, centre, radius, self.emitter_positions)
        _, _, _, n_orders, half, _ = shoebox._sphere_plan(radius, float(self.sample_rate), self.c, n_orders, half)
        positions = centre[None, :] + radius * directions
        sphere = dict(centre=centre.tolist(), radius=radius, n_orders=n_orders, half=half, directions=directions.tolist())
        mic = self._add_receivers(alias, positions, None, capsule_names, dict(metadata, is_spherical=True, sphere=sphere))
        self._spheres[alias] = dict(centre=centre, radius=radius, n_orders=n_orders, half=half, directions=directions)
        return mic

    def _add_receivers(self, alias: str, positions: np.ndarray, patterns, capsule_names, metadata: dict) -> MicArray:
        """``positions`` (P, 3) with ``patterns`` None (omni, one channel each) or (P, K, 4): a microphone of P K channels."""
        from . import shoebox

        if alias in self.microphones:
            raise KeyError(f"Microphone with alias {alias} already exists")
        md = dict(micarray_type="MicArray", coordinates_absolute=positions.tolist())
        n_channels = len(positions)
        if patterns is not None:
            patterns = shoebox.check_patterns(patterns, len(positions))
            if self.bands is not None:
                raise ValueError("bands together with patterns are not yet supported (K x B gains per image)")
            n_channels = len(positions) * patterns.shape[1]
            md["patterns"] = patterns.reshape(-1, 4).tolist()      # one row per channel, c = p K + k
        if capsule_names is not None:
            capsule_names = [str(v) for v in capsule_names]
            if len(capsule_names) != n_channels:
                raise ValueError(f"{alias} has {n_channels} channels but {len(capsule_names)} capsule names")
            md["capsule_names"] = capsule_names
        md.update(metadata)
        self._capsules[alias], self._patterns[alias] = positions, patterns
        self.microphones[alias] = MicArray(alias, n_channels, md, n_listeners=len(positions))
        self._irs = None
        return self.microphones[alias]

    def add_emitters(self, positions, alias: Optional[str] = None, patterns=None) -> str:
        """One IR column per row of ``positions`` (n, 3), appended in event order.  ``patterns`` (4,) or (n, 4): a first-order
        pattern ``(w, vx, vy, vz)`` per emitter in room axes (``shoebox.first_order``, ``cardioid``); None: omnidirectional.
        Returns the alias the rows are filed under."""
        from . import shoebox

        alias = alias if alias is not None else f"emitters{len(self.emitters):03d}"
        if alias in self.emitters:
            raise KeyError(f"Emitters with alias {alias} already exist")
        points = shoebox._points(np.atleast_2d(np.asarray(positions, dtype=np.float64)), self.room, f"emitters {alias}")
        for sphere in self._spheres.values():      # the plane-wave model: no emitter closer than 2 radius to a sphere's centre
            shoebox.check_sphere(self.room, sphere["centre"], sphere["radius"], points)
        if patterns is not None:
            self._emitter_patterns[alias] = shoebox.check_source_patterns(patterns, len(points))
        self.emitters[alias] = points
        self._irs = None
        return alias

    @property
    def num_emitters(self) -> int:
        return sum(len(v) for v in self.emitters.values())

    @property
    def emitter_positions(self) -> np.ndarray:
        return np.concatenate(list(self.emitters.values()), axis=0) if self.emitters else np.zeros((0, 3))

    @property
    def emitter_patterns(self) -> Optional[np.ndarray]:
        """(N, 4) in the order of ``emitter_positions`` (omni rows for the aliases without patterns), or None when no emitter has one."""
        from . import shoebox

        if not self._emitter_patterns:
            return None
        return np.concatenate([self._emitter_patterns.get(alias, np.tile(shoebox.omni(), (len(points), 1)))
                               for alias, points in self.emitters.items()], axis=0)

    def simulate(self) -> None:
        from . import shoebox, synthesize

        if not self.microphones:
            raise ValueError("WorldState has no microphones!")
        if not self.emitters:
            raise ValueError("WorldState has no emitters!")
        r = self.renderer or synthesize.get_renderer()
        sources = self.emitter_positions
        irs = OrderedDict()
        capsule_id0 = 0     # the tail's noise: channels are numbered through the microphones, emitters are one table already
        for alias, capsules in self._capsules.items():
            sphere = self._spheres.get(alias)
            if sphere is not None:
                buf, strides, _ = shoebox.shoebox_sphere_irs_device(r, self.room, self.betas, sources, sphere["centre"], sphere["directions"],
                                                                    sphere["radius"], self.ir_len, self.sample_rate, self.c, self.max_order,
                                                                    self.tail, 0, capsule_id0, sphere["n_orders"], sphere["half"],
                                                                    source_patterns=self.emitter_patterns, air=self.air)
            else:
                buf, strides, _ = shoebox.shoebox_irs_device(r, self.room, self.betas, sources, capsules, self.ir_len, self.sample_rate,
                                                             self.c, self.max_order, self.tail, 0, capsule_id0, self._patterns[alias],
                                                             self.bands, source_patterns=self.emitter_patterns, air=self.air)
            n_channels = self.microphones[alias].n_capsules
            irs[alias] = shoebox.DeviceIRTensor(r, buf, strides, (n_channels, len(sources), self.ir_len))
            capsule_id0 += n_channels
        self._irs = irs

    @property
    def irs(self):
        if self._irs is None:
            raise AttributeError("IRs have not been generated yet: call simulate()")
        return self._irs

    def get_irs(self):
        return self.irs

    def metrics(self, alias: Optional[str] = None, edc: bool = False) -> dict:
        """``{alias: acoustics.IRMetrics}`` of the generated tensors, measured where they lie (acoustics.ir_metrics: reverberation
        times, DRR, clarity per row): nothing but the tables is downloaded.  As ``irs``: raises before ``simulate()``.  Not part
        of ``to_dict()``."""
        from . import acoustics

        return acoustics.state_metrics(self, self.sample_rate, alias, edc)

    def band_metrics(self, alias: Optional[str] = None, bands=None, edc: bool = False) -> dict:
        """``{alias: acoustics.IRBandMetrics}``: ``metrics()`` per octave band, split and measured where the tensors lie
        (acoustics.ir_band_metrics).  ``bands`` None: the state's own bands where it has them (a room with ``bands=`` or
        ``materials=`` is measured in the bands it was built in), else the six octave centres.  Not part of ``to_dict()``."""
        from . import acoustics

        return acoustics.state_band_metrics(self, self.sample_rate, alias, self.bands if bands is None else bands, edc)

    def pair_metrics(self, alias: Optional[str] = None, pairs=None, max_lag=None, bands=None, curves: bool = False) -> dict:
        """``{alias: acoustics.IRPairMetrics}``: IACC, ITD and ILD per (capsule pair, emitter), measured where the tensors lie
        (acoustics.ir_pair_metrics; ``pairs`` None: consecutive capsules, the layout of ``add_binaural_listener``).  ``bands``: None
        for the broadband rows; True for the state's own bands where it has them, else the six octave centres; or a
        ``shoebox.ShoeboxBands`` / its dictionary (acoustics.ir_pair_band_metrics).  Not part of ``to_dict()``."""
        from . import acoustics, shoebox

        if bands is True:
            bands = self.bands if self.bands is not None else shoebox.ShoeboxBands()
        return acoustics.state_pair_metrics(self, self.sample_rate, alias, pairs, max_lag, bands, curves)

    def to_dict(self) -> dict:   # worldstate.py:2330-2356 layout, with the room in place of the mesh
        d = dict(backend=self.name, sample_rate=self.sample_rate,
                 emitters={k: v.tolist() for k, v in self.emitters.items()},
                 microphones={k: m.to_dict() for k, m in self.microphones.items()},
                 shoebox=dict(room=self.room.tolist(), betas=self.betas.tolist(), rt60=self.rt60, ir_len=self.ir_len, c=self.c,
                              max_order=self.max_order))
        if self.tail is not None:
            d["shoebox"]["tail"] = self.tail.to_dict()
        if self.bands is not None:      # betas is (6, B) then; the material names are a record, the betas are what is read back
            d["shoebox"]["bands"] = self.bands.to_dict()
            if self.materials is not None:
                d["shoebox"]["materials"] = list(self.materials)
        if self.air is not None:
            d["shoebox"]["air"] = self.air if self.bands is None else self.air.tolist()
        if self._emitter_patterns:      # beside the emitters, whose entry keeps its form
            d["shoebox"]["emitter_patterns"] = {k: v.tolist() for k, v in self._emitter_patterns.items()}
        d.update({k: v for k, v in self.metadata.items() if k not in d})
        return d

    @staticmethod
    def describes(state_d: dict) -> bool:
        """Does this state dictionary carry everything ``from_dict`` needs?"""
        box, mics = state_d.get("shoebox"), state_d.get("microphones") or {}
        return (str(state_d.get("backend", "")).upper() == "SHOEBOX" and isinstance(box, dict)
                and all(k in box for k in ("room", "betas", "ir_len")) and bool(state_d.get("emitters")) and bool(mics)
                and all(isinstance(m, dict) and m.get("coordinates_absolute") is not None for m in mics.values()))

    @classmethod
    def from_dict(cls, state_d: dict, renderer=None) -> "ShoeboxIRState":
        from . import shoebox

        box = state_d["shoebox"]
        keep = {k: v for k, v in state_d.items() if k not in ("backend", "sample_rate", "emitters", "microphones", "shoebox")}
        state = cls(box["room"], betas=box["betas"], ir_len=box["ir_len"], sample_rate=state_d.get("sample_rate") or config.SAMPLE_RATE,
                    c=box.get("c", 343.0), max_order=box.get("max_order"), renderer=renderer, metadata=keep, tail=box.get("tail"),
                    bands=box.get("bands"), air=box.get("air"))
        state.rt60 = box.get("rt60")
        state.materials = None if box.get("materials") is None else [str(v) for v in box["materials"]]
        for alias, md in state_d["microphones"].items():
            positions = shoebox._points(md["coordinates_absolute"], state.room, f"capsules of {alias}")
            sphere = md.get("sphere")
            if sphere is not None:      # capsules on a rigid sphere: the directions as they were written (check_directions takes unit
                # rows as they are, so their bits come back), else from the coordinates
                directions = sphere.get("directions")
                if directions is None:
                    directions = positions - np.asarray(sphere["centre"], dtype=np.float64)[None, :]
                mic = state._add_sphere(alias, sphere["centre"], shoebox.check_directions(directions), sphere["radius"],
                                        sphere.get("n_orders"), sphere.get("half"), md.get("capsule_names"), {})
                mic.metadata.update({k: v for k, v in md.items() if k not in ("n_capsules", "sphere", "coordinates_absolute")})
                continue
            patterns = md.get("patterns")      # one row per channel; several channels share a coordinate row (an FOA listener)
            if patterns is not None:
                patterns = np.asarray(patterns, dtype=np.float64)
                if patterns.ndim != 2 or patterns.shape[1:] != (4,) or len(patterns) % len(positions):
                    raise ValueError(f"patterns of {alias} must be (channels, 4) with a whole number of channels per position")
                patterns = patterns.reshape(len(positions), -1, 4)
            mic = state._add_receivers(alias, positions, patterns, md.get("capsule_names"), {})
            mic.metadata.update({k: v for k, v in md.items() if k not in ("n_capsules",)})
        emitter_patterns = box.get("emitter_patterns") or {}
        for alias, rows in state_d["emitters"].items():
            state.add_emitters(rows, alias, emitter_patterns.get(alias))
        return state


class Scene:
    """Container with the attributes the synthesis functions read (core.py:131-251) and ``generate``."""

    def __init__(self, duration: float, state: StaticIRState, sample_rate: int = config.SAMPLE_RATE,
                 ref_db: float = config.DEFAULT_REF_DB):
        self.duration, self.state, self.sample_rate, self.ref_db = float(duration), state, int(sample_rate), ref_db
        self.events: "OrderedDict[str, Event]" = OrderedDict()
        self.ambience: "OrderedDict[str, object]" = OrderedDict()
        self.audio: Dict[str, np.ndarray] = OrderedDict()
        self.metadata: dict = {}

    def add_event(self, event: Event) -> Event:
        if event.alias in self.events:
            raise KeyError(f"Event with alias {event.alias} already exists")
        self.events[event.alias] = event
        return event

    def add_ambience(self, ambience) -> None:
        self.ambience[ambience.alias] = ambience

    # -- metadata round trip in the REFERENCE's on-disk layout (core.py:2106-2243): everything except the samples
    def to_dict(self) -> dict:
        from datetime import datetime

        state = self.state.to_dict() if hasattr(self.state, "to_dict") else {}
        if state.get("sample_rate") is None:
            state["sample_rate"] = self.sample_rate
        return dict(audiblelight_version=f"audiblelight_amd-{VERSION}", rlr_audio_propagation_version=None,
                    creation_time=datetime.now().strftime("%Y-%m-%d_%H:%M:%S"), duration=self.duration,
                    backend=state.get("backend", getattr(self.state, "name", "static")), sample_rate=self.sample_rate,
                    ref_db=self.ref_db, max_overlap=self.metadata.get("max_overlap"),
                    fg_path=self.metadata.get("fg_path", []), bg_path=self.metadata.get("bg_path", []),
                    ambience={k: a.to_dict() for k, a in self.ambience.items() if hasattr(a, "to_dict")},
                    events={k: e.to_dict() for k, e in self.events.items()}, state=state,
                    class_mapping=self.metadata.get("class_mapping"))

    def to_json(self, path: str) -> None:
        import json

        with open(path, "w") as fh:
            json.dump(self.to_dict(), fh, indent=4, ensure_ascii=False)

    @classmethod
    def from_dict(cls, d: dict, clips: Dict[str, np.ndarray], irs: Optional[Dict[str, np.ndarray]] = None) -> "Scene":
        """Rebuild a scene from the reference's ``Scene.to_dict()`` metadata (core.py:2106-2130; what
        ``Scene.generate`` writes as ``metadata_out.json``) plus the arrays it does not carry: ``clips[event alias]``
        (decoded mono audio, see ``Event.from_dict``) and ``irs[mic alias]`` ((C, N_total, L) tensors in event order:
        ``WorldState.get_irs()``, worldstate.py:2183-2255).  A dataset can so be re-rendered on the GPU from its
        metadata without the placement / ray-tracing stages.  A state written by ``ShoeboxIRState`` (backend "SHOEBOX" with its
        room, emitter positions and capsule coordinates) is rebuilt from the metadata when ``irs`` lacks its microphones: those
        IRs are generated again on the device."""
        from . import ambience as amb_mod

        irs = {} if irs is None else irs
        for k in ("duration", "ref_db", "events", "sample_rate"):
            if k not in d:
                raise KeyError(f"Missing key: '{k}'")
        state_d = d.get("state") or {}
        mic_meta = state_d.get("microphones") or {}
        for mic, md in mic_meta.items():
            if isinstance(md, dict) and mic in irs and md.get("n_capsules") not in (None, np.asarray(irs[mic]).shape[0]):
                raise ValueError(f"Microphone {mic} has {md.get('n_capsules')} capsules in the metadata but its IR tensor "
                                 f"has {np.asarray(irs[mic]).shape[0]}")
        missing = [m for m in mic_meta if m not in irs]
        from_room = bool(missing) and ShoeboxIRState.describes(state_d)   # a shoebox scene carries its room: IRs are generated again
        if missing and not from_room:
            raise KeyError(f"No IR tensor given for microphones {missing}")
        if from_room:
            state = ShoeboxIRState.from_dict(state_d)
        else:
            state = StaticIRState(irs, {k: v for k, v in mic_meta.items() if isinstance(v, dict)},
                                  {k: v for k, v in state_d.items() if k != "microphones"})
        scene = cls(d["duration"], state, sample_rate=d["sample_rate"], ref_db=d["ref_db"])
        scene.metadata = {k: d[k] for k in ("max_overlap", "fg_path", "bg_path", "class_mapping") if k in d}
        total = 0
        for alias, ed in d["events"].items():
            if alias not in clips:
                raise KeyError(f"No clip given for event '{alias}' ({ed.get('filepath')})")
            ev = scene.add_event(Event.from_dict(dict(ed, alias=ed.get("alias", alias)), clips[alias]))
            total += len(ev)
        if from_room and state.num_emitters != total:
            raise ValueError(f"The state has {state.num_emitters} emitter positions, the events need {total}")
        for mic, tensor in ({} if from_room else state.irs).items():
            if tensor.shape[1] != total:
                raise ValueError(f"IR tensor of {mic} has {tensor.shape[1]} emitter columns, the events need {total}")
        for alias, ad in (d.get("ambience") or {}).items():
            scene.add_ambience(amb_mod.Ambience.from_dict(ad))
        return scene

    @classmethod
    def from_json(cls, path: str, clips: Dict[str, np.ndarray], irs: Optional[Dict[str, np.ndarray]] = None) -> "Scene":
        import json

        with open(path) as fh:
            return cls.from_dict(json.load(fh), clips, irs)

    def generate(self, output_dir=None, audio: bool = True, metadata_json: bool = True, metadata_dcase: bool = True,
                 audio_fname: str = "audio_out", metadata_fname: str = "metadata_out", video: bool = False,
                 video_fname: str = "video_out", audio_subtype: str = "PCM_16") -> Dict[str, np.ndarray]:
        """Render every event and mix the scene, with the reference's argument list (core.py:1789-1874).

        ``audio``: render on the GPU and, when ``output_dir`` is given, write ``<audio_fname>_<mic>.wav``: (T, C)
        interleaved frames like ``soundfile.write(mic_audio.T, sr)`` (core.py:1840-1847) in soundfile's default WAV
        subtype ``PCM_16`` (``audio_subtype="FLOAT"`` keeps float32); frames are encoded on the device.
        ``metadata_json``: write ``<metadata_fname>.json`` (``to_dict``) when ``output_dir`` is given.
        ``metadata_dcase``: write ``<metadata_fname>_<mic>.csv`` (``metadata.generate_dcase2024_metadata``, host
        bookkeeping; on by default like the reference, core.py:1794; it needs class indices and emitter positions in the
        events' metadata and raises the reference's error without them: pass ``metadata_dcase=False`` for events built from
        bare arrays).  ``video`` belongs to a host-side subsystem that is out of scope: asking for it raises
        instead of silently skipping.
        """
        if video:
            raise NotImplementedError("video output is a host-side feature of the reference (core.py:1866) and is not "
                                      "part of this path")
        import os

        if output_dir is not None:
            os.makedirs(output_dir, exist_ok=True)
        if audio:
            from . import synthesize

            synthesize.render_audio_for_all_scene_events(self)
            synthesize.generate_scene_audio_from_events(self)
            if output_dir is not None:
                from scipy.io import wavfile

                stem = os.path.splitext(str(audio_fname))[0]
                for mic in self.audio:
                    frames = synthesize.encode_scene_frames(self, mic, audio_subtype)
                    wavfile.write(os.path.join(output_dir, f"{stem}_{mic}.wav"), self.sample_rate, frames)
        if metadata_json and output_dir is not None:
            self.to_json(os.path.join(output_dir, os.path.splitext(str(metadata_fname))[0] + ".json"))
        if metadata_dcase and output_dir is not None:       # one CSV per microphone, no header (core.py:1864-1874)
            from . import metadata

            stem = os.path.splitext(str(metadata_fname))[0]
            for mic, df in metadata.generate_dcase2024_metadata(self).items():
                df.to_csv(os.path.join(output_dir, f"{stem}_{mic}.csv"), sep=",", encoding="utf-8", header=None)
        return self.audio
