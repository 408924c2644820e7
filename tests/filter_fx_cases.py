"""Scenarios of the device filter FX (LowpassFilter, HighpassFilter, LowShelfFilter, HighShelfFilter, MultibandEqualizer) and
of their entry point ``al_fx_sos``, shared by tests/test_hostemu_filter_fx.py (host emulation) and tests/test_gpu_filter_fx.py
(gfx950 build).  Every scenario takes the renderer ``r`` the package is set to.

The oracle is ``scipy.signal.sosfilt`` in float64 on float64 SOS rows built HERE, from this module's own transcription of the
definitions (first-order low/high-pass with n = tan(pi fc / fs); Audio EQ Cookbook shelves and peaks written in the cookbook's
own 2 sqrt(A) alpha form), so the package is not checked against itself.  Beside it, checks that do not depend on the formulas
at all: steady-state sinusoid gains at the cutoff and on both sides of a shelf.
"""
import json
import os

import numpy as np
import pytest
from scipy import signal as sps
from scipy import stats

from audiblelight_amd import _hip, augmentation as aug, core
from oracle import synth_oracle as orc
from tests import kernel_edges as ke
from tests.conftest import assert_parity, rel_rms

FS = (16000, 24000, 44100, 48000)
TOL = 1e-5      # HARD[0] misses this with float32 state even when only the stored state is rounded (1.3e-5)
EDGE_SOS_N = (1, 2, 3, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 16383, 16384, 16385, 2 ** 20 + 7)
CLIP_10S, CLIP_60S = 10 * 48000, 60 * 48000


# ----------------------------------------------------------------------------- the oracle's own transcription
def ref_sos(kind, fs, fc, gain_db=0.0, q=1.0):
    """(sos rows (K, 6) float64, scalar) of ONE filter stage; degenerate cutoffs are the constant gain of the stage."""
    nyq = fs / 2.0
    lin = 10.0 ** (gain_db / 20.0)
    if kind in ("lowpass", "highpass"):
        if fc == 0 or fc >= nyq:
            passes = (kind == "lowpass") == (fc >= nyq)
            return np.zeros((0, 6)), 1.0 if passes else 0.0
        k = np.tan(np.pi * fc / fs)
        b = [k, k, 0.0] if kind == "lowpass" else [1.0, -1.0, 0.0]
        return np.array([b + [1.0 + k, k - 1.0, 0.0]]), 1.0
    if fc == 0 or fc >= nyq:
        if kind == "peak":
            return np.zeros((0, 6)), 1.0
        boosted = (kind == "lowshelf") == (fc >= nyq)
        return np.zeros((0, 6)), lin if boosted else 1.0
    A = np.sqrt(lin)
    w0 = 2.0 * np.pi * fc / fs
    cs, sn = np.cos(w0), np.sin(w0)
    alpha = sn / (2.0 * q)
    if kind == "peak":
        b = [1.0 + alpha * A, -2.0 * cs, 1.0 - alpha * A]
        a = [1.0 + alpha / A, -2.0 * cs, 1.0 - alpha / A]
    else:
        t = 2.0 * np.sqrt(A) * alpha
        sgn = 1.0 if kind == "lowshelf" else -1.0     # the high shelf: A-1 -> -(A-1) in every cos term
        b = [A * ((A + 1) - sgn * (A - 1) * cs + t), sgn * 2 * A * ((A - 1) - sgn * (A + 1) * cs),
             A * ((A + 1) - sgn * (A - 1) * cs - t)]
        a = [(A + 1) + sgn * (A - 1) * cs + t, -sgn * 2 * ((A - 1) + sgn * (A + 1) * cs), (A + 1) + sgn * (A - 1) * cs - t]
    return np.array([b + a]), 1.0


def ref_stages(fx):
    """The oracle's stages for one augmentation object, from its params."""
    p, fs = fx.params, fx.sample_rate
    name = type(fx).__name__
    if name == "LowpassFilter":
        return [ref_sos("lowpass", fs, p["cutoff_frequency_hz"])]
    if name == "HighpassFilter":
        return [ref_sos("highpass", fs, p["cutoff_frequency_hz"])]
    if name in ("LowShelfFilter", "HighShelfFilter"):
        kind = "lowshelf" if name.startswith("Low") else "highshelf"
        return [ref_sos(kind, fs, p["cutoff_frequency_hz"], p["gain_db"], p["q"])]
    assert name == "MultibandEqualizer"
    return [ref_sos("peak", fs, f, g, q) for g, f, q in zip(p["gain_db"], p["cutoff_frequency_hz"], p["q"])]


def ref_apply(x, stages):
    y = np.asarray(x, dtype=np.float64)
    for rows, k in stages:
        y = y * k
        if len(rows):
            y = sps.sosfilt(rows / rows[:, 3:4], y)
    return y


def ref_fx(fx, x):
    if isinstance(fx, aug._FilterFX):
        return ref_apply(x, ref_stages(fx))
    if isinstance(fx, aug.Gain):
        return np.asarray(x, dtype=np.float64) * 10.0 ** (fx.gain_db / 20.0)
    if isinstance(fx, aug.Invert):
        return -np.asarray(x, dtype=np.float64)
    raise AssertionError(type(fx))


def noise(n, seed):
    return np.random.default_rng(seed).uniform(-1, 1, n).astype(np.float32)


# ----------------------------------------------------------------------------- 1. every class at every rate
def class_cases(fs):
    """(label, augmentation) per class at `fs`, parameters inside the reference's default ranges where fs allows."""
    nyq = fs / 2
    return [
        ("lowpass", aug.LowpassFilter(fs, cutoff_frequency_hz=min(5512.0, 0.45 * fs))),
        ("lowpass_near_nyquist", aug.LowpassFilter(fs, cutoff_frequency_hz=0.98 * nyq)),
        ("highpass", aug.HighpassFilter(fs, cutoff_frequency_hz=32.0)),
        ("highpass_1k", aug.HighpassFilter(fs, cutoff_frequency_hz=1024.0)),
        ("lowshelf", aug.LowShelfFilter(fs, gain_db=-20.0, cutoff_frequency_hz=300.0, q=0.1)),
        ("lowshelf_32", aug.LowShelfFilter(fs, gain_db=10.0, cutoff_frequency_hz=32.0, q=1.0)),
        ("highshelf", aug.HighShelfFilter(fs, gain_db=8.0, cutoff_frequency_hz=0.7 * nyq, q=0.5)),
        ("eq", aug.MultibandEqualizer(fs, n_bands=5, gain_db=[-20.0, 10.0, 3.0, -6.0, 10.0],
                                      cutoff_frequency_hz=[1024.0, 2000.0, 0.5 * nyq, 0.9 * nyq, 0.99 * nyq],
                                      q=[0.1, 1.0, 0.4, 0.7, 1.0])),
    ]


HARD = [("lowshelf_32Hz_q1_+10dB", lambda: aug.LowShelfFilter(44100, gain_db=10.0, cutoff_frequency_hz=32.0, q=1.0)),
        ("eq_22000Hz_q1_+10dB", lambda: aug.MultibandEqualizer(44100, n_bands=1, gain_db=10.0, cutoff_frequency_hz=22000.0, q=1.0))]


def check_fx(fx, x, tol=TOL, what=None):
    got = fx(x)
    assert got.dtype == np.float32 and got.shape == x.shape
    want = ref_fx(fx, x)
    err = rel_rms(got, want)
    assert err <= tol, (what, err)
    assert_parity(got, want, what=what)
    return err


def run_class_parity(fs, seconds=1.0):
    x = noise(int(seconds * fs), fs)
    for label, fx in class_cases(fs):
        check_fx(fx, x, what=(fs, label))


def run_hard_case(label, seconds=3.0):
    fx = dict(HARD)[label]()
    x = noise(int(seconds * 44100), 7)
    return check_fx(fx, x, what=label)


# ----------------------------------------------------------------------------- steady-state sinusoids (formula-free)
def sine_gain(fx, f, fs, seconds=1.0):
    """|H(f)| measured on the device output: least-squares fit of a sine and a cosine at f over the second half."""
    t = np.arange(int(seconds * fs)) / fs
    y = fx(np.sin(2 * np.pi * f * t).astype(np.float32)).astype(np.float64)
    h = len(t) // 2
    basis = np.stack([np.sin(2 * np.pi * f * t[h:]), np.cos(2 * np.pi * f * t[h:])], 1)
    coef = np.linalg.lstsq(basis, y[h:], rcond=None)[0]
    return float(np.hypot(*coef))


def run_sinusoid_gains(fs=48000):
    for fc in (100.0, 1000.0, 9000.0):
        assert sine_gain(aug.LowpassFilter(fs, cutoff_frequency_hz=fc), fc, fs) == pytest.approx(2 ** -0.5, rel=1e-4)
        assert sine_gain(aug.HighpassFilter(fs, cutoff_frequency_hz=fc), fc, fs) == pytest.approx(2 ** -0.5, rel=1e-4)
    for g, fc, q in ((10.0, 1000.0, 1.0), (-20.0, 5000.0, 0.3), (6.0, 15000.0, 0.7)):
        eq = aug.MultibandEqualizer(fs, n_bands=1, gain_db=g, cutoff_frequency_hz=fc, q=q)
        assert sine_gain(eq, fc, fs) == pytest.approx(10 ** (g / 20), rel=1e-4)
    for g in (10.0, -20.0):
        lo = aug.LowShelfFilter(fs, gain_db=g, cutoff_frequency_hz=400.0, q=0.7)
        hi = aug.HighShelfFilter(fs, gain_db=g, cutoff_frequency_hz=4000.0, q=0.7)
        assert sine_gain(lo, 20.0, fs, 2.0) == pytest.approx(10 ** (g / 20), rel=3e-3)      # boosted side
        assert sine_gain(lo, 16000.0, fs) == pytest.approx(1.0, rel=3e-3)                   # far side
        assert sine_gain(hi, 20000.0, fs) == pytest.approx(10 ** (g / 20), rel=2e-2)
        assert sine_gain(hi, 100.0, fs) == pytest.approx(1.0, rel=3e-3)


# ----------------------------------------------------------------------------- 2. edge lengths through the C ABI
def edge_rows(k, fs=48000):
    """k sections: a mix of every kind, first-order ones included; gains alternate so the cascade stays near unit level."""
    rows = []
    for i in range(k):
        kind = ("peak", "lowshelf", "highshelf", "lowpass", "highpass", "peak")[i % 6]
        fc = (1200.0, 150.0, 9000.0, 15000.0, 40.0, 20000.0)[i % 6] * (1 + 0.01 * i)
        r, _ = ref_sos(kind, fs, fc, (8.0 if i % 2 else -8.0), 0.3 + 0.05 * (i % 10))
        rows.append(r[0])
    return np.array(rows)


def run_sos_edges(r, n, k, shift=0, in_place=False):
    """al_fx_sos on n samples and k sections into a guarded buffer (G sentinel floats on each side), out of place or in place;
    more than AL_SOS_MAX_SECTIONS sections are split over calls exactly as augmentation._sos does."""
    x = ke.signal(n, 1000 + n + k, special=True)
    rows = edge_rows(k)
    out = ke.Guarded(r, n, shift=shift, init=x if in_place else None)
    src = out.buf if in_place else ke.dev(r, x)
    src_ptr = out.ptr if in_place else r.mem.ptr(src)
    for k0 in range(0, k, _hip.SOS_MAX_SECTIONS):
        part = np.ascontiguousarray(rows[k0:k0 + _hip.SOS_MAX_SECTIONS])
        r.lib.call("al_fx_sos", src_ptr if k0 == 0 else out.ptr, out.ptr, n, part.ctypes.data, len(part), r.mem.stream())
    got = out.get()
    want = sps.sosfilt(rows / rows[:, 3:4], x.astype(np.float64))
    # float64 state: the error is the float32 rounding of the output and of the k-1 intermediate signals, each carried
    # through the rest of the cascade (gains <= +8 dB per section, alternating)
    ke.record("sos cascade", ke.peak_error(got, want), 1e-6 * max(k, 1))
    if n >= 64:
        assert rel_rms(got, want) <= 1e-6 * max(k, 1)
    return got


def run_sos_long(r, n, k):
    x = noise(n, 99)
    rows = edge_rows(k)
    d = ke.dev(r, x)
    r.lib.call("al_fx_sos", r.mem.ptr(d), r.mem.ptr(d), n, np.ascontiguousarray(rows).ctypes.data, k, r.mem.stream())
    r.mem.synchronize()
    got = np.asarray(r.mem.download(d))[:n]
    want = sps.sosfilt(rows / rows[:, 3:4], x.astype(np.float64))
    assert rel_rms(got, want) <= TOL
    assert_parity(got, want, what=(n, k))


# ----------------------------------------------------------------------------- 3. degenerate cutoffs, argument errors
def run_degenerate_cutoffs():
    for fs in (16000, 24000, 48000):
        x = noise(3000, fs)
        nyqs = (fs / 2, fs / 2 + 1.0, 22050.0 if fs <= 44100 else 2.0 * fs)
        lin = np.float32(10 ** (7.0 / 20))
        cases = [(aug.LowpassFilter(fs, cutoff_frequency_hz=0), 0.0)]
        cases += [(aug.LowpassFilter(fs, cutoff_frequency_hz=f), 1.0) for f in nyqs]
        cases += [(aug.HighpassFilter(fs, cutoff_frequency_hz=0), 1.0)]
        cases += [(aug.HighpassFilter(fs, cutoff_frequency_hz=f), 0.0) for f in nyqs]
        cases += [(aug.LowShelfFilter(fs, gain_db=7.0, cutoff_frequency_hz=0, q=0.5), 1.0)]
        cases += [(aug.LowShelfFilter(fs, gain_db=7.0, cutoff_frequency_hz=f, q=0.5), lin) for f in nyqs]
        cases += [(aug.HighShelfFilter(fs, gain_db=7.0, cutoff_frequency_hz=0, q=0.5), lin)]
        cases += [(aug.HighShelfFilter(fs, gain_db=7.0, cutoff_frequency_hz=f, q=0.5), 1.0) for f in nyqs]
        cases += [(aug.MultibandEqualizer(fs, n_bands=2, gain_db=7.0, cutoff_frequency_hz=[0, f], q=1.0), 1.0) for f in nyqs]
        for fx, k in cases:
            got = fx(x)
            assert got.dtype == np.float32
            if k == 1.0:
                ke.assert_bits_equal(got, x, fx)          # the identity is not even launched
            else:
                np.testing.assert_array_equal(got, x * np.float32(k), err_msg=repr(fx))   # one float32 multiply
            assert rel_rms(got, ref_fx(fx, x)) <= 1e-7
    # a degenerate stage in front of real ones is folded into their numerator
    fx = aug.MultibandEqualizer(48000, n_bands=3, gain_db=[4.0, -3.0, 2.0], cutoff_frequency_hz=[0.0, 3000.0, 30000.0], q=0.7)
    x = noise(5000, 1)
    assert rel_rms(fx(x), ref_fx(fx, x)) <= TOL


def run_argument_errors():
    for cls in (aug.LowShelfFilter, aug.HighShelfFilter):
        with pytest.raises(ValueError, match="q"):
            cls(48000, gain_db=3.0, cutoff_frequency_hz=500.0, q=0)
        with pytest.raises(ValueError, match="positive"):
            cls(48000, gain_db=3.0, cutoff_frequency_hz=500.0, q=-0.5)
        with pytest.raises(ValueError, match="positive"):
            cls(48000, gain_db=3.0, cutoff_frequency_hz=-1.0, q=0.5)
        with pytest.raises(TypeError):
            cls(48000, gain_db=3.0, cutoff_frequency_hz="500", q=0.5)
    for cls in (aug.LowpassFilter, aug.HighpassFilter):
        with pytest.raises(ValueError, match="positive"):
            cls(48000, cutoff_frequency_hz=-100.0)
    with pytest.raises(ValueError, match="q"):
        aug.MultibandEqualizer(48000, n_bands=2, gain_db=1.0, cutoff_frequency_hz=1000.0, q=[1.0, 0.0])
    with pytest.raises(ValueError, match="positive"):
        aug.MultibandEqualizer(48000, n_bands=2, gain_db=1.0, cutoff_frequency_hz=[1000.0, -5.0], q=1.0)
    with pytest.raises(ValueError, match="positive"):
        aug.MultibandEqualizer(48000, n_bands=-2)


# ----------------------------------------------------------------------------- 4. C ABI refusals
def run_abi_refusals(r):
    x = ke.dev(r, noise(256, 3))
    ok = np.array([[0.2, 0.3, 0.1, 1.0, -0.5, 0.2]])

    def call(rows, n=256, k=None):
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        return r.lib.call("al_fx_sos", r.mem.ptr(x), r.mem.ptr(x), n, rows.ctypes.data, len(rows) if k is None else k,
                          r.mem.stream())

    def refused(match, *args, **kw):
        with pytest.raises(_hip.HipError, match=match):
            call(*args, **kw)
        assert match.split("|")[0] in r.lib.last_error(), r.lib.last_error()

    refused("n must be >= 1", ok, n=0)
    refused("n must be >= 1", ok, n=-5)
    refused("n_sections", ok, k=0)
    refused("n_sections", np.repeat(ok, 17, 0))
    refused("a0 == 0", [[1.0, 0.0, 0.0, 0.0, 0.5, 0.0]])
    for bad in (np.nan, np.inf, -np.inf):
        for col in range(6):
            row = ok.copy()
            row[0, col] = bad
            refused("non-finite", row)
    refused("non-finite", [[1.0, 0.0, 0.0, 1e-320, 0.5, 0.0]])      # finite, but not after the division by a0
    refused("section 2 has a pole", np.concatenate([ok, ok, [[1.0, 0.0, 0.0, 1.0, -1.0, 0.0]]]))   # pole at z = 1
    refused("pole", [[1.0, 0.0, 0.0, 1.0, 1.0, 0.0]])               # z = -1
    refused("pole", [[1.0, 0.0, 0.0, 1.0, 0.0, 1.0]])               # |z| = 1, complex pair
    refused("pole", [[1.0, 0.0, 0.0, 1.0, -2.5, 1.5]])              # z = 1, 1.5
    refused("pole", [[1.0, 0.0, 0.0, 2.0, 0.0, -2.0]])              # z = +-1
    assert call(np.repeat(ok, 16, 0)) == 0                            # the cap itself is accepted
    assert call([[1.0, 0.0, 0.0, 1.0, -1.999, 0.9991]]) == 0          # poles just inside the unit circle


# ----------------------------------------------------------------------------- 5. the classes
def run_class_api():
    assert all(c in aug.ALL_EVENT_AUGMENTATIONS for c in (aug.LowpassFilter, aug.HighpassFilter, aug.LowShelfFilter,
                                                          aug.HighShelfFilter, aug.MultibandEqualizer))
    for cls, keys in ((aug.LowpassFilter, ["cutoff_frequency_hz"]), (aug.HighpassFilter, ["cutoff_frequency_hz"]),
                      (aug.LowShelfFilter, ["cutoff_frequency_hz", "gain_db", "q"]),
                      (aug.HighShelfFilter, ["cutoff_frequency_hz", "gain_db", "q"]),
                      (aug.MultibandEqualizer, ["n_bands", "gain_db", "cutoff_frequency_hz", "q"])):
        for seed in range(20):
            np.random.seed(seed)
            a = cls(44100)
            np.random.seed(seed)
            b = cls(44100)
            assert a == b and a.to_dict() == b.to_dict()
            assert list(a.params) == keys
            d = a.to_dict()
            assert d["name"] == cls.__name__ and d["sample_rate"] == 44100
            again = aug.Augmentation.from_dict(json.loads(json.dumps(d)))
            assert type(again) is cls and again == a and again.to_dict() == d
            if cls is aug.MultibandEqualizer:
                assert isinstance(a.n_bands, int) and 1 <= a.n_bands <= 7
                ranges = [("gain_db", cls.MIN_GAIN, cls.MAX_GAIN), ("cutoff_frequency_hz", cls.MIN_FREQ, cls.MAX_FREQ),
                          ("q", cls.MIN_Q, cls.MAX_Q)]
                for key, lo, hi in ranges:
                    assert len(d[key]) == a.n_bands and all(lo <= v <= hi for v in d[key])
            else:
                assert cls.MIN_FREQ <= a.cutoff_frequency_hz <= cls.MAX_FREQ
                if "q" in keys:
                    assert cls.MIN_GAIN <= a.gain_db <= cls.MAX_GAIN and cls.MIN_Q <= a.q <= cls.MAX_Q
    assert (aug.LowpassFilter.MIN_FREQ, aug.LowpassFilter.MAX_FREQ) == (5512, 22050)
    assert (aug.HighpassFilter.MIN_FREQ, aug.HighpassFilter.MAX_FREQ) == (32, 1024)
    assert (aug.LowShelfFilter.MIN_FREQ, aug.LowShelfFilter.MAX_FREQ) == (32, 1024)
    assert (aug.HighShelfFilter.MIN_FREQ, aug.HighShelfFilter.MAX_FREQ) == (5512, 22050)
    # n_bands is truncated by int; every value of the default draw is 1..7
    assert aug.MultibandEqualizer(48000, n_bands=3.9).n_bands == 3
    drawn = set()
    for seed in range(200):
        np.random.seed(seed)
        drawn.add(aug.MultibandEqualizer(48000).n_bands)
    assert drawn == set(range(1, 8))
    # per-band values: scalar, list, ndarray, distribution
    eq = aug.MultibandEqualizer(48000, n_bands=3, gain_db=2.5, cutoff_frequency_hz=np.array([1000.0, 2000.0, 3000.0]),
                                q=stats.uniform(0.2, 0.1))
    assert eq.gain_db == [2.5, 2.5, 2.5] and eq.cutoff_frequency_hz == [1000.0, 2000.0, 3000.0]
    assert isinstance(eq.cutoff_frequency_hz, list) and len(set(eq.q)) == 3 and all(0.2 <= v <= 0.3 for v in eq.q)
    with pytest.raises(ValueError, match="Expected 3 values but got 2"):
        aug.MultibandEqualizer(48000, n_bands=3, gain_db=[1.0, 2.0])
    with pytest.raises(TypeError, match="Cannot handle type"):
        aug.MultibandEqualizer(48000, n_bands=3, q="sharp")
    with pytest.raises(TypeError):
        aug.LowpassFilter(48000, cutoff_frequency_hz="high")
    # the reference's on-disk layout loads
    ref_dicts = [dict(name="LowpassFilter", sample_rate=44100, cutoff_frequency_hz=8000.0),
                 dict(name="HighShelfFilter", sample_rate=44100, cutoff_frequency_hz=9000.0, gain_db=-4.0, q=0.5),
                 dict(name="MultibandEqualizer", sample_rate=44100, n_bands=2, gain_db=[1.0, -2.0],
                      cutoff_frequency_hz=[1500.0, 7000.0], q=[0.3, 0.9])]
    for d in ref_dicts:
        fx = aug.Augmentation.from_dict(d)
        assert fx.to_dict() == d
    assert aug.LowpassFilter(44100, 8000.0).host_dtype(np.dtype(np.float64)) == np.float32


# ----------------------------------------------------------------------------- 6. a chain on an Event, and in a scene
def chain(sr):
    return [aug.HighpassFilter(sr, cutoff_frequency_hz=150.0), aug.Gain(sr, gain_db=-3.5),
            aug.MultibandEqualizer(sr, n_bands=3, gain_db=[6.0, -12.0, 9.0], cutoff_frequency_hz=[500.0, 1800.0, 3500.0],
                                   q=[0.7, 0.3, 1.0])]


def oracle_chain(raw, fxs):
    y = np.asarray(raw, dtype=np.float64)
    for fx in fxs:
        y = ref_fx(fx, y)
    return orc.peak_normalise_clip(y)


def run_event_chain(r):
    sr = 8000
    rng = np.random.default_rng(5)
    raw = (rng.standard_normal(6000) * 0.4).astype(np.float32)
    fxs = chain(sr)
    ev = core.Event("f", raw, sr, augmentations=fxs)
    got = ev.load_audio()
    want = oracle_chain(raw, fxs)
    assert rel_rms(got, want) <= TOL
    assert_parity(got, want)
    # through a scene render: one upload (the staging arena), zero downloads
    C, L = 3, 600
    irs = (rng.standard_normal((C, 2, L)) * np.exp(-np.arange(L) / 120.0)).astype(np.float32)
    raws = [raw, (rng.standard_normal(5000) * 1.5).astype(np.float32)]
    chains = [chain(sr), [aug.LowShelfFilter(sr, gain_db=6.0, cutoff_frequency_hz=200.0, q=0.6), aug.Invert(sr)]]
    scene = core.Scene(1.5, core.StaticIRState({"mic000": irs}), sample_rate=sr, ref_db=-65)
    for i, (x, c) in enumerate(zip(raws, chains)):
        scene.add_event(core.Event(f"e{i}", x, sr, snr=8.0 + 3 * i, scene_start=0.2 * i, augmentations=c))
    scene.generate()
    spatials = []
    for i, ev in enumerate(scene.events.values()):
        want = orc.render_event(oracle_chain(raws[i], chains[i]), irs[:, [i], :].astype(np.float64), ev.snr, sr=sr)["spatial"]
        spatials.append(want)
        assert_parity(ev.spatial_audio["mic000"], want, what=ev.alias)
        assert ev.audio is None
        clip = ev._last_chain
        assert clip.uploads == 1 and clip.downloads == 0
    ref = orc.mix_scene(spatials, [(e.scene_start, e.scene_end) for e in scene.events.values()], 1.5, sr, keep_padded=False)
    assert_parity(scene.audio["mic000"], ref["scene"])


# ----------------------------------------------------------------------------- 7. a reference scene JSON with filter FX
def run_scene_json(tmp_path):
    here = os.path.join(os.path.dirname(__file__), "golden")
    z = np.load(os.path.join(here, "reference_scene_arrays.npz"))
    meta = json.load(open(os.path.join(here, "reference_scene.json")))
    sr = meta["sample_rate"]
    injected = {
        "event000": [dict(name="LowpassFilter", sample_rate=sr, cutoff_frequency_hz=2500.0),
                     dict(name="HighShelfFilter", sample_rate=sr, cutoff_frequency_hz=1500.0, gain_db=-6.0, q=0.8),
                     dict(name="LowShelfFilter", sample_rate=sr, cutoff_frequency_hz=5512.0, gain_db=3.0, q=0.4)],
        "event001": [dict(name="HighpassFilter", sample_rate=sr, cutoff_frequency_hz=300.0),
                     dict(name="MultibandEqualizer", sample_rate=sr, n_bands=3, gain_db=[8.0, -10.0, 4.0],
                          cutoff_frequency_hz=[700.0, 2200.0, 22050.0], q=[0.5, 1.0, 0.2])],
    }
    for alias, extra in injected.items():
        meta["events"][alias]["augmentations"] = meta["events"][alias]["augmentations"] + extra
    path = tmp_path / "scene_with_filters.json"
    path.write_text(json.dumps(meta))
    clips = {a: z[f"clip_{a}"] for a in meta["events"]}
    irs = {m: z[f"irs_{m}"] for m in meta["state"]["microphones"]}
    scene = core.Scene.from_json(str(path), clips, irs)
    assert [type(a).__name__ for a in scene.events["event001"].augmentations] == ["Gain", "Invert", "HighpassFilter",
                                                                                  "MultibandEqualizer"]
    out = scene.generate()
    cols = {"event000": 0, "event001": 1}          # one emitter each, the first two IR columns
    for mic in irs:
        old, new, slots = [], [], []
        for alias, col in cols.items():
            ev = scene.events[alias]
            want_clip = oracle_chain(clips[alias], ev.augmentations)
            want = orc.render_event(want_clip, irs[mic][:, [col], :].astype(np.float64), ev.snr, ref_db=meta["ref_db"],
                                    sr=sr)["spatial"]
            assert_parity(ev.spatial_audio[mic], want, what=(mic, alias))
            old.append(z[f"spatial_{mic}_{alias}"].astype(np.float64))
            new.append(want)
            slots.append((ev.scene_start, ev.scene_end))
        # the reference's scene with the two unfiltered contributions replaced by the oracle-filtered ones
        swap = (orc.mix_scene(new, slots, meta["duration"], sr, keep_padded=False)["scene"].astype(np.float64)
                - orc.mix_scene(old, slots, meta["duration"], sr, keep_padded=False)["scene"])
        assert_parity(out[mic], z[f"scene_{mic}"].astype(np.float64) + swap, what=mic)
