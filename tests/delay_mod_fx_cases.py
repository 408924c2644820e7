"""Scenarios of the device delay and modulation FX (Delay, Chorus, Phaser) and of their entry points ``al_fx_delay``,
``al_fx_chorus`` and ``al_fx_phaser``, shared by tests/test_hostemu_delay_mod_fx.py (host emulation) and
tests/test_gpu_delay_mod_fx.py (gfx950 build).  Every scenario takes the renderer ``r`` the package is set to.

The oracle is a plain float64 restatement of the definitions written HERE (DESIGN.md "Delay and modulation FX"), so the
package is not checked against itself: Delay through ``scipy.signal.lfilter`` (short lines) or the same recursion a line
length at a time (long ones), Chorus and Phaser as sample loops.
"""
import json
import math
import os

import numpy as np
import pytest
from scipy import signal as sps

from audiblelight_amd import _hip, augmentation as aug, core
from oracle import synth_oracle as orc
from tests import filter_fx_cases as ffc
from tests import kernel_edges as ke
from tests.conftest import assert_parity, parity_errors

FS = (16000, 24000, 44100, 48000)
TOL = 1e-5
EDGE_N = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 16385)
CLIP_10S, CLIP_60S = 10 * 48000, 60 * 48000


# ----------------------------------------------------------------------------- the oracle
def ref_delay(x, D, fb, mix):
    """d[t] = x[t - D] + fb d[t - D] (d = 0 before the line fills; D = 0 or D >= n: d = 0), y = (1 - mix) x + mix d."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    d = np.zeros(n)
    if 1 <= D < n:
        if D <= 64:
            b = np.zeros(D + 1)
            b[D] = 1.0
            a = np.zeros(D + 1)
            a[0], a[D] = 1.0, -fb
            d = sps.lfilter(b, a, x)
        else:
            for s in range(D, n, D):
                e = min(s + D, n)
                d[s:e] = x[s - D:e - D] + fb * d[s - D:e - D]
    return (1.0 - mix) * x + mix * d


def ref_chorus(x, fs, rate_hz, depth, centre_delay_ms, feedback, mix):
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    t = np.arange(n, dtype=np.float64)
    lfo = np.sin(2.0 * np.pi * rate_hz * t / fs - np.pi)
    tau = np.clip(np.maximum(1.0, 10.0 * depth * lfo + centre_delay_ms) * fs / 1000.0, 0.0, math.ceil(110.0 * fs / 1000.0))
    i = np.floor(tau).astype(np.int64)
    f = tau - i
    m = min(mix, 1.0)
    if feedback == 0.0:
        idx = np.arange(n) - i
        u0 = np.where(idx >= 0, x[np.maximum(idx, 0)], 0.0)
        u1 = np.where(idx >= 1, x[np.maximum(idx - 1, 0)], 0.0)
        v = u0 + f * (u1 - u0)
    else:
        xs, il, fl = x.tolist(), i.tolist(), f.tolist()
        u = [0.0] * n
        v = [0.0] * n
        vprev = 0.0
        for k in range(n):
            a = k - il[k]
            u0 = u[a] if a >= 0 else 0.0
            u1 = u[a - 1] if a >= 1 else 0.0
            v[k] = u0 + fl[k] * (u1 - u0)
            u[k] = xs[k] - feedback * vprev
            vprev = v[k]
        v = np.array(v)
    return (1.0 - m) * x + m * v


def ref_phaser(x, fs, rate_hz, depth, centre_frequency_hz, feedback, mix):
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    fmax = min(20000.0, 0.49 * fs)
    with np.errstate(divide="ignore"):
        c = np.log10(centre_frequency_hz / 20.0) / np.log10(fmax / 20.0)
    k = np.arange((n + 3) // 4, dtype=np.float64)
    lfo = np.clip(0.5 * depth * np.sin(2.0 * np.pi * rate_hz * 4.0 * k / fs - np.pi) + c, 0.0, 1.0)
    g = np.tan(np.pi * 20.0 * (fmax / 20.0) ** lfo / fs)
    Gs = np.repeat(g / (1.0 + g), 4)[:n].tolist()
    s = [0.0] * 6
    L = 0.0
    wet = [0.0] * n
    for t, xt in enumerate(x.tolist()):
        G = Gs[t]
        inp = xt - L
        for q in range(6):
            v = G * (inp - s[q])
            lp = v + s[q]
            s[q] = lp + v
            inp = 2.0 * lp - inp
        L = feedback * inp
        wet[t] = inp
    m = min(mix, 1.0)
    return (1.0 - m) * x + m * np.array(wet)


def ref_fx(fx, x):
    p, fs = fx.params, fx.sample_rate
    if isinstance(fx, aug.Delay):
        if p["delay_seconds"] == 0:
            return np.asarray(x, dtype=np.float64)
        D = min(int(p["delay_seconds"] * fs), 30 * fs)
        return ref_delay(x, D, p["feedback"], p["mix"])
    if isinstance(fx, aug.Chorus):
        return ref_chorus(x, fs, p["rate_hz"], p["depth"], p["centre_delay_ms"], p["feedback"], p["mix"])
    if isinstance(fx, aug.Phaser):
        return ref_phaser(x, fs, p["rate_hz"], p["depth"], p["centre_frequency_hz"], p["feedback"], p["mix"])
    return ffc.ref_fx(fx, x)


def noise(n, seed):
    return np.random.default_rng(seed).uniform(-1, 1, n).astype(np.float32)


def check(got, want, what=None, tol=TOL):
    rms, mx = parity_errors(got, want)
    assert rms <= tol and mx <= tol, (what, rms, mx)
    return rms, mx


def check_fx(fx, x, what=None):
    got = fx(x)
    assert got.dtype == np.float32 and got.shape == x.shape
    check(got, ref_fx(fx, x), what=(what, fx))


# ----------------------------------------------------------------------------- 1. every class at every rate
def class_cases(fs):
    return [
        ("delay", aug.Delay(fs, delay_seconds=0.0123, feedback=0.45, mix=0.35)),
        ("delay_short", aug.Delay(fs, delay_seconds=0.5 / fs, feedback=0.9, mix=0.8)),   # D = 0: (1 - mix) x
        ("chorus_ff", aug.Chorus(fs, rate_hz=3.3, depth=0.7, centre_delay_ms=12.5, feedback=0.0, mix=0.4)),
        ("chorus_fb", aug.Chorus(fs, rate_hz=7.1, depth=0.9, centre_delay_ms=4.0, feedback=0.6, mix=0.5)),
        ("chorus_floor", aug.Chorus(fs, rate_hz=1.0, depth=1.0, centre_delay_ms=1.0, feedback=0.3, mix=1.7)),
        ("phaser", aug.Phaser(fs, rate_hz=2.2, depth=0.8, centre_frequency_hz=1300.0, feedback=0.7, mix=0.5)),
        ("phaser_fast", aug.Phaser(fs, rate_hz=10.0, depth=1.0, centre_frequency_hz=260.0, feedback=0.0, mix=1.0)),
    ]


def run_class_parity(fs, seconds=1.0):
    x = noise(int(seconds * fs), fs)
    for label, fx in class_cases(fs):
        check_fx(fx, x, what=(fs, label))


def run_defaults_drawn(fs, seconds=1.0, seeds=range(3)):
    x = noise(int(seconds * fs), fs + 1)
    for seed in seeds:
        for cls in (aug.Delay, aug.Chorus, aug.Phaser):
            np.random.seed(seed)
            check_fx(cls(fs), x, what=(fs, seed))


# ----------------------------------------------------------------------------- 2. Delay line lengths
def delay_lengths(n):
    return (0, 1, 2, 63, 64, 65, n - 1, n, n + 5)


def call_delay(r, src_ptr, dst_ptr, n, D, fb, mix):
    import ctypes as ct

    return r.lib.call("al_fx_delay", src_ptr, dst_ptr, n, D, ct.c_float(fb), ct.c_float(mix), r.mem.stream())


def run_delay_edges(r, n, D, fb=0.7, mix=0.4, shift=0):
    x = ke.signal(n, 500 + n, special=True)
    src = ke.dev(r, x)
    out = ke.Guarded(r, n, shift=shift)
    call_delay(r, r.mem.ptr(src), out.ptr, n, D, fb, mix)
    got = out.get()
    check(got, ref_delay(x, D, float(np.float32(fb)), float(np.float32(mix))), what=(n, D))
    return got


def run_delay_special():
    x = noise(3001, 3)
    ident = aug.Delay(16000, delay_seconds=0, feedback=0.4, mix=0.9)
    ke.assert_bits_equal(ident(x), x, "delay_seconds == 0")
    # over 30 s: the line is clamped to 30 fs (fs = 1000 keeps the clip short)
    fs, n = 1000, 30 * 1000 + 4321
    x = noise(n, 4)
    long = aug.Delay(fs, delay_seconds=41.5, feedback=0.5, mix=0.5)
    assert long.delay_samples == 30 * fs
    got = long(x)
    want = ref_delay(x, 30 * fs, 0.5, 0.5)
    check(got, want, what="clamped")
    assert np.max(np.abs(got[30 * fs:] - 0.5 * x[30 * fs:])) > 0.1     # the echo is there: not the D >= n result


# ----------------------------------------------------------------------------- 3. Chorus regimes
def run_chorus_regimes(fs=48000, seconds=0.5):
    x = noise(int(seconds * fs), 11)
    cases = []
    for fb in (0.0, 0.9):
        cases += [
            aug.Chorus(fs, rate_hz=0.0, depth=0.0, centre_delay_ms=2.0, feedback=fb, mix=0.5),     # tau = 96: integer
            aug.Chorus(fs, rate_hz=0.0, depth=0.5, centre_delay_ms=5.0, feedback=fb, mix=0.5),     # lfo(0) = -0: integer
            aug.Chorus(fs, rate_hz=fs / 1000.0, depth=0.25, centre_delay_ms=3.0, feedback=fb, mix=0.5),   # integer steps
            aug.Chorus(fs, rate_hz=4.0, depth=1.0, centre_delay_ms=20.0, feedback=fb, mix=0.3),
            aug.Chorus(fs, rate_hz=2.0, depth=1.0, centre_delay_ms=105.0, feedback=fb, mix=0.6),   # hits the 110 ms clamp
            aug.Chorus(fs, rate_hz=0.5, depth=0.0, centre_delay_ms=500.0, feedback=fb, mix=0.6),   # always clamped
            aug.Chorus(fs, rate_hz=9.0, depth=0.3, centre_delay_ms=0.0, feedback=fb, mix=1.0),     # always the 1 ms floor
        ]
    for fx in cases:
        check_fx(fx, x, what="chorus")


# ----------------------------------------------------------------------------- 4. Phaser centre frequencies
def run_phaser_centres(fs, n=None):
    n = n if n is not None else int(0.37 * fs) + 3        # neither a multiple of 4 nor of the run length
    x = noise(n, fs + 7)
    for fc in (0.0, 19.0, 260.0, 6500.0, 0.49 * fs + 1.0):
        for fb in (0.0, 0.85):
            fx = aug.Phaser(fs, rate_hz=5.5, depth=0.6, centre_frequency_hz=fc, feedback=fb, mix=0.7)
            check_fx(fx, x, what=("phaser", fs, fc, fb))


# ----------------------------------------------------------------------------- 5. guarded edge lengths, all three
def run_edge_lengths(r, n, shift=0, fs=48000):
    x = ke.signal(n, 900 + n, special=True)
    src = ke.dev(r, x)
    for D in sorted({0, 1, 2, max(n // 3, 1), n - 1, n}):
        out = ke.Guarded(r, n, shift=shift)
        call_delay(r, r.mem.ptr(src), out.ptr, n, D, 0.6, 0.5)
        check(out.get(), ref_delay(x, D, 0.6, 0.5), what=("delay", n, D))
    for fb in (0.0, 0.5):
        out = ke.Guarded(r, n, shift=shift)
        r.lib.call("al_fx_chorus", r.mem.ptr(src), out.ptr, n, float(fs), 6.0, 0.8, 1.5, fb, 0.5, r.mem.stream())
        check(out.get(), ref_chorus(x, fs, 6.0, 0.8, 1.5, fb, 0.5), what=("chorus", n, fb))
    out = ke.Guarded(r, n, shift=shift)
    r.lib.call("al_fx_phaser", r.mem.ptr(src), out.ptr, n, float(fs), 8.0, 0.9, 900.0, 0.8, 0.6, r.mem.stream())
    check(out.get(), ref_phaser(x, fs, 8.0, 0.9, 900.0, 0.8, 0.6), what=("phaser", n))


def run_chorus_case(r, n, fs, rate_hz, depth, centre_delay_ms, feedback, mix, shift=0):
    """al_fx_chorus with every parameter the caller's, into a guarded buffer, against the oracle; returns the device output."""
    x = ke.signal(n, 700 + n, special=True)
    src = ke.dev(r, x)
    out = ke.Guarded(r, n, shift=shift)
    r.lib.call("al_fx_chorus", r.mem.ptr(src), out.ptr, n, float(fs), rate_hz, depth, centre_delay_ms, feedback, mix, r.mem.stream())
    got = out.get()
    check(got, ref_chorus(x, fs, rate_hz, depth, centre_delay_ms, feedback, mix), what=("chorus", n, fs, feedback))
    return got


def run_phaser_case(r, n, fs, rate_hz, depth, centre_frequency_hz, feedback, mix, shift=0):
    """al_fx_phaser likewise."""
    x = ke.signal(n, 800 + n, special=True)
    src = ke.dev(r, x)
    out = ke.Guarded(r, n, shift=shift)
    r.lib.call("al_fx_phaser", r.mem.ptr(src), out.ptr, n, float(fs), rate_hz, depth, centre_frequency_hz, feedback, mix,
               r.mem.stream())
    got = out.get()
    check(got, ref_phaser(x, fs, rate_hz, depth, centre_frequency_hz, feedback, mix), what=("phaser", n, fs, feedback))
    return got


def run_long(r, kind, n, fs=48000, **kw):
    """One long clip through one entry point against the oracle (the lengths the profile is reported at)."""
    x = noise(n, 77)
    src = ke.dev(r, x)
    dst = r.mem.empty(n)
    if kind == "delay":
        call_delay(r, r.mem.ptr(src), r.mem.ptr(dst), n, kw["D"], kw["fb"], kw["mix"])
        want = ref_delay(x, kw["D"], float(np.float32(kw["fb"])), float(np.float32(kw["mix"])))
    elif kind == "chorus":
        r.lib.call("al_fx_chorus", r.mem.ptr(src), r.mem.ptr(dst), n, float(fs), 3.0, 0.7, 8.0, kw["fb"], 0.5, r.mem.stream())
        want = ref_chorus(x, fs, 3.0, 0.7, 8.0, kw["fb"], 0.5)
    else:
        r.lib.call("al_fx_phaser", r.mem.ptr(src), r.mem.ptr(dst), n, float(fs), 1.5, 0.8, 1200.0, 0.7, 0.5, r.mem.stream())
        want = ref_phaser(x, fs, 1.5, 0.8, 1200.0, 0.7, 0.5)
    r.mem.synchronize()
    got = np.asarray(r.mem.download(dst))[:n]
    check(got, want, what=(kind, n, kw))


# ----------------------------------------------------------------------------- 6. C ABI refusals
def run_abi_refusals(r):
    n = 256
    x = ke.dev(r, noise(n, 3))
    y = r.mem.empty(n)
    xp, yp = r.mem.ptr(x), r.mem.ptr(y)

    def refused(match, entry, *args):
        with pytest.raises(_hip.HipError, match=match):
            if entry == "al_fx_delay":
                src, dst, nn, D, fb, mix = args
                call_delay(r, src, dst, nn, D, fb, mix)
            else:
                r.lib.call(entry, *args, r.mem.stream())
        assert match in r.lib.last_error(), r.lib.last_error()
        assert entry in r.lib.last_error(), r.lib.last_error()

    # al_fx_delay
    refused("null pointer", "al_fx_delay", None, yp, n, 10, 0.5, 0.5)
    refused("null pointer", "al_fx_delay", xp, None, n, 10, 0.5, 0.5)
    refused("n must be >= 1", "al_fx_delay", xp, yp, 0, 10, 0.5, 0.5)
    refused("dst overlaps src", "al_fx_delay", xp, xp, n, 10, 0.5, 0.5)
    refused("dst overlaps src", "al_fx_delay", xp, xp + 4 * (n - 1), n, 10, 0.5, 0.5)
    refused("delay_samples must be >= 0", "al_fx_delay", xp, yp, n, -1, 0.5, 0.5)
    refused("feedback must be finite and >= 0", "al_fx_delay", xp, yp, n, 10, float("nan"), 0.5)
    refused("feedback must be finite and >= 0", "al_fx_delay", xp, yp, n, 10, -0.1, 0.5)
    refused("feedback must be < 1", "al_fx_delay", xp, yp, n, 10, 1.0, 0.5)
    refused("mix must be finite and >= 0", "al_fx_delay", xp, yp, n, 10, 0.5, float("inf"))
    refused("mix must be finite and >= 0", "al_fx_delay", xp, yp, n, 10, 0.5, -0.5)
    # al_fx_chorus and al_fx_phaser: fs, rate_hz, depth, centre, feedback, mix
    for entry, centre in (("al_fx_chorus", "centre_delay_ms"), ("al_fx_phaser", "centre_frequency_hz")):
        good = [48000.0, 2.0, 0.5, 7.0 if entry == "al_fx_chorus" else 1000.0, 0.5, 0.5]
        refused("null pointer", entry, None, yp, n, *good)
        refused("null pointer", entry, xp, None, n, *good)
        refused("n must be >= 1", entry, xp, yp, -3, *good)
        refused("dst overlaps src", entry, xp, xp + 8, n, *good)
        for i, name in enumerate(["fs", "rate_hz", "depth", centre, "feedback", "mix"]):
            for bad in (float("nan"), float("inf"), -1.0):
                args = list(good)
                args[i] = bad
                refused(f"{name} must be finite and >= 0", entry, xp, yp, n, *args)
        args = list(good)
        args[4] = 1.0
        refused("feedback must be < 1", entry, xp, yp, n, *args)
    refused("fs out of range", "al_fx_chorus", xp, yp, n, 999.0, 2.0, 0.5, 7.0, 0.5, 0.5)
    refused("fs out of range", "al_fx_chorus", xp, yp, n, 148000.0, 2.0, 0.5, 7.0, 0.5, 0.5)
    refused("fs out of range", "al_fx_phaser", xp, yp, n, 40.0, 2.0, 0.5, 1000.0, 0.5, 0.5)
    # accepted at the edges: adjacent buffers, the largest chorus rate, the smallest phaser rate, mix > 1
    big = r.mem.empty(2 * n)
    bp = r.mem.ptr(big)
    assert call_delay(r, bp, bp + 4 * n, n, 10, 0.5, 0.5) == 0
    assert r.lib.call("al_fx_chorus", xp, yp, n, 147000.0, 2.0, 0.5, 7.0, 0.5, 2.0, r.mem.stream()) == 0
    assert r.lib.call("al_fx_phaser", xp, yp, n, 41.0, 2.0, 0.5, 1000.0, 0.5, 2.0, r.mem.stream()) == 0
    r.mem.synchronize()


# ----------------------------------------------------------------------------- 7. the classes
KEYS = {aug.Delay: ["delay_seconds", "feedback", "mix"],
        aug.Chorus: ["rate_hz", "depth", "centre_delay_ms", "feedback", "mix"],
        aug.Phaser: ["rate_hz", "depth", "centre_frequency_hz", "feedback", "mix"]}


def run_class_api():
    assert all(c in aug.ALL_EVENT_AUGMENTATIONS for c in KEYS)
    assert (aug.Delay.MIN_DELAY, aug.Delay.MAX_DELAY, aug.Delay.MIN_FEEDBACK, aug.Delay.MAX_FEEDBACK, aug.Delay.MIN_MIX,
            aug.Delay.MAX_MIX) == (0.01, 1.0, 0.1, 0.5, 0.1, 0.5)
    for cls in (aug.Chorus, aug.Phaser):
        assert (cls.MIN_RATE, cls.MAX_RATE, cls.MIN_DEPTH, cls.MAX_DEPTH, cls.MIN_MIX, cls.MAX_MIX, cls.MIN_FEEDBACK,
                cls.MAX_FEEDBACK) == (0, 10, 0.0, 1.0, 0.1, 0.5, 0.0, 0.9)
    assert (aug.Chorus.MIN_DELAY, aug.Chorus.MAX_DELAY) == (1.0, 20.0)
    assert (aug.Phaser.MIN_FREQ, aug.Phaser.MAX_FREQ) == (260, 6500)
    ranges = {"delay_seconds": (0.01, 1.0), "rate_hz": (0, 10), "depth": (0.0, 1.0), "centre_delay_ms": (1.0, 20.0),
              "centre_frequency_hz": (260, 6500), "mix": (0.1, 0.5)}
    for cls, keys in KEYS.items():
        for seed in range(20):
            np.random.seed(seed)
            a = cls(44100)
            np.random.seed(seed)
            b = cls(44100)
            assert a == b and a.to_dict() == b.to_dict()
            assert list(a.params) == keys
            d = a.to_dict()
            assert d["name"] == cls.__name__ and d["sample_rate"] == 44100
            for key in keys:
                lo, hi = ranges.get(key, (cls.MIN_FEEDBACK, cls.MAX_FEEDBACK))
                assert lo <= d[key] <= hi, (cls, key, d[key])
                assert getattr(a, key) == d[key]
            again = aug.Augmentation.from_dict(json.loads(json.dumps(d)))
            assert type(again) is cls and again == a and again.to_dict() == d
        assert cls(44100).host_dtype(np.dtype(np.float64)) == np.float32
        with pytest.raises(ValueError, match="feedback"):
            cls(44100, feedback=1.0)
        with pytest.raises(ValueError, match="feedback"):
            cls(44100, feedback=1.5)
        with pytest.raises(ValueError, match="positive"):
            cls(44100, feedback=-0.1)
        with pytest.raises(ValueError, match="positive"):
            cls(44100, mix=-0.2)
        with pytest.raises(TypeError):
            cls(44100, mix="wet")
    # the reference's on-disk layout loads
    ref_dicts = [dict(name="Phaser", sample_rate=44100, rate_hz=1.25, depth=0.5, centre_frequency_hz=1300.0, feedback=0.0,
                      mix=0.5),
                 dict(name="Chorus", sample_rate=48000, rate_hz=1.0, depth=0.25, centre_delay_ms=7.0, feedback=0.0, mix=0.5),
                 dict(name="Delay", sample_rate=22050, delay_seconds=0.5, feedback=0.0, mix=0.5)]
    for d in ref_dicts:
        fx = aug.Augmentation.from_dict(d)
        assert type(fx).__name__ == d["name"] and fx.to_dict() == d
    assert aug.Delay(48000, delay_seconds=0.0123).delay_samples == int(0.0123 * 48000)


# ----------------------------------------------------------------------------- 8. a chain on an Event, and in a scene
def chain(sr):
    return [aug.Phaser(sr, rate_hz=1.5, depth=0.7, centre_frequency_hz=900.0, feedback=0.6, mix=0.5),
            aug.LowpassFilter(sr, cutoff_frequency_hz=2500.0),
            aug.Delay(sr, delay_seconds=0.0371, feedback=0.45, mix=0.4)]


def oracle_chain(raw, fxs):
    y = np.asarray(raw, dtype=np.float64)
    for fx in fxs:
        y = ref_fx(fx, y)
    return orc.peak_normalise_clip(y)


def run_event_chain(r, monkeypatch):
    sr = 16000
    rng = np.random.default_rng(5)
    raw = (rng.standard_normal(9000) * 0.4).astype(np.float32)
    fxs = chain(sr)

    def no_host_fx(self, *a, **k):
        raise AssertionError(f"{self.name} ran as a host FX call")

    monkeypatch.setattr(aug.Augmentation, "process", no_host_fx)    # the foreign-callables branch calls aug(out)
    ev = core.Event("dm", raw, sr, augmentations=fxs)
    got = ev.load_audio()
    want = oracle_chain(raw, fxs)
    check(got, want)
    assert_parity(got, want)
    # through a scene render: one upload (the staging arena), zero downloads
    C, L = 3, 500
    irs = (rng.standard_normal((C, 2, L)) * np.exp(-np.arange(L) / 100.0)).astype(np.float32)
    raws = [raw, (rng.standard_normal(7000) * 1.5).astype(np.float32)]
    chains = [chain(sr), [aug.Chorus(sr, rate_hz=2.0, depth=0.5, centre_delay_ms=6.0, feedback=0.5, mix=0.4), aug.Invert(sr)]]
    scene = core.Scene(1.5, core.StaticIRState({"mic000": irs}), sample_rate=sr, ref_db=-65)
    for i, (x, c) in enumerate(zip(raws, chains)):
        scene.add_event(core.Event(f"e{i}", x, sr, snr=8.0 + 3 * i, scene_start=0.2 * i, augmentations=c))
    scene.generate()
    spatials = []
    for i, ev in enumerate(scene.events.values()):
        want = orc.render_event(oracle_chain(raws[i], chains[i]), irs[:, [i], :].astype(np.float64), ev.snr, sr=sr)["spatial"]
        spatials.append(want)
        assert_parity(ev.spatial_audio["mic000"], want, what=ev.alias)
        clip = ev._last_chain
        assert clip.uploads == 1 and clip.downloads == 0
    ref = orc.mix_scene(spatials, [(e.scene_start, e.scene_end) for e in scene.events.values()], 1.5, sr, keep_padded=False)
    assert_parity(scene.audio["mic000"], ref["scene"])


# ----------------------------------------------------------------------------- 9. a reference scene JSON naming all three
def run_scene_json(tmp_path):
    here = os.path.join(os.path.dirname(__file__), "golden")
    z = np.load(os.path.join(here, "reference_scene_arrays.npz"))
    meta = json.load(open(os.path.join(here, "reference_scene.json")))
    sr = meta["sample_rate"]
    injected = {
        "event000": [dict(name="Delay", sample_rate=sr, delay_seconds=0.0625, feedback=0.35, mix=0.3),
                     dict(name="Chorus", sample_rate=sr, rate_hz=1.7, depth=0.6, centre_delay_ms=9.0, feedback=0.4, mix=0.45)],
        "event001": [dict(name="Phaser", sample_rate=sr, rate_hz=3.1, depth=0.9, centre_frequency_hz=2100.0, feedback=0.5,
                          mix=0.35)],
    }
    for alias, extra in injected.items():
        meta["events"][alias]["augmentations"] = meta["events"][alias]["augmentations"] + extra
    path = tmp_path / "scene_with_delay_mod.json"
    path.write_text(json.dumps(meta))
    clips = {a: z[f"clip_{a}"] for a in meta["events"]}
    irs = {m: z[f"irs_{m}"] for m in meta["state"]["microphones"]}
    scene = core.Scene.from_json(str(path), clips, irs)
    assert [type(a).__name__ for a in scene.events["event000"].augmentations][-2:] == ["Delay", "Chorus"]
    assert [type(a).__name__ for a in scene.events["event001"].augmentations][-1:] == ["Phaser"]
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
        # the reference's scene with the two plain contributions replaced by the oracle-processed ones
        swap = (orc.mix_scene(new, slots, meta["duration"], sr, keep_padded=False)["scene"].astype(np.float64)
                - orc.mix_scene(old, slots, meta["duration"], sr, keep_padded=False)["scene"])
        assert_parity(out[mic], z[f"scene_{mic}"].astype(np.float64) + swap, what=mic)
