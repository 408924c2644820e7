"""Scenarios of the device time-stretch FX (SpeedUp, PitchShift) and of their entry points ``al_fx_time_stretch`` and
``al_fx_resample_sinc``, shared by tests/test_hostemu_time_stretch_fx.py (host emulation) and tests/test_gpu_time_stretch_fx.py
(gfx950 build).  Every scenario takes the renderer ``r`` the package is set to.

The oracle is a plain float64 restatement, written HERE with numpy alone, of the definition in DESIGN.md "Time-stretch FX"
(librosa 0.11's ``effects.time_stretch`` / ``phase_vocoder`` restated, and a Kaiser-windowed sinc resampler; NOT checked against
a running librosa or pedalboard), vectorised over frames and bins, so the package is not checked against itself.

Bounds.  Noise of at most 1 s: the project's FX bound, 1e-5 on the relative RMS and on max-abs / peak (the definition run with
float32 transforms sits at 0.4e-6 .. 1.8e-6 of the float64 one).  Pure tones and the 10 s clip are conditioned differently:
near-empty bins carry arbitrary phases into the accumulator and the error grows with the frame count, so there the bound is
max(1e-5, 4 E32) on each figure, E32 being the oracle run with float32 ``rfft`` / ``irfft`` against the float64 oracle on the
same input (the factor 4: the device's Stockham transform is another float32 algorithm than pocketfft, its error of the same
order but not equal).

Not vacuous: every parity case asserts FROM THE ORACLE ALONE that the 2 pi wrap changes d in at least 5 % of the (t, k) entries,
that alpha_t is non-zero in at least half of the frames (counted over t >= 1: step_0 = 0 whatever the rate, and at rate 1.5, where
alpha alternates between 0 and 0.5, an odd frame count would otherwise fall one frame short of the half), and, for pitch-up
cases, that the resampler's c is below 0.95.
"""
import collections
import json
import os

import numpy as np
import pytest

from audiblelight_amd import _hip, augmentation as aug, core
from oracle import synth_oracle as orc
from tests import dynamics_fx_cases as dyn
from tests import kernel_edges as ke
from tests.conftest import assert_parity, parity_errors

TOL = 1e-5
N_FFT = 2048
PV_TILE = _hip.PV_TILE          # csrc/al_stretchfx.h PV_TILE = 32
assert PV_TILE == 32
MAX_GRID_ROWS = 32768           # csrc/al_stft.h
FLT_MIN = float(np.finfo(np.float32).tiny)
FS = (16000, 48000)
EDGE_N = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097)
EDGE_RATES = (0.25, 0.7, 1.0, 1.5, 4.0)
RESAMPLE_CASES = ((1, 1), (1, 7), (7, 1), (1000, 841), (841, 1000), (4097, 4096), (5000, 5000))
CLIP_10S = 10 * 48000


# ----------------------------------------------------------------------------- the oracle
def frames_in(n, n_fft):
    return 1 + n // (n_fft // 4)


def steps_of(F, rate):
    """step_t = t rate in float64 for every t >= 0 with step_t < F."""
    t = np.arange(int(np.ceil(F / rate)) + 2, dtype=np.float64)
    steps = t * np.float64(rate)
    return steps[steps < F]


def ref_stretch(x, rate, n_fft, n_out, float32_transforms=False, info=None):
    """stretch(x, rate, n_fft, n_out) of the definition.  ``float32_transforms``: rfft and irfft run in float32 (numpy keeps the
    precision of its input), everything else stays float64: the E32 run.  ``info``: a dict that receives F, T, the fraction of
    (t, k) entries the wrap changes and the fraction of the frames t >= 1 with alpha != 0 (step_0 = 0 whatever the rate)."""
    x = np.asarray(x, dtype=np.float64)
    n, hop, bins = len(x), n_fft // 4, n_fft // 2 + 1
    ft = np.float32 if float32_transforms else np.float64
    w = np.sin(np.pi * np.arange(n_fft) / n_fft) ** 2
    xpad = np.concatenate([np.zeros(n_fft // 2), x, np.zeros(n_fft // 2)])
    F = frames_in(n, n_fft)
    idx = np.arange(F)[:, None] * hop + np.arange(n_fft)[None, :]
    D = np.fft.rfft((w * xpad[idx]).astype(ft), axis=1)
    assert D.dtype == (np.complex64 if float32_transforms else np.complex128)
    D = np.concatenate([D.astype(np.complex128), np.zeros((2, bins), dtype=np.complex128)])
    steps = steps_of(F, rate)
    T = len(steps)
    i = np.floor(steps).astype(np.int64)
    alpha = steps - i
    mod, arg = np.abs(D), np.angle(D)           # np.angle(0) = 0
    mag = (1.0 - alpha)[:, None] * mod[i] + alpha[:, None] * mod[i + 1]
    phi = np.pi * hop * np.arange(bins) / (n_fft / 2)
    d0 = arg[i + 1] - arg[i] - phi
    turns = np.round(d0 / (2.0 * np.pi))
    inc = phi + (d0 - 2.0 * np.pi * turns)
    acc = arg[0] + np.concatenate([np.zeros((1, bins)), np.cumsum(inc[:-1], axis=0)])   # exclusive prefix sum over t
    S = mag * np.exp(1j * acc)
    fr = np.fft.irfft(S.astype(np.complex64) if float32_transforms else S, n=n_fft, axis=1)
    assert fr.dtype == ft
    wf = w * fr.astype(np.float64)
    y = np.zeros((T + 3, hop))
    ws = np.zeros((T + 3, hop))
    w2 = w ** 2
    for q in range(4):          # frame t covers rows t .. t + 3 of the (hop-wide) output
        y[q:q + T] += wf[:, q * hop:(q + 1) * hop]
        ws[q:q + T] += w2[q * hop:(q + 1) * hop]
    y, ws = y.reshape(-1), ws.reshape(-1)
    assert len(y) == n_fft + hop * (T - 1)
    big = ws > FLT_MIN
    y[big] /= ws[big]
    out = np.zeros(n_out)
    seg = y[n_fft // 2: n_fft // 2 + n_out]
    out[:len(seg)] = seg
    if info is not None:
        info.update(F=F, T=T, wrapped=float(np.mean(turns != 0)), alpha_nonzero=float(np.mean(alpha[1:] != 0)) if T > 1 else 0.0)
    return out


def resample_c(m, n):
    return 0.95 * min(1.0, n / m)


def ref_resample(y1, n):
    """y1 (m samples) resampled to n samples by the Kaiser-windowed sinc of the definition."""
    y1 = np.asarray(y1, dtype=np.float64)
    m = len(y1)
    c = resample_c(m, n)
    H, beta = 16.0 / c, 8.6
    K = int(H) + 2
    offs = np.arange(-K, K + 1, dtype=np.int64)
    out = np.zeros(n)
    for t0 in range(0, n, 4096):
        t = np.arange(t0, min(t0 + 4096, n), dtype=np.int64)
        i, rem = np.divmod(t * m, n)                    # p = i + rem / n, exact
        j = i[:, None] + offs[None, :]
        dlt = (i[:, None] - j).astype(np.float64) + (rem / n)[:, None]      # p - j
        valid = (j >= 0) & (j < m) & (np.abs(dlt) <= H)
        kern = c * np.sinc(c * dlt) * np.i0(beta * np.sqrt(np.clip(1.0 - (dlt / H) ** 2, 0.0, None))) / np.i0(beta)
        out[t0:t0 + len(t)] = np.sum(np.where(valid, y1[np.clip(j, 0, m - 1)] * kern, 0.0), axis=1)
    return out


def wrap_to(y, n):
    """The reference's pad_mode="wrap" / truncation back to n samples (al_wrap_copy: dst[i] = src[i mod len])."""
    return y[:n] if len(y) >= n else y[np.arange(n) % len(y)]


def speedup_n_out(n, factor):
    return max(1, int(round(n / factor)))


def pitch_geometry(n, semitones):
    r = 2.0 ** (-semitones / 12.0)
    return r, max(1, int(round(n / r)))


def ref_fx(fx, x, float32_transforms=False, info=None):
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    if isinstance(fx, aug.SpeedUp):
        if fx.stretch_factor == 1.0:
            return x
        return wrap_to(ref_stretch(x, fx.stretch_factor, N_FFT, speedup_n_out(n, fx.stretch_factor), float32_transforms, info), n)
    if isinstance(fx, aug.PitchShift):
        if fx.semitones == 0:
            return x
        r, m = pitch_geometry(n, fx.semitones)
        if info is not None:
            info["c"] = resample_c(m, n)
        return ref_resample(ref_stretch(x, r, N_FFT, m, float32_transforms, info), n)
    return dyn.ref_fx(fx, x)


def assert_exercised(info, what=None, pitch_up=False):
    assert info["wrapped"] >= 0.05, (what, info)
    assert info["alpha_nonzero"] >= 0.5, (what, info)
    if pitch_up:
        assert info["c"] < 0.95, (what, info)


def noise(n, seed, sigma=0.2):
    return (np.random.default_rng(seed).standard_normal(n) * sigma).astype(np.float32)


def check(got, want, what=None, tol=TOL):
    rms, mx = parity_errors(got, want)
    print(f"time-stretch {what}: rel rms {rms:.3g} max/peak {mx:.3g} (bound {tol:.3g})")
    assert rms <= tol and mx <= tol, (what, rms, mx, tol)
    return rms, mx


def check_fx(fx, x, what=None):
    info = {}
    want = ref_fx(fx, x, info=info)
    assert_exercised(info, what=(what, fx), pitch_up=isinstance(fx, aug.PitchShift) and fx.semitones > 0)
    got = fx(x)
    assert got.dtype == np.float32 and got.shape == x.shape
    check(got, want, what=(what, fx))
    return got


# ----------------------------------------------------------------------------- 1. both classes
def class_cases(fs):
    return [aug.SpeedUp(fs, stretch_factor=0.7), aug.SpeedUp(fs, stretch_factor=1.5), aug.SpeedUp(fs, stretch_factor=1.25),
            aug.PitchShift(fs, semitones=-3), aug.PitchShift(fs, semitones=3), aug.PitchShift(fs, semitones=1)]


def run_class_parity(fs, case):
    x = noise(fs // 2, fs)
    check_fx(class_cases(fs)[case], x, what=fs)


def run_defaults_drawn(fs, seeds=range(3)):
    x = noise(fs // 2, fs + 1)
    for seed in seeds:
        np.random.seed(seed)
        speed, pitch = aug.SpeedUp(fs), aug.PitchShift(fs)
        assert 0.7 <= speed.stretch_factor <= 1.5 and -3 <= pitch.semitones <= 3
        check_fx(speed, x, what=(fs, seed))
        if pitch.semitones != 0:
            check_fx(pitch, x, what=(fs, seed))
        else:
            ke.assert_bits_equal(pitch(x), x, (fs, seed))


# ----------------------------------------------------------------------------- 2. edge lengths through the C entry
def stretch(r, x, rate, n_fft, n_out, shift=0):
    """al_fx_time_stretch into a guarded output, with a guarded workspace of exactly the floats the library asks for."""
    n = len(x)
    floats = r.lib.call("al_fx_time_stretch_workspace_floats", n, float(rate), n_fft)
    assert floats > 0
    work = ke.workspace(r, floats)
    out = ke.Guarded(r, n_out, shift=shift)
    src = ke.dev(r, np.asarray(x, dtype=np.float32))
    r.lib.call("al_fx_time_stretch", r.mem.ptr(src), n, out.ptr, n_out, float(rate), n_fft, work.ptr, r.mem.stream())
    got = out.get()
    work.get()
    return got


def check_stretch(r, x, rate, n_fft, n_out, what, shift=0, tol=TOL):
    info = {}
    want = ref_stretch(x, rate, n_fft, n_out, info=info)
    got = stretch(r, x, rate, n_fft, n_out, shift=shift)
    peak = float(np.max(np.abs(want)))
    if peak == 0.0:
        ke.assert_bits_equal(got, np.zeros(n_out, dtype=np.float32), what)
    else:
        check(got, want, what=what, tol=tol)
    return info


def run_edge_lengths(r, n, n_fft=256):
    x = noise(n, 700 + n)
    for rate in EDGE_RATES:
        n_out = max(1, int(round(n / rate)))
        check_stretch(r, x, rate, n_fft, n_out, what=("edge", n, rate), shift=n % 2)
    # 300 samples longer than the stretch: the zero tail starts where the overlap-add ends
    n_out = max(1, int(round(n / 0.7)))
    check_stretch(r, x, 0.7, n_fft, n_out + 300, what=("edge, zero tail", n))
    tail = stretch(r, x, 0.7, n_fft, n_out + 300)
    T = len(steps_of(frames_in(n, n_fft), 0.7))
    written = n_fft + (n_fft // 4) * (T - 1) - n_fft // 2
    assert written < len(tail)
    ke.assert_bits_equal(tail[written:], np.zeros(len(tail) - written, dtype=np.float32), ("zero tail", n))
    # truncated to one sample: the first sample of the full-length output (checked above), bit for bit -- and against the oracle,
    # the error taken relative to the peak of the full-length oracle output (one sample has no peak of its own to speak of)
    one = stretch(r, x, 0.7, n_fft, 1)
    ke.assert_bits_equal(one, tail[:1], ("truncated to one sample", n))
    want = ref_stretch(x, 0.7, n_fft, n_out)
    assert abs(float(one[0]) - want[0]) <= TOL * np.max(np.abs(want)), (n, one[0], want[0])


def tile_edge_sizes(n_fft=256, rate=1.1):
    """(n, T) with T = PV_TILE - 1, PV_TILE, PV_TILE + 1, 2 PV_TILE + 1: the smallest n that gives each (a rate above 1 reaches
    every T: T = ceil(F / rate) grows by less than one per frame)."""
    hop, found = n_fft // 4, {}
    for F in range(1, 200):
        T = len(steps_of(F, rate))
        found.setdefault(T, (F - 1) * hop)
    wanted = (PV_TILE - 1, PV_TILE, PV_TILE + 1, 2 * PV_TILE + 1)
    assert all(T in found for T in wanted), found
    return [(max(found[T], 1), T) for T in wanted]


def run_tile_edges(r, n_fft=256, rate=1.1):
    for n, T in tile_edge_sizes(n_fft, rate):
        x = noise(n, 900 + T)
        info = check_stretch(r, x, rate, n_fft, max(1, int(round(n / rate))), what=("tile edge", n, T))
        assert info["T"] == T


# ----------------------------------------------------------------------------- 3. past one launch group
def run_past_one_group(r, n_fft=64, n=16 * 32768 + 5, rate=0.9):
    x = noise(n, 17)
    info = check_stretch(r, x, rate, n_fft, max(1, int(round(n / rate))), what=("past one launch group", n))
    assert info["F"] > MAX_GRID_ROWS and info["T"] > MAX_GRID_ROWS, info
    assert_exercised(info, what="past one launch group")


# ----------------------------------------------------------------------------- 4. the resampler alone
def resample(r, y1, n, shift=0):
    m = len(y1)
    src = ke.dev(r, np.asarray(y1, dtype=np.float32))
    out = ke.Guarded(r, n, shift=shift)
    r.lib.call("al_fx_resample_sinc", r.mem.ptr(src), m, out.ptr, n, r.mem.stream())
    return out.get()


def run_resampler(r, m, n):
    y1 = noise(m, 40 + m + n)
    want = ref_resample(y1, n)
    check(resample(r, y1, n, shift=(m + n) % 2), want, what=("resample", m, n))
    if m == n and m > 100:
        # not the identity: a low-pass at 0.95 of the band
        assert resample_c(m, n) == 0.95
        rms, _ = parity_errors(want, y1.astype(np.float64))
        assert rms > 0.05, rms
    if n < m:
        assert resample_c(m, n) < 0.95


# ----------------------------------------------------------------------------- 5. structure: where the spectral peak lands
def peak_hz(y, fs):
    """The spectral peak of the middle half of y, by parabolic interpolation of the Hann-windowed log spectrum, zero-padded."""
    mid = np.asarray(y, dtype=np.float64)[len(y) // 4: len(y) // 4 + len(y) // 2]
    size = 1 << 18
    spec = np.abs(np.fft.rfft(mid * np.hanning(len(mid)), size))
    k = int(np.argmax(spec))
    a, b, c = np.log(spec[k - 1: k + 2])
    return (k + 0.5 * (a - c) / (a - 2 * b + c)) * fs / size


def tone_bound(fx, x, what):
    """max(1e-5, 4 E32) on each figure, E32 from the oracle alone."""
    e32 = parity_errors(ref_fx(fx, x, float32_transforms=True), ref_fx(fx, x))
    print(f"time-stretch {what}: E32 rel rms {e32[0]:.3g} max/peak {e32[1]:.3g}")
    return max(TOL, 4 * e32[0]), max(TOL, 4 * e32[1])


def check_conditioned(got, want, bound, what):
    rms, mx = parity_errors(got, want)
    print(f"time-stretch {what}: rel rms {rms:.3g} (bound {bound[0]:.3g}) max/peak {mx:.3g} (bound {bound[1]:.3g})")
    assert rms <= bound[0] and mx <= bound[1], (what, rms, mx, bound)


def run_structure(fs=48000, hz=1500.0):
    n = fs // 4
    assert hz * N_FFT / fs == round(hz * N_FFT / fs)         # bin-centred
    x = (0.5 * np.sin(2 * np.pi * hz * np.arange(n) / fs)).astype(np.float32)
    cases = [(aug.PitchShift(fs, semitones=3), hz * 2 ** (3 / 12)), (aug.PitchShift(fs, semitones=-3), hz * 2 ** (-3 / 12)),
             (aug.SpeedUp(fs, stretch_factor=0.7), hz), (aug.SpeedUp(fs, stretch_factor=1.5), hz)]
    for fx, want_hz in cases:
        want = ref_fx(fx, x)
        assert abs(peak_hz(want, fs) - want_hz) <= 1.0, ("oracle", fx, peak_hz(want, fs), want_hz)       # the oracle first
        got = fx(x)
        assert abs(peak_hz(got, fs) - want_hz) <= 1.0, (fx, peak_hz(got, fs), want_hz)
        check_conditioned(got, want, tone_bound(fx, x, ("tone", fx)), ("tone", fx))


# ----------------------------------------------------------------------------- 6. silence, identity parameters
def counting(r, monkeypatch):
    calls = []
    real = r.lib.call

    def counted(name, *args):
        calls.append((name, args))
        return real(name, *args)

    monkeypatch.setattr(r.lib, "call", counted)
    return calls, real


def run_silence_and_identity(r, monkeypatch, fs=16000):
    zeros = np.zeros(3000, dtype=np.float32)
    for fx in (aug.SpeedUp(fs, stretch_factor=0.7), aug.SpeedUp(fs, stretch_factor=1.5), aug.PitchShift(fs, semitones=2),
               aug.PitchShift(fs, semitones=-2)):
        ke.assert_bits_equal(fx(zeros), zeros, ("silence", fx))
    x = noise(3000, 3)
    calls, real = counting(r, monkeypatch)
    for fx in (aug.SpeedUp(fs, stretch_factor=1.0), aug.SpeedUp(fs, stretch_factor=1), aug.PitchShift(fs, semitones=0),
               aug.PitchShift(fs, semitones=0.9)):
        got = fx(x)
        assert got is x                                     # the reference's ``process`` returns its input
        clip = aug.DeviceClip(r, x)
        fx.process_device(clip)                             # and in a chain: nothing launched
        ke.assert_bits_equal(clip.host(), x, ("identity", fx))
    monkeypatch.setattr(r.lib, "call", real)
    assert calls == [], calls


# ----------------------------------------------------------------------------- 7. C ABI refusals
def run_abi_refusals(r):
    n, n_fft = 1000, 256
    x = ke.dev(r, noise(2 * n, 3))
    poison = np.full(n, 0.625, dtype=np.float32)
    out = ke.Guarded(r, n, init=poison)
    work = r.mem.empty(r.lib.call("al_fx_time_stretch_workspace_floats", n, 1.0, n_fft))
    xp, yp, wp, st = r.mem.ptr(x), out.ptr, r.mem.ptr(work), r.mem.stream()
    nan, inf = float("nan"), float("inf")

    def refused(match, entry, *args):
        with pytest.raises(_hip.HipError, match=match):
            r.lib.call(entry, *args, st)
        err = r.lib.last_error()
        assert entry in err, err

    ts, rs = "al_fx_time_stretch", "al_fx_resample_sinc"
    good = (xp, n, yp, n, 1.0, n_fft, wp)
    refused("null pointer", ts, None, n, yp, n, 1.0, n_fft, wp)
    refused("null pointer", ts, xp, n, None, n, 1.0, n_fft, wp)
    refused("null pointer", ts, xp, n, yp, n, 1.0, n_fft, None)
    for bad in (0, -3):
        refused("n must be >= 1", ts, xp, bad, yp, n, 1.0, n_fft, wp)
        refused("n_out must be >= 1", ts, xp, n, yp, bad, 1.0, n_fft, wp)
    refused("dst overlaps src", ts, xp, n, xp, n, 1.0, n_fft, wp)
    refused("dst overlaps src", ts, xp, n, xp + 4 * (n - 1), n, 1.0, n_fft, wp)
    refused("dst overlaps src", ts, xp + 4 * 10, n, xp, 11, 1.0, n_fft, wp)        # the ranges have their own lengths
    for bad in (0, 32, 63, 96, 255, 8192, -256):
        refused(r"n_fft must be a power of two in \[64, 4096\]", ts, xp, n, yp, n, 1.0, bad, wp)
    for bad in (nan, inf, -inf, 0.0, -1.0, 0.2499, 4.0001):
        refused(r"rate must be finite and in \[0.25, 4\]", ts, xp, n, yp, n, bad, n_fft, wp)
    # F or T past the frame indexing (2^30): refused before anything is read
    refused("too many analysis frames", ts, xp, (1 << 30) * 16, yp, n, 1.0, 64, wp)
    refused("too many output frames", ts, xp, (1 << 29) * 16, yp, n, 0.25, 64, wp)
    assert r.lib.call("al_fx_time_stretch_workspace_floats", (1 << 30) * 16, 1.0, 64) == 0
    assert r.lib.call("al_fx_time_stretch_workspace_floats", n, 5.0, n_fft) == 0
    assert r.lib.call("al_fx_time_stretch_workspace_floats", n, 1.0, 100) == 0
    assert r.lib.call("al_fx_time_stretch_workspace_floats", 0, 1.0, n_fft) == 0
    refused("null pointer", rs, None, n, yp, n)
    refused("null pointer", rs, xp, n, None, n)
    for bad in (0, -1):
        refused("m must be >= 1", rs, xp, bad, yp, n)
        refused("n must be >= 1", rs, xp, n, yp, bad)
    refused("dst overlaps src", rs, xp, n, xp, n)
    refused("dst overlaps src", rs, xp, n, xp + 4 * (n - 1), 5)
    r.mem.synchronize()
    ke.assert_bits_equal(out.get(), poison, "a refused call wrote")
    # accepted at the edges: both ends of the rate and n_fft ranges, adjacent buffers
    for rate, fft in ((0.25, n_fft), (4.0, n_fft), (1.0, 64), (1.0, 4096)):
        w = r.mem.empty(r.lib.call("al_fx_time_stretch_workspace_floats", n, rate, fft))
        assert r.lib.call(ts, xp, n, yp, n, rate, fft, r.mem.ptr(w), st) == 0
    big = r.mem.empty(2 * n)
    big[:] = 0.25
    bp = r.mem.ptr(big)
    assert r.lib.call(ts, bp, n, bp + 4 * n, n, *good[4:], st) == 0
    assert r.lib.call(rs, bp, n, bp + 4 * n, n, st) == 0
    r.mem.synchronize()
    out.get()


# ----------------------------------------------------------------------------- 8. the classes
def run_class_api():
    S, P = aug.SpeedUp, aug.PitchShift
    assert S in aug.ALL_EVENT_AUGMENTATIONS and P in aug.ALL_EVENT_AUGMENTATIONS and len(aug.ALL_EVENT_AUGMENTATIONS) == 25
    assert (S.MIN_SHIFT, S.MAX_SHIFT) == (0.7, 1.5) and (P.MIN_SEMITONES, P.MAX_SEMITONES) == (-3, 3)
    for cls, key in ((S, "stretch_factor"), (P, "semitones")):
        for seed in range(20):
            np.random.seed(seed)
            a = cls(44100)
            np.random.seed(seed)
            b = cls(44100)
            assert a == b and a.to_dict() == b.to_dict()
            assert list(a.params) == [key]
            d = a.to_dict()
            assert d["name"] == cls.__name__ and d["sample_rate"] == 44100 and getattr(a, key) == d[key]
            again = aug.Augmentation.from_dict(json.loads(json.dumps(d)))
            assert type(again) is cls and again == a and again.to_dict() == d
        assert cls(44100).host_dtype(np.dtype(np.float64)) == np.float32
        assert cls(44100).batch_job(None) is None
    # the draws: one uniform each, over the reference's ranges
    np.random.seed(7)
    want = (float(np.random.uniform(0.7, 1.5)), int(np.random.uniform(-3, 3)))
    np.random.seed(7)
    assert (S(48000).stretch_factor, P(48000).semitones) == want
    assert isinstance(P(48000).semitones, int)
    assert P(44100, semitones=2.9).semitones == 2 and P(44100, semitones=-2.9).semitones == -2
    with pytest.raises(ValueError, match="positive"):
        S(44100, stretch_factor=-1.2)
    with pytest.raises(TypeError):
        S(44100, stretch_factor="fast")
    for bad in (0.0, 0.2, 4.5):
        with pytest.raises(ValueError, match="stretch factor"):
            S(44100, stretch_factor=bad)
    for bad in (25, -25, 100.0):
        with pytest.raises(ValueError, match="semitones"):
            P(44100, semitones=bad)
    assert S(44100, stretch_factor=0.25).stretch_factor == 0.25 and S(44100, stretch_factor=4).stretch_factor == 4.0
    assert P(44100, semitones=24).semitones == 24 and P(44100, semitones=-24).semitones == -24
    # the reference's on-disk layout loads
    for d in (dict(name="SpeedUp", sample_rate=44100, stretch_factor=1.2), dict(name="PitchShift", sample_rate=48000, semitones=-2)):
        fx = aug.Augmentation.from_dict(d)
        assert type(fx).__name__ == d["name"] and fx.to_dict() == d


# ----------------------------------------------------------------------------- 9. a chain on an Event, and in a scene
def chains(sr):
    return [[aug.SpeedUp(sr, stretch_factor=1.25), aug.LowpassFilter(sr, cutoff_frequency_hz=2500.0), aug.PitchShift(sr, semitones=2)],
            [aug.PitchShift(sr, semitones=-3), aug.Invert(sr)]]


def oracle_chain(raw, fxs):
    y = np.asarray(raw, dtype=np.float64)
    for fx in fxs:
        y = ref_fx(fx, y)
    return orc.peak_normalise_clip(y)


def run_event_chain(r, monkeypatch):
    sr = 16000
    raws = [noise(9000, 31), noise(7000, 32, sigma=0.3)]
    fxs = chains(sr)

    def no_host_fx(self, *a, **k):
        raise AssertionError(f"{self.name} ran as a host FX call")

    for cls in (aug.Augmentation, aug._TimeStretchFX):
        monkeypatch.setattr(cls, "process", no_host_fx)     # the foreign-callables branch calls aug(out)
    for raw, chain in zip(raws, fxs):
        got = core.Event("stretch", raw, sr, augmentations=chain).load_audio()
        want = oracle_chain(raw, chain)
        check(got, want, what="load_audio")
        assert_parity(got, want)
    # through a scene render: one upload (the staging arena), zero downloads, every time-stretch FX run in place in chain order
    C, L = 3, 500
    rng = np.random.default_rng(5)
    irs = (rng.standard_normal((C, 2, L)) * np.exp(-np.arange(L) / 100.0)).astype(np.float32)
    scene = core.Scene(1.5, core.StaticIRState({"mic000": irs}), sample_rate=sr, ref_db=-65)
    for i, (x, c) in enumerate(zip(raws, fxs)):
        scene.add_event(core.Event(f"e{i}", x, sr, snr=8.0 + 3 * i, scene_start=0.2 * i, augmentations=c))
    calls, real = counting(r, monkeypatch)
    scene.generate()
    monkeypatch.setattr(r.lib, "call", real)
    names = collections.Counter(name for name, _ in calls)
    assert names["al_fx_time_stretch"] == 3 and names["al_fx_resample_sinc"] == 2, names
    launches = collections.Counter((args[0], args[2]) for name, args in calls if name == "al_fx_batch_launch")
    assert launches == {(_hip.FXB_SOS, 1): 1}, launches      # the low-pass between them is still a batched job
    spatials = []
    for i, ev in enumerate(scene.events.values()):
        want = orc.render_event(oracle_chain(raws[i], fxs[i]), irs[:, [i], :].astype(np.float64), ev.snr, sr=sr)["spatial"]
        spatials.append(want)
        assert_parity(ev.spatial_audio["mic000"], want, what=ev.alias)
        clip = ev._last_chain
        assert clip.uploads == 1 and clip.downloads == 0
    ref = orc.mix_scene(spatials, [(e.scene_start, e.scene_end) for e in scene.events.values()], 1.5, sr, keep_padded=False)
    assert_parity(scene.audio["mic000"], ref["scene"])


# ----------------------------------------------------------------------------- 10. a reference scene JSON naming both
def run_scene_json(tmp_path):
    here = os.path.join(os.path.dirname(__file__), "golden")
    z = np.load(os.path.join(here, "reference_scene_arrays.npz"))
    meta = json.load(open(os.path.join(here, "reference_scene.json")))
    sr = meta["sample_rate"]
    injected = {
        "event000": [dict(name="SpeedUp", sample_rate=sr, stretch_factor=1.2)],
        "event001": [dict(name="PitchShift", sample_rate=sr, semitones=-2)],
    }
    for alias, extra in injected.items():
        meta["events"][alias]["augmentations"] = meta["events"][alias]["augmentations"] + extra
    path = tmp_path / "scene_with_time_stretch.json"
    path.write_text(json.dumps(meta))
    clips = {a: z[f"clip_{a}"] for a in meta["events"]}
    irs = {m: z[f"irs_{m}"] for m in meta["state"]["microphones"]}
    scene = core.Scene.from_json(str(path), clips, irs)
    assert type(scene.events["event000"].augmentations[-1]).__name__ == "SpeedUp"
    assert type(scene.events["event001"].augmentations[-1]).__name__ == "PitchShift"
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


# ----------------------------------------------------------------------------- 11. one long clip
def run_long(r, n=CLIP_10S, rate=0.7, n_fft=N_FFT):
    x = noise(n, 77)
    n_out = max(1, int(round(n / rate)))
    info = {}
    want = ref_stretch(x, rate, n_fft, n_out, info=info)
    assert_exercised(info, what="long")
    e32 = parity_errors(ref_stretch(x, rate, n_fft, n_out, float32_transforms=True), want)
    print(f"time-stretch long: E32 rel rms {e32[0]:.3g} max/peak {e32[1]:.3g}")
    src = ke.dev(r, x)
    dst = r.mem.empty(n_out)
    work = r.mem.empty(r.lib.call("al_fx_time_stretch_workspace_floats", n, rate, n_fft))
    r.lib.call("al_fx_time_stretch", r.mem.ptr(src), n, r.mem.ptr(dst), n_out, rate, n_fft, r.mem.ptr(work), r.mem.stream())
    r.mem.synchronize()
    got = np.asarray(r.mem.download(dst))[:n_out]
    check_conditioned(got, want, (max(TOL, 4 * e32[0]), max(TOL, 4 * e32[1])), ("long", n, rate))
