"""Edge-shape scenarios for the standalone kernels of the C ABI (everything a scene passes through after the accumulate stage,
plus ingest and encode), each called directly through ``r.lib.call`` and compared with an independent float64 restatement.
Shared by tests/test_hostemu_kernel_edges.py (host emulation) and tests/test_gpu_kernel_edges.py (gfx950 build).

Every output is written into a guarded buffer: G elements of a sentinel bit pattern before and after it, checked after the
call, so a store past either end is seen.  Where the ABI does not demand 16-byte alignment the interior pointer is also run one
element off alignment.  The workspaces of al_noise_irfft, al_stft and al_istft_ola are guarded buffers too, of exactly the
number of floats the matching al_*_workspace_floats call returns: a formula that comes up short is a guard violation.

Bounds (eps = float32 machine epsilon 2^-23, u = eps / 2 the unit roundoff):
  data movement (reverse, invert, clip, bitcrush, wrap copy, frame shuffle, packs, encode)   bit-exact
  one correctly rounded float32 operation (gain, scale, axpy)                                  exact / <= 0.5 ulp
  scans, reductions, FFTs                                                                      max-abs relative to the peak,
                                                                                               derived at each check
"""
import ctypes as ct

import numpy as np
from scipy import fft as sp_fft

from audiblelight_amd import _hip
from oracle import synth_oracle as orc
from tests.conftest import assert_parity, pcm16

EPS = float(np.finfo(np.float32).eps)      # 2^-23
U = EPS / 2                                # unit roundoff of float32
TINY32 = float(np.finfo(np.float32).tiny)
FLT_MAX = float(np.finfo(np.float32).max)
G = 64                                     # guard elements on each side of every output
SENTINEL = np.array([0xAD, 0xDE, 0xC0, 0x7F], dtype=np.uint8)   # float32 0x7FC0DEAD: a NaN payload no kernel writes

GRID_CAP = 4096 * 256 + 1        # first sample of the second grid-stride trip of the 4096-block launches
GRID_CAP_ROWS = 2048 * 256 + 1   # the same for al_axpy_rows / al_scale_matrix_rows (2048 blocks per row)
GRID_CAP_FLAT = 8192 * 256 + 1   # the same for al_scale_rows / al_scale_rows_f64 (8192 blocks)
CLIP_60S = 60 * 48000            # a 60 s clip at 48 kHz
EDGE_N = (2, 255, 256, 257, 1023, 1024, 1025)


# ----------------------------------------------------------------------------- guarded buffers
def sentinel_bytes(n):
    """n bytes of the repeated sentinel (np.resize(SENTINEL, n), which takes seconds at the tens of megabytes of a long fill)."""
    return np.tile(SENTINEL, (n + 3) // 4)[:n]


class Guarded:
    """A device buffer of n elements of `dtype` with ``guard`` (G unless given) sentinel elements on each side; ``shift`` moves
    the interior that many elements off the (at least 16-byte aligned) position it would have.  ``init`` fills the interior."""

    def __init__(self, r, n, dtype=np.float32, shift=0, init=None, guard=G):
        self.r, self.n, self.dtype = r, int(n), np.dtype(dtype)
        item = self.dtype.itemsize
        self.lo = (guard + shift) * item
        self.hi = self.lo + self.n * item
        total = (self.hi + guard * item + 3) // 4 * 4
        host = sentinel_bytes(total)
        if init is not None:
            host[self.lo:self.hi] = np.ascontiguousarray(init, dtype=self.dtype).reshape(-1).view(np.uint8)
        self.buf = r.mem.upload(host)
        self.ptr = r.mem.ptr(self.buf) + self.lo
        assert shift != 0 or self.ptr % 16 == 0, "guarded interior lost its 16-byte alignment"

    def get(self):
        """The interior, after asserting both guard bands still hold the sentinel."""
        self.r.mem.synchronize()
        raw = np.asarray(self.r.mem.download(self.buf)).view(np.uint8)
        pattern = sentinel_bytes(len(raw))
        bad = np.flatnonzero(np.concatenate([raw[:self.lo] != pattern[:self.lo], raw[self.hi:] != pattern[self.hi:]]))
        assert bad.size == 0, f"{bad.size} guard bytes overwritten (first at byte {int(bad[0])} of the guards)"
        return raw[self.lo:self.hi].view(self.dtype).copy()


def workspace(r, n_floats):
    """A transform workspace of exactly n_floats floats (what an al_*_workspace_floats call returned), its guard bands as long
    as the workspace itself (at most 2^20 floats): a formula that comes up a whole buffer short then still writes into the band,
    where it is seen, and not into whatever lies behind.  The interior starts as the sentinel NaN, like uninitialised memory."""
    n_floats = int(n_floats)
    assert n_floats > 0
    return Guarded(r, n_floats, guard=max(G, (min(n_floats, 1 << 20) + 3) // 4 * 4))


def dev(r, arr):
    return r.mem.upload(np.ascontiguousarray(arr))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 2: np.uint16, 8: np.uint64}[a.dtype.itemsize])


def assert_bits_equal(got, want, what=None):
    """Bit-exact: sign of zero and NaN payloads included."""
    want = np.ascontiguousarray(want, dtype=got.dtype)
    assert got.shape == want.shape, (got.shape, want.shape, what)
    diff = np.flatnonzero(bits(got) != bits(want))
    assert diff.size == 0, (what, f"{diff.size} elements differ, first at {int(diff[0])}: {got.flat[diff[0]]!r} vs {want.flat[diff[0]]!r}")


def ulps(got, ref):
    """|got - ref| in units of the float32 spacing at |ref| (ref in float64)."""
    ref = np.asarray(ref, dtype=np.float64)
    spacing = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - ref) / spacing


def peak_error(got, ref):
    """max|got - ref| / max|ref| (complex arrays: moduli)."""
    ref = np.asarray(ref, dtype=np.complex128 if np.iscomplexobj(ref) else np.float64)
    peak = float(np.max(np.abs(ref)))
    return float(np.max(np.abs(np.asarray(got, dtype=ref.dtype) - ref))) / (peak if peak > 0 else 1.0)


MARGINS = {}


def record(family, observed, bound):
    """Worst observed error / bound per family (test_*_kernel_edges.py print them at the end of the module)."""
    assert observed <= bound, (family, observed, bound)
    seen = MARGINS.setdefault(family, [0.0, bound])
    if observed / bound >= seen[0] / seen[1]:
        MARGINS[family] = [observed, bound]


def signal(n, seed, special=True):
    """Uniform noise in (-1, 1) with the awkward values planted from index 2 on, around the midpoint and at the end: +-0,
    denormals, the smallest normal, values just below 1.  x[0] and x[1] stay random: the emphasis filters' extrapolation
    term ((2 - c) x0 - x1) / (3 - c) must not vanish."""
    x = np.random.default_rng(seed).uniform(-1, 1, n).astype(np.float32)
    if special and n >= 16:
        vals = np.array([0.0, -0.0, 1e-40, -1e-40, TINY32, -TINY32, np.nextafter(np.float32(1), np.float32(0)), -1.0],
                        dtype=np.float32)
        x[2:10] = vals
        x[n // 2 - 4:n // 2 + 4] = vals[::-1]
        x[-8:] = vals
    return x


def fx(r, op, src, dst, n, p0=0.0, iparams=None):
    pa = (ct.c_float * 1)(p0)
    ip = (ct.c_int32 * 4)(*iparams) if iparams is not None else None
    r.lib.call("al_fx_apply", op, src, dst, n, ct.cast(pa, ct.c_void_p), ct.cast(ip, ct.c_void_p) if ip is not None else None,
               r.mem.stream())


# ----------------------------------------------------------------------------- al_fx_apply: pointwise ops
def run_fx_pointwise(r, n, shift=0, seed=0):
    """Every k_fx_pointwise op at length n, out of place into a guarded buffer, and in place for the in-place ops."""
    x = signal(n, seed)
    x64 = x.astype(np.float64)
    src = dev(r, x)
    p_gain = float(np.float32(10 ** (5.3 / 20)))
    p_clip = float(np.float32(10 ** (-3.0 / 20)))
    p_drive = float(np.float32(10 ** (17.0 / 20)))
    cases = [  # (op, p0, float64 reference, bound kind)
        (_hip.FX_GAIN, p_gain, x64 * p_gain, "exact"),          # one product of two float32: its float64 value is exact
        (_hip.FX_INVERT, 0.0, -x, "bits"),
        (_hip.FX_REVERSE, 0.0, x[::-1], "bits"),
        (_hip.FX_CLIP, p_clip, np.clip(x, -np.float32(p_clip), np.float32(p_clip)), "bits"),
        (_hip.FX_BITCRUSH, 2.0 ** 8, np.rint(x64 * 256.0) / 256.0, "exact"),   # power-of-two scale: every step is exact
        (_hip.FX_TANH, p_drive, np.tanh(np.float64(p_drive) * x64), "tanh"),
    ]
    for op, p0, ref, kind in cases:
        out = Guarded(r, n, shift=shift)
        fx(r, op, r.mem.ptr(src), out.ptr, n, p0)
        got = out.get()
        if kind == "bits":
            assert_bits_equal(got, ref, (op, n))
        elif kind == "exact":
            np.testing.assert_array_equal(got, np.asarray(ref).astype(np.float32), err_msg=str((op, n)))
        else:
            # tanhf(p * x): the float32 product is within u of p*x and tanh's relative condition number is <= 1, so the
            # argument costs 0.5 ulp; the device library's tanhf is allowed 2 ulp; the result's own rounding 0.5 ulp
            record("fx_tanh (ulp)", float(ulps(got, ref).max()), 3.0)
        if op in (_hip.FX_GAIN, _hip.FX_INVERT, _hip.FX_CLIP, _hip.FX_BITCRUSH, _hip.FX_TANH):   # in place: the same bits
            inplace = Guarded(r, n, shift=shift, init=x)
            fx(r, op, inplace.ptr, inplace.ptr, n, p0)
            assert_bits_equal(inplace.get(), got, ("in place", op, n))
    # the three out-of-place ops refuse src == dst
    for op in (_hip.FX_REVERSE, _hip.FX_PREEMPH, _hip.FX_DEEMPH):
        try:
            fx(r, op, r.mem.ptr(src), r.mem.ptr(src), n, 0.5)
        except _hip.HipError as exc:
            assert "dst != src" in str(exc)
        else:
            raise AssertionError(f"fx op {op} accepted src == dst")


def run_fx_preemphasis(r, n, coef, shift=0, seed=1):
    """y[t] = x[t] - c x[t-1], y[0] = x[0] + (2 x[0] - x[1]) (librosa's zi).  Each output is a sum of at most three terms
    with at most two roundings, so |err| <= 2u * (sum of the terms' magnitudes) = eps * S per element."""
    x = signal(n, seed)
    c = float(np.float32(coef))
    out = Guarded(r, n, shift=shift)
    src = dev(r, x)
    fx(r, _hip.FX_PREEMPH, r.mem.ptr(src), out.ptr, n, c)
    got = out.get().astype(np.float64)
    ref = orc.fx_preemphasis(x, c)
    x64 = x.astype(np.float64)
    S = np.abs(x64).copy()
    S[1:] += abs(c) * np.abs(x64[:-1])
    S[0] = 3 * abs(x64[0]) + abs(x64[1])
    err = np.abs(got - ref)
    record("fx_preemphasis (err / (eps*S))", float(np.max(err / (EPS * np.maximum(S, TINY32)))), 1.0)


def run_fx_deemphasis(r, n, coef, shift=0, seed=2):
    """y = IIR 1/(1 - c z^-1) from zero state minus the extrapolation term ((2-c) x0 - x1)/(3-c) * c^t.

    Bound: each step of the float32 recursion y = fma(c, y, x) adds at most u|y|, and an error entering at step k is carried
    on with weight c^(t-k), so the scan itself is off by at most u * max|y| / (1 - c).  The run-carry fold multiplies by
    powers c^k built by repeated products (relative error k*u) and k*u*c^k <= u / (e (1 - c)); the correction term's
    powf(c, lo) and running product the same again.  Together: |err| <= 4u * max|y| / (1 - c) = 2 eps max|y| / (1 - c).
    The reference runs with the float32 coefficient the kernel receives.  x0 and x1 are set so that the extrapolation term
    is as large as the signal: every run's powf(c, lo) and running power c^t are then measured, not multiplied by zero."""
    x = signal(n, seed)
    x[:2] = (0.875, -0.625)
    c = float(np.float32(coef))
    out = Guarded(r, n, shift=shift)
    src = dev(r, x)
    fx(r, _hip.FX_DEEMPH, r.mem.ptr(src), out.ptr, n, c)
    got = out.get()
    ref = orc.fx_deemphasis(x, c)
    record("fx_deemphasis (err/peak * (1-c) / eps)", peak_error(got, ref) * (1 - c) / EPS, 2.0)
    if c <= 0.999:
        assert_parity(got, ref, what=("deemphasis", n, coef))
    return got


def run_fx_fade(r, n, n_in, n_out, shape_in, shape_out, shift=0, seed=3):
    """x * fade_in(t) * fade_out(t) with the reference's curves on np.linspace(0, 1, len) (augmentation.py:1490-1554).

    Bound per element, relative to |x|: the ramp r = t / (len-1) is rounded (|dr| <= u r), the steepest curve (logarithmic
    fade-out near r = 1, slope 1/(0.1 ln 10) = 4.4) turns that into 2.2u; log10f(0.1 + r) sees the rounding of 0.1 + r
    amplified by 1.1 / (0.1 ln 10) = 4.8, i.e. 2.4u; the device's exp2f / log10f / sinpif are allowed 2 ulp; the clamp,
    the product of the two gains and the product with x one rounding each.  About 12u; asserted: 8 eps = 16u."""
    x = signal(n, seed)
    names = {v: k for k, v in _hip.FADE_SHAPES.items()}
    out = Guarded(r, n, shift=shift)
    src = dev(r, x)
    fx(r, _hip.FX_FADE, r.mem.ptr(src), out.ptr, n, 0.0, [n_in, n_out, shape_in, shape_out])
    got = out.get().astype(np.float64)
    env = orc.fade_envelope(n, 1, n_in, n_out, names[shape_in], names[shape_out])
    ref = x.astype(np.float64) * env
    scale = np.maximum(np.abs(x.astype(np.float64)), TINY32)
    record("fx_fade (err / (eps |x|))", float(np.max(np.abs(got - ref) / scale)) / EPS, 8.0)


# ----------------------------------------------------------------------------- al_fx_frame_shuffle, al_wrap_copy
def run_frame_shuffle(r, n, frame_len, row_len, n_rows, shift=0, seed=4):
    rng = np.random.default_rng(seed)
    m = frame_len * row_len
    x = signal(m, seed)
    rows = np.stack([rng.integers(0, frame_len, n_rows), rng.integers(0, 3, n_rows)], axis=1).astype(np.int32)
    rows[0] = (frame_len - 1, 2)   # the last source row, reversed
    out = Guarded(r, n, shift=shift)
    src, d_rows = dev(r, x), dev(r, rows.reshape(-1))
    r.lib.call("al_fx_frame_shuffle", r.mem.ptr(src), out.ptr, n, frame_len, row_len, r.mem.ptr(d_rows), n_rows, r.mem.stream())
    pieces = []
    for q in range(n_rows):
        row = x[rows[q, 0] + frame_len * np.arange(row_len)]
        pieces.append(np.zeros(row_len, np.float32) if rows[q, 1] == 1 else row[::-1] if rows[q, 1] == 2 else row)
    cat = np.concatenate(pieces)
    assert_bits_equal(out.get(), np.resize(cat, n), ("frame_shuffle", n))


def run_wrap_copy(r, m, n, shift=0, seed=5, guarded=None):
    """``guarded``: another guarded-buffer class for the destination (tests/transfer_cases.py: page-locked host memory)."""
    x = signal(m, seed)
    out = (guarded or Guarded)(r, n, shift=shift)
    src = dev(r, x)
    r.lib.call("al_wrap_copy", r.mem.ptr(src), m, out.ptr, n, r.mem.stream())
    assert_bits_equal(out.get(), np.resize(x, n), ("wrap_copy", m, n))


# ----------------------------------------------------------------------------- row-wise scalings
def run_row_scalings(r, rows, cols, shift=0, seed=6):
    """al_axpy_rows (one fma: correctly rounded), al_scale_matrix_rows, al_scale_rows and al_scale_rows_f64 (one product:
    exact in float64, so the float32 result must equal its rounding)."""
    rng = np.random.default_rng(seed)
    x = np.stack([signal(cols, seed + i) for i in range(rows)]).astype(np.float32)
    y = rng.uniform(-1, 1, (rows, cols)).astype(np.float32)
    a = rng.uniform(-2, 2, rows).astype(np.float32)
    out = Guarded(r, rows * cols, shift=shift, init=y)
    d_x, d_a = dev(r, x.reshape(-1)), dev(r, a)
    r.lib.call("al_axpy_rows", out.ptr, r.mem.ptr(d_x), r.mem.ptr(d_a), rows, cols, r.mem.stream())
    ref = a[:, None].astype(np.float64) * x + y.astype(np.float64)
    record("axpy_rows (ulp)", float(ulps(out.get(), ref.reshape(-1)).max()), 0.5 + 1e-6)   # 1e-6: the float64 sum's own rounding

    out = Guarded(r, rows * cols, shift=shift, init=x)
    r.lib.call("al_scale_matrix_rows", out.ptr, rows, cols, r.mem.ptr(d_a), r.mem.stream())
    np.testing.assert_array_equal(out.get(), (a[:, None].astype(np.float64) * x).astype(np.float32).reshape(-1))

    s64 = np.array([-0.7315926535897932], dtype=np.float64)
    out = Guarded(r, rows * cols, shift=shift, init=x)
    d_s = dev(r, s64)
    r.lib.call("al_scale_rows_f64", out.ptr, rows * cols, r.mem.ptr(d_s), r.mem.stream())
    s32 = np.float64(np.float32(s64[0]))
    np.testing.assert_array_equal(out.get(), (s32 * x.astype(np.float64)).astype(np.float32).reshape(-1))

    out = Guarded(r, rows * cols, shift=shift, init=x)
    d_s32 = dev(r, np.array([s32], np.float32))
    r.lib.call("al_scale_rows", out.ptr, rows * cols, r.mem.ptr(d_s32), r.mem.stream())
    np.testing.assert_array_equal(out.get(), (s32 * x.astype(np.float64)).astype(np.float32).reshape(-1))


# ----------------------------------------------------------------------------- al_peak_scale
def run_peak_scale(r, n, seed=7):
    """scale = s / (|s| max|x| + tiny32), evaluated in float64 and rounded once (0.5 ulp), clamped to the float32 range."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(-1, 1, n).astype(np.float32)
    clips = {
        "noise": base,
        "peak_at_end": np.concatenate([base[:-1] * 0.5, [np.float32(-1.5)]]).astype(np.float32),
        "denormal": (base * np.float32(1e-40)).astype(np.float32),
        "zeros": np.zeros(n, np.float32),
        "neg_zeros": np.full(n, -0.0, np.float32),
        "inf": np.concatenate([base[:n // 2], [np.inf], base[n // 2 + 1:]]).astype(np.float32)[:n],
        "nan": np.concatenate([base[:n // 2], [np.nan], base[n // 2 + 1:]]).astype(np.float32)[:n],
    }
    every = []
    for name, clip in clips.items():
        d = dev(r, clip)
        for s in (1.0, -1.0, float(np.float32(10 ** (12 / 20))), 4.0, 1e-3):
            out = Guarded(r, 1)
            r.lib.call("al_peak_scale", r.mem.ptr(d), n, ct.c_float(s), out.ptr, r.mem.stream())
            got = out.get()[0]
            every.append(got)
            s32 = float(np.float32(s))
            # fmaxf drops NaN, so the scale comes from the finite samples (the NaN samples themselves still reach the render,
            # whose finite check refuses them); an all-NaN clip leaves max 0
            finite_or_inf = np.abs(clip.astype(np.float64))[~np.isnan(clip)]
            ref = s32 / (abs(s32) * float(np.max(finite_or_inf, initial=0.0)) + TINY32)
            ref = float(np.clip(ref, -FLT_MAX, FLT_MAX))
            assert np.isfinite(got), (name, s, got)
            if ref == 0.0:
                assert got == 0.0, (name, s, got)
            else:
                record("peak_scale (ulp)", float(ulps(np.float64(got), ref)), 0.5 + 1e-6)
    return np.array(every, np.float32)


def run_clip_scales(r, lens, seed=17):
    """al_clip_scales over a batch whose events table points into one audio buffer: mode 0 passes prescale[e] through
    (bit-exact), mode 1 is the peak scale of the clip (same bound as al_peak_scale).  The descriptor carries only what the
    entry point reads: events, audio, clip_scale (a guarded output indexed by event)."""
    rng = np.random.default_rng(seed)
    E = len(lens)
    events = np.zeros(E, _hip.EVENT_DTYPE)
    offs = np.concatenate([[0], np.cumsum([(n + 3) // 4 * 4 for n in lens])])
    audio = rng.uniform(-1, 1, int(offs[-1])).astype(np.float32)
    for e, n in enumerate(lens):
        events[e]["audio_off"], events[e]["len"], events[e]["valid_len"] = offs[e], n, n
        if e % 3 == 2:
            audio[offs[e]:offs[e] + n] *= np.float32(1e-40)              # a denormal clip
    prescale = rng.choice(np.array([1.0, -1.0, 10 ** (12 / 20), -4.0, 1e-3], np.float32), E)
    mode = (np.arange(E) % 2).astype(np.int32)
    d_audio, d_events, d_pre, d_mode = dev(r, audio), dev(r, events), dev(r, prescale), dev(r, mode)
    out = Guarded(r, E)
    desc = _hip.AlBatch(log2_block=10, n_capsules=1, n_events=E, hop=1, audio=r.mem.ptr(d_audio), events=r.mem.ptr(d_events),
                        clip_scale=out.ptr)
    r.lib.call("al_clip_scales", ct.byref(desc), r.mem.ptr(d_pre), r.mem.ptr(d_mode), r.mem.stream())
    got = out.get()
    for e, n in enumerate(lens):
        s32 = float(prescale[e])
        if mode[e] == 0:
            assert_bits_equal(got[e:e + 1], prescale[e:e + 1], ("clip_scales mode 0", e))
            continue
        peak = float(np.max(np.abs(audio[offs[e]:offs[e] + n].astype(np.float64))))
        ref = float(np.clip(s32 / (abs(s32) * peak + TINY32), -FLT_MAX, FLT_MAX))
        record("peak_scale (ulp)", float(ulps(np.float64(got[e]), ref)), 0.5 + 1e-6)
    return got


# ----------------------------------------------------------------------------- al_row_stats, al_ambience_scales
def run_row_stats(r, rows, cols, nonfinite=False, seed=8):
    """{sum|x|, max|x|, non-finite count, sum x^2} per row.  Each partial is 64 serial float32 additions per thread, then a
    6-level wave tree and 4 waves in series: at most 73 roundings on non-negative terms, |err| <= 73u * sum; the float64
    combination of the partials is negligible.  Asserted: 40 eps = 80u, relative to the exact sum.  max and count exact."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (rows, cols)).astype(np.float32)
    chunk_ends = np.arange(16383, cols, 16384)
    x[:, chunk_ends] = 3.0 + rng.uniform(0, 1, (rows, len(chunk_ends)))   # each chunk's last sample sets that chunk's peak
    x[:, -1] = -5.0
    if nonfinite:
        x[0, cols // 3] = np.inf
        x[-1, cols // 2] = np.nan
        x[-1, 0] = -np.inf
    d = dev(r, x.reshape(-1))
    partials = r.mem.empty(r.lib.call("al_row_stats_partials", rows, cols))
    out = Guarded(r, 4 * rows, dtype=np.float64)
    r.lib.call("al_row_stats", r.mem.ptr(d), rows, cols, r.mem.ptr(partials), out.ptr, r.mem.stream())
    got = out.get().reshape(rows, 4)
    a = np.abs(x.astype(np.float64))
    bad = ~np.isfinite(a)
    np.testing.assert_array_equal(got[:, 2], bad.sum(axis=1))
    np.testing.assert_array_equal(got[:, 1], np.nanmax(np.where(np.isnan(a), -1.0, a), axis=1))   # fmaxf drops NaN, keeps Inf
    fin = ~bad.any(axis=1)
    for k, ref in ((0, a.sum(axis=1)), (3, (a * a).sum(axis=1))):
        err = np.abs(got[fin, k] - ref[fin]) / ref[fin]
        record("row_stats sums (rel err / eps)", float(err.max()) / EPS if err.size else 0.0, 40.0)
        np.testing.assert_array_equal(got[~fin, k], ref[~fin])    # Inf stays Inf, NaN (or Inf - Inf) is NaN
    return got


def run_ambience_scales(r, rows, cols, seed=9):
    """scales[c] from float64 row statistics computed here (no kernel output feeds it): float64 arithmetic, one rounding."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (rows, cols)) * rng.uniform(0.1, 3, (rows, 1))
    a = np.abs(x)
    stats = np.stack([a.sum(1), a.max(1), np.zeros(rows), (x * x).sum(1)], axis=1)
    if rows > 2:
        stats[1] = 0.0                     # a silent channel
    d = dev(r, stats.reshape(-1))
    tiny64 = np.finfo(np.float64).tiny
    every = []
    for normalize in (0, 1, 2):
        for ref_db in (-65.0, 0.0, 12.5):
            out = Guarded(r, rows)
            r.lib.call("al_ambience_scales", r.mem.ptr(d), rows, cols, ct.c_float(ref_db), normalize, out.ptr, r.mem.stream())
            got = out.get()
            every.append(got)
            inv = 1.0 / (stats[:, 1] + tiny64) if normalize else np.ones(rows)
            mean_abs = np.sum(stats[:, 0] * inv) / (rows * cols)
            mult = 10.0 ** (float(np.float32(ref_db)) / 20.0) / (mean_abs + tiny64)
            ref = np.clip(inv if normalize == 2 else mult * inv, -FLT_MAX, FLT_MAX)
            assert np.all(np.isfinite(got))
            record("ambience_scales (ulp)", float(ulps(got, ref).max()), 1.0)   # 0.5 rounding + float64 summation order
    return np.concatenate(every)


# ----------------------------------------------------------------------------- al_resample_poly
def resample_taps(up, down, half):
    from scipy import signal as sp_signal

    if half == 0:
        return np.array([up], np.float32)
    return (up * sp_signal.firwin(2 * half + 1, 1.0 / max(up, down, 2), window=("kaiser", 5.0))).astype(np.float32)


def run_resample(r, rows, n_in, up, down, half, pad=0, shift=0, seed=10):
    """out[m] = sum_j x[j] h[m*down - j*up + half] for m < n_out, zeros to out_pitch: the zero-stuffed input convolved with h
    and decimated, restated in float64 one polyphase branch at a time (every j with a tap in range, nothing clipped but the
    ends of x).  An output is an fma chain of at most K = ceil((2 half + 1) / up) terms: |err| <= K u sum|x_j h_i| per
    element (the standard gamma_K bound)."""
    x = np.stack([signal(n_in, seed + i) for i in range(rows)]).astype(np.float32)
    h = resample_taps(up, down, half)
    n_out = -(-n_in * up // down)
    pitch = n_out + pad
    out = Guarded(r, rows * pitch, shift=shift)
    d_x, d_h = dev(r, x.reshape(-1)), dev(r, h)
    r.lib.call("al_resample_poly", r.mem.ptr(d_x), rows, n_in, r.mem.ptr(d_h), half, up, down, out.ptr, n_out, pitch,
               r.mem.stream())
    got = out.get().reshape(rows, pitch)
    assert np.all(bits(got[:, n_out:]) == 0), "padding beyond n_out must be +0.0"
    K = -(-(2 * half + 1) // up)
    h64, x64 = h.astype(np.float64), x.astype(np.float64)
    worst = 0.0
    for m0 in range(0, n_out, 1 << 16):
        c = down * np.arange(m0, min(n_out, m0 + (1 << 16)), dtype=np.int64)
        j = -((half - c) // up) + np.arange(K + 1)[:, None]          # ceil((c - half) / up) + k: every j whose tap is in range
        tap = c - j * up + half
        ok = (j >= 0) & (j < n_in) & (tap >= 0) & (tap <= 2 * half)
        jj, tt = np.where(ok, j, 0), np.where(ok, tap, 0)
        hw = np.where(ok, h64[tt], 0.0)
        ref = (x64[:, jj] * hw).sum(axis=1)
        mag = (np.abs(x64[:, jj]) * np.abs(hw)).sum(axis=1)
        g = got[:, m0:m0 + len(c)].astype(np.float64)
        worst = max(worst, float(np.max(np.abs(g - ref) / np.maximum(K * U * mag, TINY32))))
        assert np.all(g[mag == 0] == 0)                               # an output no tap reaches is exactly zero
    record("resample_poly (err / (K u sum|x h|))", worst, 1.0)


# ----------------------------------------------------------------------------- IR packing
def run_pack_irs(r, rows, length, pitch, shift=0, seed=11):
    rng = np.random.default_rng(seed)
    src64 = rng.standard_normal((rows, length)) * np.exp(-rng.uniform(0, 40, (rows, length)))
    flat = src64.reshape(-1)
    flat[: min(8, flat.size)] = [0.5 + 2.0 ** -25, 1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, -0.0, 1e-42, 7e-46, 1e39, -np.inf][: min(8, flat.size)]
    want = np.zeros((rows, pitch), np.float32)
    with np.errstate(over="ignore"):
        want[:, :length] = src64.astype(np.float32)   # numpy's round-to-nearest-even cast (overflow -> inf)
    out = Guarded(r, rows * pitch, shift=shift)
    d64 = dev(r, src64.reshape(-1))
    r.lib.call("al_pack_irs_f64", r.mem.ptr(d64), out.ptr, rows, length, pitch, r.mem.stream())
    assert_bits_equal(out.get(), want.reshape(-1), ("pack_irs_f64", rows, length, pitch))
    src32 = signal(rows * length, seed).reshape(rows, length)
    want[:, :length] = src32
    out = Guarded(r, rows * pitch, shift=shift)
    d32 = dev(r, src32.reshape(-1))
    r.lib.call("al_pack_irs_f32", r.mem.ptr(d32), out.ptr, rows, length, pitch, r.mem.stream())
    assert_bits_equal(out.get(), want.reshape(-1), ("pack_irs_f32", rows, length, pitch))


def run_pack_ragged(r, lens, pitch, shift=0, seed=12):
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int32)
    gaps = rng.integers(0, 5, len(lens))
    offsets = np.cumsum(np.concatenate([[3], (lens + gaps)[:-1]])).astype(np.int64)
    total = int(offsets[-1] + lens[-1] + 3)
    for f64 in (0, 1):
        src = rng.standard_normal(total) if f64 else signal(total, seed)
        want = np.zeros((len(lens), pitch), np.float32)
        for i, (o, n) in enumerate(zip(offsets, lens)):
            want[i, :n] = src[o:o + n].astype(np.float32)
        out = Guarded(r, len(lens) * pitch, shift=shift)
        d_src, d_off, d_len = dev(r, src), dev(r, offsets), dev(r, lens)
        r.lib.call("al_pack_ragged_irs", r.mem.ptr(d_src), f64, r.mem.ptr(d_off), r.mem.ptr(d_len), len(lens), pitch, out.ptr,
                   r.mem.stream())
        assert_bits_equal(out.get(), want.reshape(-1), ("pack_ragged", f64))


# ----------------------------------------------------------------------------- al_noise_irfft: the any-size inverse real FFT
# Lengths n of the inverse real transform, chosen by the COMPLEX length the Stockham passes run (len = n / 2 for even n, n for
# odd n).  k_big_pass<R> gives one thread to each of the len / R butterflies of a pass, 256 threads to a workgroup, and
# big_fft takes the radices in the order 4, 2, 3, 5, 7 (ns = the product of the radices already done).  Each row says what it
# is there for; test_*_kernel_edges.py run them all with rows = 2 (blockIdx.y) and one of them with rows = 3.
NOISE_STOCKHAM_N = [
    # the last workgroup of an odd-radix pass exactly full: len / R == 256
    (1536, "len 768 = 4^4 3: the radix-3 pass is one full workgroup (256 butterflies)"),
    (2560, "len 1280 = 4^4 5: the radix-5 pass is one full workgroup"),
    (3584, "len 1792 = 4^4 7: the radix-7 pass is one full workgroup"),
    # ... and a little over: a second, partly filled workgroup
    (1920, "len 960 = 4^3 3 5: radix 3 runs 320 butterflies (64 live lanes in workgroup 1), radix 5 192"),
    (2880, "len 1440 = 4^2 2 3^2 5: radix 5 runs 288 (32 live lanes in workgroup 1), both radix-3 passes 480"),
    (3780, "len 1890 = 2 3^3 5 7: radix 7 runs 270 (14 live lanes in workgroup 1) at ns = 270"),
    # pure prime powers: the generic butterfly with its (r q) % R twiddle in every pass, ns growing to len / R; odd n = len
    # takes the Hermitian-extension branch of k_noise_pack / k_noise_unpack over several workgroups
    (2187, "len 3^7, odd n: seven radix-3 passes of 729 butterflies (3 workgroups), ns 1 .. 729"),
    (3125, "len 5^5, odd n: five radix-5 passes of 625 butterflies (3 workgroups), ns 1 .. 625"),
    (2401, "len 7^4, odd n: four radix-7 passes of 343 butterflies (2 workgroups), ns 1 .. 343"),
    (16807, "len 7^5, odd n: five radix-7 passes of 2401 butterflies (10 workgroups), ns 1 .. 2401"),
    # the same len from an even n: the half-length packing (E + iO) with an odd len
    (4374, "len 3^7 from even n: half-length packing with an odd len"),
    (4802, "len 7^4 from even n: half-length packing with an odd len"),
    # all five radices in one transform, in the dispatch order 4, 2, 3, 3, 5, 7, the radix-7 pass in two workgroups
    (5040, "len 2520 = 2^3 3^2 5 7: passes 4, 2, 3, 3, 5, 7; radix 7 runs 360 butterflies (2 workgroups) at ns = 360"),
    (11025, "len 11025 = 3^2 5^2 7^2, odd n: an odd mix, passes 3, 3, 5, 5, 7, 7; radix 7 at ns = 225 and 1575 (7 workgroups)"),
    (22050, "len 11025 from even n"),
]
NOISE_STOCKHAM_ROWS3 = 5040       # the rows = 3 case: every radix, the radix-7 pass multi-block
# a large ns under each odd radix (one odd pass after nine radix-4 or eight radix-4 and one radix-2 pass) and the two long prime
# powers: emulated workgroups are too slow for these
NOISE_STOCKHAM_N_GPU = [
    (2 * 3 * 2 ** 18, "len 3 2^18: the radix-3 pass at ns = 2^18 (1024 workgroups)"),
    (2 * 5 * 2 ** 17, "len 5 2^17: the radix-5 pass at ns = 2^17 (512 workgroups)"),
    (2 * 7 * 2 ** 17, "len 7 2^17: the radix-7 pass at ns = 2^17 (512 workgroups)"),
    (2 * 5 ** 8, "len 5^8 = 390625 from even n: eight radix-5 passes of 78125 butterflies, ns 1 .. 78125"),
    (7 ** 7, "len 7^7 = 823543, odd n: seven radix-7 passes of 117649 butterflies, ns 1 .. 117649"),
]

# (fft, win, hop) of al_stft and al_istft_ola beyond the powers of two and the Bluestein sizes of the parametrisations
STFT_GEOMETRIES = [
    # smooth, not a power of two: Stockham passes of radix 3 / 5 / 7 behind the STFT entry points
    (384, 256, 64),      # 2^7 3
    (480, 240, 120),     # 2^5 3 5
    (1000, 500, 125),    # 2^3 5^3
    (210, 105, 35),      # 2 3 5 7, odd window and hop
    (105, 64, 16),       # odd smooth: 3 5 7
    (343, 128, 32),      # odd prime power 7^3
    (2520, 512, 128),    # every radix; the radix-7 pass (360 butterflies) in two workgroups per series
    # crop: fft < win keeps the first fft samples of each windowed frame (rfft(frames, n=fft)); the inverse overlap-adds
    # fft-sample frames and still slices from win
    (48, 64, 16),
    # win == hop: no left padding, frames do not overlap in the forward direction
    (32, 16, 16),
    # tiny: a length-1 transform runs no pass at all and returns its input buffer; win = 1 makes the sin^2 window zero
    (1, 1, 1), (2, 2, 1), (3, 2, 1),
]
# more series than one launch group (MAX_GRID_ROWS = 32768) holds: a smooth size and a Bluestein size (its scratch and
# chirp spectrum are made again by the second group)
GROUP_FFTS = (6, 11)
GROUP_STFT = dict(rows=2, n=40000, win=4, hop=2)        # 20 001 frames, 40 002 series: group 1 starts at frame 12 767 of row 1
GROUP_ISTFT = dict(n_frames=11000, n_ch=3, win=4, hop=2)  # 33 000 series: series 32 768 is channel 2 of frame 10 922


def fft_bound(length):
    """(log2 of the transform length the kernels run, Bluestein?) for a complex transform of `length` points: Stockham
    passes where it factors into 2 / 3 / 5 / 7, else Bluestein on L = the next power of two >= 2 length - 1."""
    m = length
    for f in (2, 3, 5, 7):
        while m % f == 0:
            m //= f
    if m == 1:
        return max(float(np.log2(max(length, 2))), 1.0), False
    L = 1
    while L < 2 * length - 1:
        L <<= 1
    return float(np.log2(L)), True


def run_noise_irfft(r, rows, n, seed=13):
    """out = irfft(shape * (zr + i zi) with the DC / Nyquist fix-ups) * inv_sigma, reference numpy's float64 irfft.

    Bound: a radix-r Stockham pass adds at most a few u of the data's norm (twiddles from float64 sincospi); log2(len) passes
    give |err|_2 <= c log2(len) u |y|_2.  Against the peak of a noise-like output (peak ~ 4 rms, errors spread evenly) that is a
    max-abs error of about log2(len) u; the real-packing step adds one level.  Bluestein runs three FFTs of length L = 2^k
    >= 2 len - 1 and two chirp multiplications: about 3 log2(L) u.  Asserted: 2 (log2 len + 1) eps (Stockham), and
    3 (log2 L + 1) eps (Bluestein), relative to max|ref|.

    The constants were argued for radix-2 / 4 passes.  A length made of 5s or 7s runs fewer passes than log2(len), each output
    of a pass taking R - 1 complex multiply-adds; measured, those lengths sit as far below the bound as the powers of two do
    (profiles/r10_anyfft_edges.txt: 7^5 0.08, 5^5 0.10, 3^2 5^2 7^2 0.10 of the 2 in the host emulation), so log2(len)
    stays the count."""
    rng = np.random.default_rng(seed)
    bins = n // 2 + 1
    zr = rng.standard_normal((rows, bins)).astype(np.float32)
    zi = rng.standard_normal((rows, bins)).astype(np.float32)
    shape = (1.0 / np.sqrt(1.0 + np.arange(bins))).astype(np.float32)     # a 1/f-like shaping
    inv_sigma = float(np.float32(0.37))
    work = workspace(r, r.lib.call("al_noise_workspace_floats", rows, n))
    out = Guarded(r, rows * n)
    d_zr, d_zi, d_s = dev(r, zr.reshape(-1)), dev(r, zi.reshape(-1)), dev(r, shape)
    r.lib.call("al_noise_irfft", r.mem.ptr(d_zr), r.mem.ptr(d_zi), r.mem.ptr(d_s), rows, n, ct.c_float(inv_sigma), out.ptr,
               work.ptr, r.mem.stream())
    got = out.get().reshape(rows, n)
    work.get()
    S = shape.astype(np.float64) * (zr.astype(np.float64) + 1j * zi.astype(np.float64))
    S[:, 0] = S[:, 0].real * np.sqrt(2)
    if n % 2 == 0:
        S[:, -1] = S[:, -1].real * np.sqrt(2)
    ref = np.fft.irfft(S, n=n, axis=-1) * inv_sigma
    lg, blue = fft_bound(n if n % 2 else n // 2)      # even n: half-length complex transform + real packing
    bound = (3.0 if blue else 2.0) * (lg + 1) * EPS
    for row in range(rows):
        record(f"noise_irfft {'bluestein' if blue else 'stockham'} (err/peak / ((log2+1) eps))",
               peak_error(got[row], ref[row]) / ((lg + 1) * EPS), bound / ((lg + 1) * EPS))
        if n >= 16:
            assert_parity(got[row], ref[row], what=("noise_irfft", n, row))


# ----------------------------------------------------------------------------- al_stft / al_istft_ola
def run_stft(r, rows, n, fft, win, hop, seed=14, last_written=False):
    """sin^2-windowed rFFT frames (oracle.stft_frames, scipy float64).  Same FFT bound as the noise path, relative to the
    spectrum's peak; every output guarded (the spectrum is written by k_stft_take_half, one row per series), every element
    compared.  fft < win crops each windowed frame to its first fft samples, as the reference's rfft(frames, n=fft) does.
    ``last_written``: also assert that the last series is not silent (an unwritten last launch group must not pass)."""
    x = np.stack([signal(n, seed + i, special=False) for i in range(rows)]).astype(np.float32)
    n_frames = orc.frame_count(n, hop)
    nf = fft // 2 + 1
    work = workspace(r, r.lib.call("al_stft_workspace_floats", rows * n_frames, fft))
    out = Guarded(r, rows * n_frames * nf * 2)
    d = dev(r, x.reshape(-1))
    r.lib.call("al_stft", r.mem.ptr(d), rows, n, fft, win, hop, out.ptr, work.ptr, r.mem.stream())
    got = out.get().view(np.complex64).reshape(rows, n_frames, nf)
    work.get()
    if last_written:
        assert np.abs(got[-1]).max() > 0, "the last row of the spectrum is silent"
        assert np.abs(got[-1, -1]).max() > 0, "the last series of the last launch group is silent"
    lg, blue = fft_bound(fft)
    bound = 3.0 if blue else 2.0            # in units of (log2 + 1) eps, as for the noise path
    for row in range(rows):
        ref = orc.stft_frames(x[row].astype(np.float64), fft, win, hop)
        assert ref.shape == got[row].shape
        record(f"stft {'bluestein' if blue else 'stockham'} (err/peak / ((log2+1) eps))",
               peak_error(got[row], ref) / ((lg + 1) * EPS), bound)
        assert_parity(np.stack([got[row].real, got[row].imag]), np.stack([ref.real, ref.imag]), what=("stft", fft, row))


def run_tv_stft_mac(r, n_frames, n_frames_ir, n_freq, n_ch, n_irs, seed=18):
    """out[i] = sum_{k <= min(i, F_ir - 1)} S[i-k] * sum_l W[i-k, l] H[k, :, :, l] (oracle.convolve_moving_stft's loop),
    restated with numpy in complex128.  Per element: an fma chain of n_irs terms for the weighted IR, one complex product and
    one complex accumulation per k, so |err| <= (n_irs + K + 2) eps * sum_k |S| sum_l |W| |H| with K = min(i, F_ir-1) + 1."""
    rng = np.random.default_rng(seed)
    cplx = lambda *shape: (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    s_a, s_h = cplx(n_frames, n_freq), cplx(n_frames_ir, n_freq, n_ch, n_irs)
    w = rng.uniform(0, 1, (n_frames, n_irs)).astype(np.float32)
    w[w < 0.3] = 0.0                                                     # the kernel skips zero weights
    out = Guarded(r, n_frames * n_freq * n_ch * 2)
    d_a, d_h, d_w = dev(r, s_a.view(np.float32)), dev(r, s_h.view(np.float32)), dev(r, w)
    r.lib.call("al_tv_stft_mac", r.mem.ptr(d_a), r.mem.ptr(d_h), r.mem.ptr(d_w), n_frames, n_frames_ir, n_freq, n_ch, n_irs, out.ptr,
               r.mem.stream())
    got = out.get().view(np.complex64).reshape(n_frames, n_freq, n_ch).astype(np.complex128)
    A, H, W = s_a.astype(np.complex128), s_h.astype(np.complex128), w.astype(np.float64)
    ref = np.zeros((n_frames, n_freq, n_ch), np.complex128)
    mag = np.zeros((n_frames, n_freq, n_ch))
    for i in range(n_frames):
        for k in range(min(i, n_frames_ir - 1) + 1):
            ref[i] += A[i - k][:, None] * (H[k] @ W[i - k])
            mag[i] += np.abs(A[i - k])[:, None] * (np.abs(H[k]) @ W[i - k])
    K = np.minimum(np.arange(n_frames), n_frames_ir - 1) + 1
    bound = (n_irs + K + 2)[:, None, None] * EPS * mag
    record("tv_stft_mac (err / ((n_irs + K + 2) eps sum|S W H|))", float(np.max(np.abs(got - ref) / np.maximum(bound, TINY32))), 1.0)


def run_istft(r, n_frames, n_ch, fft, win, hop, seed=15, last_written=False):
    """irfft(n=fft, norm="forward") of every (frame, channel), overlap-add at i*hop, slice [win, n_frames*hop): the
    reference restated with numpy's float64 irfft.  Each output sample sums ceil(fft/hop) frames: FFT bound + that many
    additions, relative to the output's peak.  The overlap-add buffer here is long enough for any fft (the reference's own
    holds (n_frames + 1) hop + win samples, so it raises for fft > 2 hop + win; the slice it returns ends before that tail
    and is the same).  ``last_written``: also assert that the last output sample, which only frames of the last launch group
    reach, is not silent."""
    nf = fft // 2 + 1
    rng = np.random.default_rng(seed)
    spec = (rng.standard_normal((n_frames, nf, n_ch)) + 1j * rng.standard_normal((n_frames, nf, n_ch))).astype(np.complex64)
    work = workspace(r, r.lib.call("al_istft_workspace_floats", n_frames, n_ch, fft))
    n_out = n_frames * hop - win
    out = Guarded(r, n_out * n_ch)
    d = dev(r, spec.view(np.float32).reshape(-1))
    r.lib.call("al_istft_ola", r.mem.ptr(d), n_frames, nf, n_ch, fft, win, hop, out.ptr, work.ptr, r.mem.stream())
    got = out.get().reshape(n_out, n_ch)
    work.get()
    if last_written:
        assert np.abs(got[-1]).max() > 0, "the last output sample (fed by the last launch group alone) is silent"
    frames = sp_fft.irfft(spec.astype(np.complex128), n=fft, axis=1, norm="forward")     # (F, fft, ch)
    ola = np.zeros((n_frames * hop + fft, n_ch))
    for i in range(n_frames):
        ola[i * hop:i * hop + fft] += frames[i]
    ref = ola[win:n_frames * hop]
    lg, blue = fft_bound(fft)
    overlap = -(-fft // hop)
    bound = (3.0 if blue else 2.0) + overlap / (lg + 1)      # in units of (log2 + 1) eps
    record(f"istft_ola {'bluestein' if blue else 'stockham'} (err/peak / ((log2+1) eps))", peak_error(got, ref) / ((lg + 1) * EPS),
           bound)
    assert_parity(got, ref, what=("istft", fft))


# ----------------------------------------------------------------------------- al_encode_frames
# scaled = x * 32768 at every rounding tie near zero, at the saturation points and just inside / outside them.  (At exactly
# 32767.0 and -32768.0 the saturating branch and the rintf branch give the same value, so `>=` vs `>` there is unobservable.)
PCM_EDGES = np.array([0.0, -0.0, 1e-40, -1e-40, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, -0.5 / 32768, -2.5 / 32768,
                      32766.5 / 32768, 32767.0 / 32768, 32767.4 / 32768, 32767.5 / 32768, 32767.9 / 32768, 1.0, 1.5, np.inf,
                      -32767.5 / 32768, -32768.0 / 32768, -32768.5 / 32768, -1.5, -np.inf], dtype=np.float32)


def run_encode(r, n_capsules, n_samples, fmt, shift=0, seed=16, guarded=None):
    """(C, T) -> (T, C) frames, bit-exact: float32 copies, PCM_16 = tests.conftest.pcm16 (libsndfile's clipping f2s).
    ``guarded``: another guarded-buffer class for the frames (tests/transfer_cases.py: page-locked host memory)."""
    rng = np.random.default_rng(seed)
    scene = rng.uniform(-1.05, 1.05, (n_capsules, n_samples)).astype(np.float32)
    flat = scene.reshape(-1)
    k = min(len(PCM_EDGES), flat.size)
    flat[:k] = PCM_EDGES[:k]
    flat[-k:] = PCM_EDGES[::-1][:k]
    dtype = np.int16 if fmt == _hip.FRAMES_PCM16 else np.float32
    out = (guarded or Guarded)(r, n_capsules * n_samples, dtype=dtype, shift=shift)
    d = dev(r, flat)
    r.lib.call("al_encode_frames", r.mem.ptr(d), n_capsules, n_samples, fmt, out.ptr, r.mem.stream())
    want = pcm16(scene.T) if fmt == _hip.FRAMES_PCM16 else scene.T
    got = out.get()
    assert_bits_equal(got, np.ascontiguousarray(want).reshape(-1), ("encode", n_capsules, n_samples, fmt))
    return got
