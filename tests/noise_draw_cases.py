"""Scenarios that pin the device-drawn ambience noise (Ambience(rng="device")) element for element, shared by
tests/test_hostemu_noise_draws.py (host emulation, reduced sizes) and tests/test_gpu_noise_draws.py (gfx950 build).

A chain of three comparisons, each link resting on a float64 restatement or on a link already made; no device output is kept
as a golden array:

  A  al_normal_fill equals its documented function.  Element i is normal (i % 4) of Philox-4x32-10 block q = i // 4 with
     counter (q lo, q hi, tag, 0) and key (seed lo, seed hi) (oracle.synth_oracle.philox4x32_10, itself held to the Random123
     known-answer vectors), Box-Muller as csrc/al_rng.h states it: u1 and u2 formed in float32, radius and angle here in float64.
     Tolerance: rtol 2e-5, atol 2e-6 |scale| (the device's logf / sqrtf / sincospif against float64), on both back ends.
  B  al_noise_irfft_seeded equals al_noise_irfft on the device's own draws.  A tag-1, scale-1 fill of 4 * rows * bins elements
     holds exactly what spectrum_draw reads: zr[row, f] = fill[4 (row bins + f)], zi[row, f] = fill[4 (row bins + f) + 1]; A ties
     that fill to the restatement and tests/kernel_edges.py holds al_noise_irfft to float64 at these lengths, so the seeded call
     must return the SAME BITS as the explicit one.  (Both kernels inline the same box_muller, which holds no multiply-add pair
     a compiler could contract.)  Beside it the seeded output is compared with a float64 irfft of the restated draws: the
     transform's bound of tests/kernel_edges.py plus A's draw tolerance carried through the transform.
  C  the Python layer hands out those draws: powerlaw_psd_gaussian (white: the tag-2 fill; coloured: B's chain), a "gaussian"
     Ambience (the tag-3 fill), a seed=None Ambience through its dictionary, and a scene whose oracle mix takes its noise from
     the restated chain.

Every output is a guarded buffer (tests/kernel_edges.py): a 16-byte store past n is seen."""
import ctypes as ct
import functools

import numpy as np

from audiblelight_amd import _hip, ambience as amb
from oracle import synth_oracle as orc
from tests.kernel_edges import EPS, NOISE_STOCKHAM_N, Guarded, assert_bits_equal, dev, fft_bound, peak_error, record, sentinel_bytes, workspace

RTOL, ATOL = 2e-5, 2e-6                 # of one draw against the float64 restatement (tests/test_hostemu_rng.py holds the same)
FILL_CAP = 4 * 16384 * 256              # elements one trip of al_normal_fill's grid covers: 16 384 blocks, 256 threads, 4 each
TAG_SPECTRUM, TAG_WHITE, TAG_GAUSSIAN = 1, 2, 3

FILL_SMALL_N = (1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025)     # 1023 / 1025 = 4 * 256 -+ 1: one full workgroup of quads less / more one
SEEDS = (0xFFFFFFFF00000001, 0x12345678, 0)        # all high key bits set, below 2^32, zero
TAGS = (1, 2, 3, 7)

# lengths of the seeded transform: tiny; both parities around one 256-thread workgroup of k_noise_pack (even n runs n / 2
# threads, so 510 / 512 / 514 straddle it, odd n runs n); a smooth multi-radix length; Bluestein of each parity
SEEDED_N = (1, 2, 3, 4, 510, 511, 512, 513, 514, 1920, 1009, 2018)
assert 1920 in [n for n, _ in NOISE_STOCKHAM_N]


# ----------------------------------------------------------------------------- the restatement
@functools.lru_cache(maxsize=None)
def _block(seed, tag, q):
    """The four N(0, 1) of Philox block q under (seed, tag), float64."""
    x = orc.philox4x32_10((q & 0xffffffff, q >> 32, tag, 0), (seed & 0xffffffff, seed >> 32))
    out = []
    for h in range(2):
        u1 = (np.float32(x[2 * h]) + np.float32(0.5)) * np.float32(2.0 ** -32)
        u2 = np.float32(x[2 * h + 1]) * np.float32(2.0 ** -32)
        rad = np.sqrt(-2.0 * np.log(np.float64(u1)))
        out += [rad * np.cos(2 * np.pi * np.float64(u2)), rad * np.sin(2 * np.pi * np.float64(u2))]
    return tuple(float(v) for v in out)


def restated_normals(seed, tag, lo, hi):
    """Elements [lo, hi) of the unit-scale fill under (seed, tag), float64."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    flat = np.array([_block(seed, int(tag), q) for q in range(lo // 4, (hi + 3) // 4)], dtype=np.float64).reshape(-1)
    return flat[lo - 4 * (lo // 4): hi - 4 * (lo // 4)]


def restated_spectrum_draws(seed, rows, bins):
    """(zr, zi), each (rows, bins) float64: the first Box-Muller pair of block row * bins + f under tag 1."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    z = np.array([_block(seed, TAG_SPECTRUM, q)[:2] for q in range(rows * bins)], dtype=np.float64).reshape(rows, bins, 2)
    return z[..., 0], z[..., 1]


def check_draws(got, want, scale, family, what=None):
    """|got - scale * want| <= ATOL |scale| + RTOL |scale * want| on every element; the worst ratio is recorded."""
    s = float(np.float32(scale))
    want = np.asarray(want, dtype=np.float64) * s
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape, what)
    assert np.all(np.isfinite(got)), what
    ratio = np.abs(got - want) / (ATOL * abs(s) + RTOL * np.abs(want))
    worst = float(ratio.max())
    assert worst <= 1.0, (family, what, f"element {int(ratio.argmax())}: {got.reshape(-1)[ratio.argmax()]!r} vs "
                          f"{want.reshape(-1)[ratio.argmax()]!r}, {worst:.3g} of the tolerance")
    record(family, worst, 1.0)


def raises_badarg(call, *needles):
    try:
        call()
    except _hip.HipError as exc:
        assert f"({_hip.AL_E_BADARG})" in str(exc), exc
        for needle in needles:
            assert needle in str(exc), (needle, str(exc))
    else:
        raise AssertionError("the call was accepted")


# ----------------------------------------------------------------------------- A: al_normal_fill
def fill(r, n, seed, tag, scale=1.0):
    """al_normal_fill into a guarded buffer; returns the Guarded (its .get() checks the bands)."""
    out = Guarded(r, n)
    r.lib.call("al_normal_fill", out.ptr, n, ct.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), tag, ct.c_float(scale), r.mem.stream())
    return out


def run_fill(r, n, seed, tag, scale=1.0, windows=None):
    """One fill compared with the restatement in full, or on the given [lo, hi) windows.  Returns the output."""
    got = fill(r, n, seed, tag, scale).get()
    for lo, hi in (windows or [(0, n)]):
        check_draws(got[lo:hi], restated_normals(seed, tag, lo, hi), scale, "normal_fill (err / tolerance)",
                    (n, hex(seed), tag, scale, lo, hi))
    return got


def white_scale(n):
    return float(np.sqrt(2.0 / n) / amb._flat_sigma(n))


def run_fill_independence(r, n=1024):
    """Another tag or another high key word is another stream.  Two independent float32 normals coincide with a probability of
    about 1e-8 (density 0.4 times the spacing near 1), so even one equal pair among 1024 is not chance; a mapping that drops
    the tag or the high key word makes all of them equal."""
    base = fill(r, n, 5, 1).get()
    for what, other in (("tag 2", fill(r, n, 5, 2)), ("tag 3", fill(r, n, 5, 3)), ("seed + 2^32", fill(r, n, 5 + (1 << 32), 1)),
                        ("seed + 1", fill(r, n, 6, 1))):
        same = int(np.sum(other.get() == base))
        assert same == 0, (what, same)
        assert abs(np.corrcoef(other.get(), base)[0, 1]) < 6 / np.sqrt(n), what


def run_fill_prefix(r, n, ks, seed=0xC0FFEE12345, tag=2, scale=0.75):
    """Geometry independence: the first k elements of a fill of n are a fill of k, bit for bit (a fill of k launches another
    grid, and for k or n above FILL_CAP the later trips of the stride)."""
    whole = fill(r, n, seed, tag, scale).get()
    for k in ks:
        assert_bits_equal(fill(r, k, seed, tag, scale).get(), whole[:k], ("prefix", n, k))
    return whole


def run_fill_refusals(r):
    g = Guarded(r, 64)
    s = r.mem.stream()
    raises_badarg(lambda: r.lib.call("al_normal_fill", g.ptr + 4, 8, ct.c_uint64(1), 1, ct.c_float(1.0), s), "16-byte aligned")
    raises_badarg(lambda: r.lib.call("al_normal_fill", g.ptr, 0, ct.c_uint64(1), 1, ct.c_float(1.0), s))
    raises_badarg(lambda: r.lib.call("al_normal_fill", g.ptr, -4, ct.c_uint64(1), 1, ct.c_float(1.0), s))
    raises_badarg(lambda: r.lib.call("al_normal_fill", None, 8, ct.c_uint64(1), 1, ct.c_float(1.0), s))
    raw = np.asarray(r.mem.download(g.buf)).view(np.uint8)          # refused before anything was launched: the interior too
    assert np.array_equal(raw, sentinel_bytes(len(raw)))
    g.get()


# ----------------------------------------------------------------------------- B: al_noise_irfft_seeded
def pink_shape(n):
    """(shape, 1 / sigma) as powerlaw_noise_device forms them for pink noise.  Below n = 4 _spectral_shape has no finite answer
    (no bin above DC to take the DC value from), so those lengths get a 1/f-like shape of their own."""
    if n >= 4:
        s, sigma = amb._spectral_shape(1, n, 0)
        return np.array(s, dtype=np.float32), float(1.0 / sigma)
    return (1.0 / np.sqrt(1.0 + np.arange(n // 2 + 1))).astype(np.float32), 0.37


def device_draws(r, seed, rows, bins):
    """(zr, zi) as (rows, bins) float32 out of the tag-1, unit-scale fill: what spectrum_draw computes for (row, f)."""
    f = fill(r, 4 * rows * bins, seed, TAG_SPECTRUM).get()
    return f[0::4].reshape(rows, bins).copy(), f[1::4].reshape(rows, bins).copy()


def seeded(r, seed, shape, rows, n, inv_sigma):
    work = workspace(r, r.lib.call("al_noise_workspace_floats", rows, n))
    out = Guarded(r, rows * n)
    d_s = dev(r, shape) if shape is not None else None
    r.lib.call("al_noise_irfft_seeded", ct.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), r.mem.ptr(d_s) if d_s is not None else None,
               rows, n, ct.c_float(inv_sigma), out.ptr, work.ptr, r.mem.stream())
    got = out.get().reshape(rows, n)
    work.get()
    return got


def explicit(r, zr, zi, shape, rows, n, inv_sigma):
    work = workspace(r, r.lib.call("al_noise_workspace_floats", rows, n))
    out = Guarded(r, rows * n)
    d_zr, d_zi, d_s = dev(r, zr.reshape(-1)), dev(r, zi.reshape(-1)), dev(r, shape)
    r.lib.call("al_noise_irfft", r.mem.ptr(d_zr), r.mem.ptr(d_zi), r.mem.ptr(d_s), rows, n, ct.c_float(inv_sigma), out.ptr,
               work.ptr, r.mem.stream())
    got = out.get().reshape(rows, n)
    work.get()
    return got


def float64_noise(zr, zi, shape, n, inv_sigma):
    """(irfft of the shaped spectrum with the DC / Nyquist fix-ups) * inv_sigma in float64, and per row the worst |error| the
    draw tolerance can cause in any output sample: the transform is linear, bin f reaches every sample with weight c_f / n
    (c = 2, the fix-up bins sqrt 2), and a draw is off by at most RTOL |z| + ATOL per component."""
    s = np.asarray(shape, dtype=np.float64)
    S = s * (zr + 1j * zi)
    S[:, 0] = S[:, 0].real * np.sqrt(2)
    c = np.full(len(s), 2.0)
    c[0] = np.sqrt(2)
    dz = np.hypot(RTOL * np.abs(zr) + ATOL, RTOL * np.abs(zi) + ATOL)
    if n % 2 == 0:
        S[:, -1] = S[:, -1].real * np.sqrt(2)
        c[-1] = np.sqrt(2)
    dz[:, 0] = RTOL * np.abs(zr[:, 0]) + ATOL
    if n % 2 == 0:
        dz[:, -1] = RTOL * np.abs(zr[:, -1]) + ATOL
    s32 = abs(float(np.float32(inv_sigma)))
    return np.fft.irfft(S, n=n, axis=-1) * float(np.float32(inv_sigma)), (c * s * dz).sum(axis=1) * s32 / n


def run_seeded(r, rows, n, seed, shaped=True, identical=True):
    """al_noise_irfft_seeded against (1) al_noise_irfft on the draws al_normal_fill made for the same seed: the same bits, and
    (2) the float64 transform of the restated draws.  ``shaped=False`` runs the shape == nullptr arm against a vector of ones.
    ``identical=False`` drops (1) (see profiles/r11_untested_paths.txt for where that would be needed)."""
    bins = n // 2 + 1
    shape, inv_sigma = pink_shape(n) if shaped else (np.ones(bins, np.float32), float(np.float32(1.0 / np.sqrt(n))))
    got = seeded(r, seed, shape if shaped else None, rows, n, inv_sigma)
    if identical:
        zr, zi = device_draws(r, seed, rows, bins)
        assert_bits_equal(got, explicit(r, zr, zi, shape, rows, n, inv_sigma), ("seeded vs explicit", rows, n, hex(seed), shaped))
    ref, carried = float64_noise(*restated_spectrum_draws(seed, rows, bins), shape, n, inv_sigma)
    lg, blue = fft_bound(n if n % 2 else n // 2)
    for row in range(rows):
        peak = float(np.max(np.abs(ref[row])))
        bound = (3.0 if blue else 2.0) * (lg + 1) * EPS + carried[row] / peak
        record("noise_irfft_seeded vs float64 of the restated draws (err/peak / bound)", peak_error(got[row], ref[row]) / bound, 1.0)
    for a in range(rows):                 # rows are streams of their own
        for b in range(a + 1, rows):
            assert not np.array_equal(got[a], got[b]), ("rows repeat", a, b)
    return got


def run_seeded_refusals(r):
    s = r.mem.stream()
    n, rows = 16, 2
    shape = dev(r, np.ones(n // 2 + 1, np.float32))
    work = workspace(r, r.lib.call("al_noise_workspace_floats", rows, n))
    out = Guarded(r, rows * n)
    call = lambda o, w, rw, nn: r.lib.call("al_noise_irfft_seeded", ct.c_uint64(3), r.mem.ptr(shape), rw, nn, ct.c_float(1.0), o, w, s)
    raises_badarg(lambda: call(None, work.ptr, rows, n), "bad noise arguments")
    raises_badarg(lambda: call(out.ptr, None, rows, n), "bad noise arguments")
    raises_badarg(lambda: call(out.ptr, work.ptr, 0, n), "bad noise arguments")
    raises_badarg(lambda: call(out.ptr, work.ptr, rows, 0), "bad noise arguments")
    raw = np.asarray(r.mem.download(out.buf)).view(np.uint8)
    assert np.array_equal(raw, sentinel_bytes(len(raw)))
    work.get()


# ----------------------------------------------------------------------------- C: the Python layer
def run_python_white(r, rows, n, seed):
    """powerlaw_psd_gaussian(0, ...) is the flat tag-2 fill of rows * n elements times sqrt(2 / n) / _flat_sigma(n): row k starts
    at element k n."""
    got = amb.powerlaw_psd_gaussian(0, (rows, n), seed=seed, rng="device")
    assert got.shape == (rows, n) and got.dtype == np.float64
    scale = white_scale(n)
    check_draws(got.reshape(-1), restated_normals(seed, TAG_WHITE, 0, rows * n), scale, "python white (err / tolerance)", (rows, n))
    assert_bits_equal(got.astype(np.float32).reshape(-1), fill(r, rows * n, seed, TAG_WHITE, scale).get(), ("white vs fill", rows, n))
    for a in range(rows):
        for b in range(a + 1, rows):
            assert int(np.sum(got[a] == got[b])) == 0, ("rows repeat", a, b)


def run_python_coloured(r, rows, n, seed, identical=True):
    """powerlaw_psd_gaussian(1, ...) is B's chain with _spectral_shape(1, n, 0)."""
    got = amb.powerlaw_psd_gaussian(1, (rows, n), seed=seed, rng="device")
    assert got.shape == (rows, n)
    shape, inv_sigma = pink_shape(n)
    bins = n // 2 + 1
    if identical:
        zr, zi = device_draws(r, seed, rows, bins)
        assert_bits_equal(got.astype(np.float32), explicit(r, zr, zi, shape, rows, n, inv_sigma), ("coloured vs explicit", rows, n))
    ref, carried = float64_noise(*restated_spectrum_draws(seed, rows, bins), shape, n, inv_sigma)
    lg, blue = fft_bound(n if n % 2 else n // 2)
    for row in range(rows):
        bound = (3.0 if blue else 2.0) * (lg + 1) * EPS + carried[row] / float(np.max(np.abs(ref[row])))
        record("python coloured vs float64 of the restated draws (err/peak / bound)", peak_error(got[row], ref[row]) / bound, 1.0)


def run_python_gaussian(r, channels, total, seed, sr=8000):
    """A "gaussian" device Ambience, not normalised, is the tag-3 fill of channels * total elements at scale 1."""
    a = amb.Ambience(channels, total / sr, alias="g", noise="gaussian", sample_rate=sr, rng="device", seed=seed)
    got = a.load_ambience(normalize=False)
    assert got.shape == (channels, total)
    check_draws(got.reshape(-1), restated_normals(seed, TAG_GAUSSIAN, 0, channels * total), 1.0, "python gaussian (err / tolerance)",
                (channels, total))


def run_python_seedless(r, channels, total, sr=8000):
    """seed=None: the key is entropy drawn once and recorded as device_seed; the dictionary's twin draws with THAT key."""
    a = amb.Ambience(channels, total / sr, alias="g", noise="gaussian", sample_rate=sr, rng="device")
    key = a.to_dict()["device_seed"]
    assert isinstance(key, int) and 0 <= key < 1 << 64
    twin = amb.Ambience.from_dict(a.to_dict())
    assert twin.to_dict()["device_seed"] == key
    got = twin.load_ambience(normalize=False)
    check_draws(got.reshape(-1), restated_normals(key, TAG_GAUSSIAN, 0, channels * total), 1.0, "python gaussian (err / tolerance)",
                ("seedless", channels, total))
    assert_bits_equal(a.load_ambience(normalize=False), got, "an Ambience and the twin made from its dictionary")
    other = amb.Ambience(channels, total / sr, alias="g", noise="gaussian", sample_rate=sr, rng="device")
    assert other.to_dict()["device_seed"] != key                    # fresh entropy per object


def run_scene_against_restated_noise():
    """tests/test_hostemu_rng.py's scene with a device-drawn pink ambience, the oracle's noise taken from the restated chain --
    restated draws, float64 irfft, peak normalisation as orc.mix_scene takes it -- and not from a twin Ambience."""
    from audiblelight_amd import core
    from tests.conftest import rel_rms

    rng = np.random.default_rng(5)
    sr, C, L, seed = 8000, 3, 300, 11
    irs = (rng.standard_normal((C, 2, L)) * np.exp(-np.arange(L) / 60.0)).astype(np.float32)
    scene = core.Scene(1.0, core.StaticIRState({"mic000": irs}), sample_rate=sr, ref_db=-60)
    clips = [rng.standard_normal(n).astype(np.float32) for n in (3000, 2500)]
    for i, c in enumerate(clips):
        scene.add_event(core.Event(f"e{i}", c, sr, snr=10.0 + i, scene_start=0.1 + 0.2 * i))
    a = amb.Ambience(C, 1.0, alias="a", noise="pink", ref_db=-55, sample_rate=sr, rng="device", seed=seed)
    scene.add_ambience(a)
    got = scene.generate()["mic000"]
    assert a.audio is None
    shape, inv_sigma = pink_shape(sr)
    noise, _ = float64_noise(*restated_spectrum_draws(seed, C, sr // 2 + 1), shape, sr, inv_sigma)
    noise = noise / (np.max(np.abs(noise), axis=1, keepdims=True) + np.finfo(np.float64).tiny)
    spat = [orc.render_event(orc.peak_normalise_clip(c), irs[:, [i], :].astype(np.float64), 10.0 + i, ref_db=-60, sr=sr)["spatial"]
            for i, c in enumerate(clips)]
    want = orc.mix_scene(spat, [(e.scene_start, e.scene_end) for e in scene.events.values()], 1.0, sr,
                         ambiences=[(noise, -55)], keep_padded=False)["scene"]
    err = rel_rms(got, want)
    print(f"\nscene with restated noise: rel_rms {err:.3g} (bound 1e-4)")
    assert err < 1e-4
