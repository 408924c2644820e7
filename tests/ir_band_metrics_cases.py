"""Scenarios of the octave-band IR metrics (al_ir_band_split, al_ir_band_metrics, acoustics.ir_band_metrics / ir_band_rows, the states'
band_metrics()) and the float64 numpy restatement of the band split (the header comment of al_ir_band_split in
include/audiblelight_hip.h; no reference code computes this).  tests/test_hostemu_ir_band_metrics.py runs them on the host-emulated
kernels, tests/test_gpu_ir_band_metrics.py on the gfx950 build.

THE RESTATEMENT of a band row: g64 = np.convolve(float64(h), phi_b)[half : half + L]: the zero-phase FIR with h taken as 0 outside
the row, cut to the row.

THE BOUND (derived, not tuned; u = 2^-53), on every sample, none excluded:
    |g - g64| <= 2^-24 |g64| + (2 half + 3) u S + 2^-150,     S = sum_j |phi_b[j]| |h[t - j]| = np.convolve(|h|, |phi_b|)[half : half + L].
The device's sum is a chain of 2 half + 1 fused multiply-adds from +0: step k rounds a partial sum no larger than S once, so the chain
is within (2 half + 1) u S of the exact sum to first order; the restatement's own float64 sum takes the remaining 2 u S at the
fraction of its worst case that float64 sums reach in practice (the observed error over the bound is printed; where it is near 1 it
is the rounding to float32 that fills it, which is 2^-24 |g| at the most and, below the normal range, 2^-150 absolutely: the count
of samples that differ from float32(g64) at all is printed beside it).

THE BAND METRICS have no bound of their own: the contract is that (row, b) of al_ir_band_metrics carries the BITS al_ir_metrics gives
for row (row, b) of the tensor al_ir_band_split writes (run_composition), and al_ir_metrics is held against its restatement in
tests/ir_metrics_cases.py.  What the numbers mean is held against a construction (run_meaning): rows whose two ends of the spectrum
decay at different, known rates.
"""
import json
import math
import os

import numpy as np
import pytest

from audiblelight_amd import _hip, acoustics, core, engine, shoebox
from tests import ir_metrics_cases as broadband

FS = 16000.0
U = 2.0 ** -53
WORST = {}
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shoebox_materials.json")
SENTINEL = np.array([0xFFC12345], dtype=np.uint32).view(np.float32)[0]      # a NaN no arithmetic here produces
SENTINEL64 = np.array([0xFFF8DEADBEEF1234], dtype=np.uint64).view(np.float64)[0]
CENTRES = {1: (1000.0,), 3: (250.0, 1000.0, 3000.0), 5: (125.0, 400.0, 1000.0, 2500.0, 6000.0),
           6: (125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0), 8: (63.0, 125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0, 7000.0)}

bits = broadband.bits
same_bits = broadband.same_bits


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def table_of(n_bands, half, fs=FS):
    return shoebox.band_filters(CENTRES[n_bands], fs, half)


def noise_rows(C, N, L, seed):
    """(C, N, L) float32: seeded Gaussian noise under a decay of its own per row, a direct tap a few samples in."""
    rng = np.random.default_rng(seed)
    t = np.arange(L)
    rows = np.empty((C * N, L), dtype=np.float32)
    for i in range(C * N):
        lead = min(L - 1, (3 * i) % 11)
        h = 0.3 * rng.standard_normal(L) * 10.0 ** (-3.0 * t / ((0.02 + 0.01 * i) * FS))
        h[lead] = 1.5 if i % 2 == 0 else -1.25
        rows[i] = h
    return rows.reshape(C, N, L)


# ----------------------------------------------------------------------------- the restatement and its bound
def restate_split(rows, table, half):
    """(g64, bound), each (C N, B, L) float64."""
    C, N, L = rows.shape
    flat = rows.reshape(-1, L).astype(np.float64)
    g64 = np.empty((C * N, len(table), L))
    bound = np.empty_like(g64)
    for i, h in enumerate(flat):
        for b, phi in enumerate(table):
            g64[i, b] = np.convolve(h, phi)[half: half + L]
            S = np.convolve(np.abs(h), np.abs(phi))[half: half + L]
            bound[i, b] = 2.0 ** -24 * np.abs(g64[i, b]) + (2 * half + 3) * U * S + 2.0 ** -150
    return g64, bound


def assert_split(g, rows, table, half, what):
    g64, bound = restate_split(rows, table, half)
    assert g.shape == g64.shape, (what, g.shape, g64.shape)
    assert np.all(np.isfinite(g)), f"{what}: a band row is not finite"
    err = np.abs(g.astype(np.float64) - g64)
    over = err > bound
    assert not np.any(over), f"{what}: {np.count_nonzero(over)} samples over the bound, first at {np.argwhere(over)[0].tolist()}"
    frac = float(np.max(err / bound))
    WORST["split"] = max(WORST.get("split", 0.0), frac)
    off = int(np.count_nonzero(bits32(g) != bits32(g64.astype(np.float32))))
    print(f"\n[band split] {what}: worst error / bound {frac:.3g}; {off} of {g.size} samples are not float32(g64)")
    return bound


# ----------------------------------------------------------------------------- the device
def lay_out(r, rows, pitch=None, stride_c=None, offset=0):
    """The tensor at the given pitch, stride and element offset in a buffer whose every other float is a NaN: (buffer, stride_c, pitch)."""
    C, N, L = rows.shape
    pitch = (L + 3) // 4 * 4 if pitch is None else pitch
    stride_c = N * pitch if stride_c is None else stride_c
    host = np.full(offset + C * stride_c + 8, np.nan, dtype=np.float32)
    for c in range(C):
        for n in range(N):
            at = offset + c * stride_c + n * pitch
            host[at: at + L] = rows[c, n]
    return r.mem.upload(host), stride_c, pitch


def run_split(r, rows, table, half, pitch=None, stride_c=None, offset=0, out_pitch=None):
    """al_ir_band_split into a buffer filled with a sentinel, eight sentinels in front of `out` and eight behind: the guards intact,
    no output word left at the sentinel, pad bits 0; returns (C N, B, L) float32."""
    C, N, L = rows.shape
    B = len(table)
    buf, stride_c, pitch = lay_out(r, rows, pitch, stride_c, offset)
    out_pitch = (L + 3) // 4 * 4 if out_pitch is None else out_pitch
    n_out = C * N * B * out_pitch
    out = r.mem.upload(np.full(n_out + 16, SENTINEL, dtype=np.float32))
    filters = r.mem.upload(np.ascontiguousarray(table, dtype=np.float64).reshape(-1))
    r.lib.call("al_ir_band_split", r.mem.ptr(buf) + 4 * offset, C, N, stride_c, pitch, L, r.mem.ptr(filters), B, half, r.mem.ptr(out) + 32,
               out_pitch, r.mem.stream())
    got = np.array(r.mem.download(out))[: n_out + 16]
    guard = bits32(SENTINEL)
    assert np.all(bits32(got[:8]) == guard) and np.all(bits32(got[8 + n_out:]) == guard), "a sentinel beside out was overwritten"
    g = got[8: 8 + n_out].reshape(C * N, B, out_pitch)
    assert not np.any(bits32(g) == guard), f"{np.count_nonzero(bits32(g) == guard)} output words were not written"
    assert not np.any(bits32(g[:, :, L:])), "a pad word is not +0"
    return np.ascontiguousarray(g[:, :, :L])


# (ir_len, half, n_bands, (C, N)): every ir_len around a lane's 16 outputs, a tap chunk and the tile; half below, at and past one tap
# chunk and, at 4096, a reach far longer than the row (the three segment sizes of the kernel); every band count; both pair shapes
SPLIT_SHAPES = ((1, 1, 1, (1, 1)), (5, 16, 3, (3, 5)), (5, 4096, 1, (1, 1)), (255, 16, 6, (1, 1)), (256, 1, 8, (1, 1)),
                (257, 300, 3, (1, 1)), (700, 4096, 3, (1, 1)), (1023, 16, 1, (3, 5)), (1024, 300, 6, (1, 1)), (1025, 16, 8, (1, 1)),
                (1025, 1, 3, (3, 5)), (2100, 300, 6, (1, 1)), (2100, 16, 3, (3, 5)))


def run_split_shape(r, ir_len, half, n_bands, pair):
    rows = noise_rows(*pair, ir_len, 1000 + ir_len + half)
    table = table_of(n_bands, half)
    g = run_split(r, rows, table, half)
    assert_split(g, rows, table, half, f"ir_len {ir_len}, half {half}, {n_bands} bands, {pair[0]} x {pair[1]}")


def run_split_layouts(r):
    """A larger pitch (NaN in the input pads: never read), a larger stride_c, an odd pitch at a base off 16-byte alignment, larger
    out_pitch (a few pad words; a whole tile of pads): the bits of the tight layout."""
    L, half, B = 1023, 16, 3
    rows = noise_rows(3, 5, L, 77)
    table = table_of(B, half)
    g = run_split(r, rows, table, half)
    assert_split(g, rows, table, half, "layouts, tight")
    tight = (L + 3) // 4 * 4
    for name, kw in (("a larger pitch", dict(pitch=tight + 8)), ("a larger stride_c", dict(stride_c=5 * tight + 16)),
                     ("an odd pitch at an unaligned base", dict(pitch=tight + 3, stride_c=5 * (tight + 3) + 5, offset=1)),
                     ("out_pitch with pad words", dict(out_pitch=tight + 8)), ("out_pitch with a tile of pads", dict(out_pitch=tight + 1028)),
                     ("a second run", dict())):
        g2 = run_split(r, rows, table, half, **kw)
        assert np.array_equal(bits32(g2), bits32(g)), f"{name}: the band rows differ from the tight layout's"


def run_exact(r):
    """The unit impulse as a table gives the row back; a doubled table the doubled band rows; the bands of band_filters sum to the row."""
    L, half = 1100, 16
    rows = noise_rows(1, 2, L, 5)
    delta = np.zeros((2, 2 * half + 1))
    delta[:, half] = 1.0
    g = run_split(r, rows, delta, half)
    flat = rows.reshape(2, L)
    for b in range(2):
        keep = flat != 0.0
        assert np.array_equal(bits32(g[:, b][keep]), bits32(flat[keep])), f"the impulse in band {b} does not return the row"
    table = table_of(3, half)
    g1, g2 = run_split(r, rows, table, half), run_split(r, rows, 2.0 * table, half)
    assert np.array_equal(bits32(g2), bits32(np.float32(2.0) * g1)), "a doubled table does not give doubled band rows"
    for B, hf in ((6, 16), (3, 300)):
        table = table_of(B, hf)
        g = run_split(r, rows, table, hf)
        bound = assert_split(g, rows, table, hf, f"partition of unity, {B} bands, half {hf}")
        reach = np.stack([np.convolve(np.abs(h.astype(np.float64)), np.ones(2 * hf + 1))[hf: hf + L] for h in flat])
        err = np.abs(g.astype(np.float64).sum(axis=1) - flat.astype(np.float64))
        assert np.all(err <= bound.sum(axis=1) + 1e-15 * reach), f"{B} bands, half {hf}: the band rows do not sum to the row"


# ----------------------------------------------------------------------------- composition
def band_metrics_call(r, buf, C, N, stride_c, pitch, L, filters, B, half, rows_in_workspace, offset=0, fs=FS):
    """al_ir_band_metrics with a workspace of exactly `rows_in_workspace` rows' share and a guard behind it: (table (C N B, 16),
    knots (C N B, n_knots))."""
    per_row = r.lib.call("al_ir_band_metrics_workspace_bytes", B, L)
    assert per_row > 0 and per_row % 16 == 0
    nbytes = rows_in_workspace * per_row
    ws = r.mem.upload(np.full(nbytes // 8 + 8, SENTINEL64, dtype=np.float64))
    k = acoustics.n_knots_of(L)
    out = r.mem.upload(np.full(C * N * B * 16, SENTINEL64, dtype=np.float64))
    knots = r.mem.upload(np.full(C * N * B * k, SENTINEL64, dtype=np.float64))
    r.lib.call("al_ir_band_metrics", r.mem.ptr(buf) + 4 * offset, C, N, stride_c, pitch, L, fs, r.mem.ptr(filters), B, half, r.mem.ptr(ws),
               nbytes, r.mem.ptr(out), r.mem.ptr(knots), r.mem.stream())
    guard = np.array(r.mem.download(ws))[nbytes // 8: nbytes // 8 + 8]
    assert np.all(bits(guard) == bits(SENTINEL64)), "the guard behind the workspace was overwritten"
    table = np.array(r.mem.download(out))[: C * N * B * 16].reshape(C * N * B, 16)
    curve = np.array(r.mem.download(knots))[: C * N * B * k].reshape(C * N * B, k)
    assert not np.any(bits(table) == bits(SENTINEL64)) and not np.any(bits(curve) == bits(SENTINEL64)), "a word of the tables was not written"
    return table, curve


def composed(r, rows, table, half, fs=FS):
    """al_ir_metrics over what al_ir_band_split writes, as a tensor of (C N, B) rows: the definition of the band metrics."""
    C, N, L = rows.shape
    g = run_split(r, rows, table, half)
    return broadband.run_table(r, g.reshape(C * N, len(table), L), fs=fs)


def run_composition(r):
    C, N, L, half, B = 3, 5, 1500, 16, 3
    rows = noise_rows(C, N, L, 31)
    table = table_of(B, half)
    want, want_knots = composed(r, rows, table, half)
    assert np.all(want[:, 0] == 0.0) and np.all(np.isfinite(want[:, 1:4]))
    filters = r.mem.upload(table.reshape(-1))
    buf, stride_c, pitch = lay_out(r, rows)
    for in_ws in (1, 4, C * N, C * N, C * N + 3):      # one row per pass; a last pass part full; all rows, twice; room to spare
        got, got_knots = band_metrics_call(r, buf, C, N, stride_c, pitch, L, filters, B, half, in_ws)
        same_bits(got, want, f"workspace of {in_ws} rows: table")
        same_bits(got_knots, want_knots, f"workspace of {in_ws} rows: knots")
    tight = (L + 3) // 4 * 4
    buf2, stride2, pitch2 = lay_out(r, rows, pitch=tight + 3, stride_c=N * (tight + 3) + 5, offset=1)
    got, got_knots = band_metrics_call(r, buf2, C, N, stride2, pitch2, L, filters, B, half, 4, offset=1)
    same_bits(got, want, "an odd pitch, a larger stride_c, an unaligned base: table")
    same_bits(got_knots, want_knots, "an odd pitch, a larger stride_c, an unaligned base: knots")
    for c, n in ((0, 0), (1, 3), (2, 4)):
        one = np.ascontiguousarray(rows[c: c + 1, n: n + 1])
        b1, s1, p1 = lay_out(r, one)
        got, got_knots = band_metrics_call(r, b1, 1, 1, s1, p1, L, filters, B, half, 1)
        at = (c * N + n) * B
        same_bits(got, want[at: at + B], f"row ({c}, {n}) alone: table")
        same_bits(got_knots, want_knots[at: at + B], f"row ({c}, {n}) alone: knots")


def run_non_finite(r):
    """One NaN in one row: bad > 0 and NaN elsewhere in every band of that row; the other rows keep their bits."""
    C, N, L, half, B = 2, 3, 1500, 16, 3
    rows = noise_rows(C, N, L, 32)
    table = table_of(B, half)
    filters = r.mem.upload(table.reshape(-1))
    buf, stride_c, pitch = lay_out(r, rows)
    clean, clean_knots = band_metrics_call(r, buf, C, N, stride_c, pitch, L, filters, B, half, 4)
    dirty = rows.copy()
    dirty[1, 0, 700] = np.nan
    buf, stride_c, pitch = lay_out(r, dirty)
    got, got_knots = band_metrics_call(r, buf, C, N, stride_c, pitch, L, filters, B, half, 4)
    hit = np.arange(3 * B, 4 * B)
    others = np.setdiff1d(np.arange(C * N * B), hit)
    assert np.all(got[hit, 0] == 2 * half + 1), got[hit, 0]      # the NaN reaches the 2 half + 1 outputs around it in every band
    assert np.all(np.isnan(got[hit, 1:]))
    same_bits(got[others], clean[others], "the rows beside the NaN: table")
    same_bits(got_knots[others], clean_knots[others], "the rows beside the NaN: knots")


# ----------------------------------------------------------------------------- what the numbers mean
def two_rate_rows(L=9000, fs=FS, seed=0):
    """(1, 2, L).  Row A: noise below 200 Hz decaying at 0.30 s plus noise above 3.5 kHz decaying at 0.12 s plus a direct tap; row B: the
    two times swapped.  The noises are cut in the frequency domain before the decay is laid over them.
    THE SEED.  A band 200 Hz wide has about eight independent samples in the 40 ms over which a 0.12 s decay falls 20 dB, so the
    realisation alone moves the bottom band's T20 by 10 to 20 %.  Seeds 0 .. 11 were put through the numpy restatement (np.convolve
    with the half = 256 table, then ir_metrics_cases.restate_row: no device code), worst deviation from the nominal four times 0.109,
    0.174, 0.153, 0.417, 0.124, 0.933, 0.249, 0.163, 0.184, 0.186, 0.118, 0.150; seed 0 is the closest: 0.333 / 0.113 s and 0.111 / 0.307 s."""
    rng = np.random.default_rng(seed)
    n_pad = 2 * L
    f = np.fft.rfftfreq(n_pad, 1.0 / fs)
    t = np.arange(L)

    def noise(keep):
        spec = np.fft.rfft(rng.standard_normal(n_pad))
        x = np.fft.irfft(np.where(keep, spec, 0.0), n_pad)[L // 2: L // 2 + L]
        return x / np.sqrt(np.mean(x * x))

    low, high = noise(f < 200.0), noise(f > 3500.0)
    rows = []
    for rt_low, rt_high in ((0.30, 0.12), (0.12, 0.30)):
        h = 0.2 * low * 10.0 ** (-3.0 * t / (rt_low * fs)) + 0.2 * high * 10.0 ** (-3.0 * t / (rt_high * fs))
        h[0] += 1.0
        rows.append(h)
    return np.stack(rows).astype(np.float32).reshape(1, 2, L)


def run_meaning(r):
    """The T20 of the bottom and the top band of the two-rate rows, at 16 kHz, centres (250, 1000, 3000), half 256: each within 20 % of
    the rate its end of the spectrum was given, the slow end 1.5 times the fast one at least.  (The broadband T20, one number for both
    ends, is printed, not asserted.)"""
    rows = two_rate_rows()
    m = acoustics.ir_band_metrics(rows, FS, shoebox.ShoeboxBands(centres=CENTRES[3], half=256), renderer=r)
    wide = acoustics.ir_metrics(rows, FS, renderer=r)
    t20 = m.t20[0]
    print(f"\n[band metrics] two-rate rows: T20 bottom / top band: row A {t20[0, 0]:.3f} / {t20[0, 2]:.3f} s (asked for 0.30 / 0.12), "
          f"row B {t20[1, 0]:.3f} / {t20[1, 2]:.3f} s (0.12 / 0.30); broadband T20 {wide.t20[0, 0]:.3f} and {wide.t20[0, 1]:.3f} s")
    assert np.all(m.bad == 0) and np.all(np.isfinite(t20[:, [0, 2]]))
    assert t20[0, 0] > 1.5 * t20[0, 2] and t20[1, 2] > 1.5 * t20[1, 0]
    for got, nominal in ((t20[0, 0], 0.30), (t20[0, 2], 0.12), (t20[1, 0], 0.12), (t20[1, 2], 0.30)):
        assert abs(got - nominal) <= 0.2 * nominal, (got, nominal)


# ----------------------------------------------------------------------------- schedule independence (the gfx950 builds)
def run_shake_rows(r):
    """What the schedule-perturbed builds must reproduce bit for bit: band rows (held to the split's bound first) and the tables and
    knots of one call with half = 300 (more than one tap chunk), five bands and two passes."""
    C, N, L, half, B = 2, 3, 2100, 300, 5
    rows = noise_rows(C, N, L, 41)
    table = table_of(B, half)
    g = run_split(r, rows, table, half)
    assert_split(g, rows, table, half, "schedule independence")
    filters = r.mem.upload(table.reshape(-1))
    buf, stride_c, pitch = lay_out(r, rows)
    got, knots = band_metrics_call(r, buf, C, N, stride_c, pitch, L, filters, B, half, 3)
    return {"band rows": g.astype(np.float64), "table": got, "knots": knots}


# ----------------------------------------------------------------------------- the layers
def run_abi_refusals(r):
    C, N, L, half, B = 2, 3, 300, 16, 3
    rows = noise_rows(C, N, L, 9)
    table = table_of(B, half)
    buf, stride_c, pitch = lay_out(r, rows)
    filters = r.mem.upload(table.reshape(-1))
    n_out = C * N * B * pitch
    out = r.mem.upload(np.full(n_out, SENTINEL, dtype=np.float32))
    per_row = r.lib.call("al_ir_band_metrics_workspace_bytes", B, L)
    ws = r.mem.empty(C * N * per_row // 8 + 2, np.float64)
    tab = r.mem.upload(np.full(C * N * B * 16, SENTINEL64, dtype=np.float64))
    good = dict(irs=r.mem.ptr(buf), C=C, N=N, stride_c=stride_c, pitch=pitch, L=L, fs=FS, filters=r.mem.ptr(filters), B=B, half=half,
                out=r.mem.ptr(out), out_pitch=pitch, ws=r.mem.ptr(ws), nbytes=C * N * per_row, tab=r.mem.ptr(tab))

    def split(**kw):
        a = {**good, **kw}
        return r.lib._al_ir_band_split(a["irs"], a["C"], a["N"], a["stride_c"], a["pitch"], a["L"], a["filters"], a["B"], a["half"], a["out"],
                                       a["out_pitch"], r.mem.stream())

    def metrics(**kw):
        a = {**good, **kw}
        return r.lib._al_ir_band_metrics(a["irs"], a["C"], a["N"], a["stride_c"], a["pitch"], a["L"], a["fs"], a["filters"], a["B"], a["half"],
                                         a["ws"], a["nbytes"], a["tab"], None, r.mem.stream())

    extent = "n_capsules, n_sources and ir_len must be >= 1"
    shared = ((dict(irs=None), "irs must not be null"), (dict(C=0), extent), (dict(N=0), extent), (dict(L=0), extent), (dict(N=-1), extent),
              (dict(pitch=L - 1), "pitch < ir_len"), (dict(stride_c=N * pitch - 1), "stride_c < n_sources * pitch"),
              (dict(C=1 << 16, N=1 << 15, stride_c=(1 << 15) * pitch), "more than 2^31 - 1 rows"),
              (dict(B=0), "n_bands must be in 1 .. 8"), (dict(B=9), "n_bands must be in 1 .. 8"),
              (dict(half=0), "half must be in 1 .. 4096"), (dict(half=4097), "half must be in 1 .. 4096"),
              (dict(filters=None), "filters must not be null"))
    rate = "fs must be finite and positive"
    for call, entry, own in (
            (split, "al_ir_band_split",
             ((dict(out=None), "out must not be null"), (dict(out=good["out"] + 4), "out must be 16-byte aligned"),
              (dict(out_pitch=296), "out_pitch < ir_len"), (dict(out_pitch=302), "out_pitch must be a multiple of 4"),
              (dict(C=1 << 15, N=1 << 15, L=3 * 1024, pitch=3 * 1024, out_pitch=3 * 1024, stride_c=(1 << 15) * 3 * 1024),
               "more than 2^31 - 1 (row, 1024-sample tile of out_pitch) pairs"))),
            (metrics, "al_ir_band_metrics",
             ((dict(tab=None), "out and workspace must not be null"), (dict(ws=None), "out and workspace must not be null"),
              (dict(fs=0.0), rate), (dict(fs=-1.0), rate), (dict(fs=float("nan")), rate), (dict(fs=float("inf")), rate),
              (dict(ws=good["ws"] + 8), "workspace must be 16-byte aligned"),
              (dict(nbytes=per_row - 1), "workspace_bytes < al_ir_band_metrics_workspace_bytes(...)")))):
        for kw, text in shared + own:
            assert call(**kw) == _hip.AL_E_BADARG, (entry, kw)
            assert r.lib.last_error().startswith(entry + ": ") and text in r.lib.last_error(), (entry, kw, r.lib.last_error())
    assert np.all(bits32(np.array(r.mem.download(out))[:n_out]) == bits32(SENTINEL)), "a refused al_ir_band_split wrote to out"
    assert np.all(bits(np.array(r.mem.download(tab))[: C * N * B * 16]) == bits(SENTINEL64)), "a refused al_ir_band_metrics wrote to out"
    for n_bands, ir_len in ((0, L), (9, L), (B, 0)):
        assert r.lib.call("al_ir_band_metrics_workspace_bytes", n_bands, ir_len) < 0
    assert split() == 0 and metrics() == 0


def run_python_errors(r):
    good = noise_rows(2, 3, 300, 9)
    for bad in ("octaves", 3, dict(centres=(500.0, 250.0)), dict(centres=("a", "b")), dict(half=0), dict(half=5000), dict(centres=()),
                shoebox.ShoeboxBands(centres=tuple(100.0 * (i + 1) for i in range(9))),
                dict(centres=(1000.0, 8000.0)), dict(centres=(1000.0, 9000.0))):        # the last two: at and above fs / 2
        for fn in (acoustics.ir_band_metrics, acoustics.ir_band_rows):
            with pytest.raises(ValueError):
                fn(good, FS, bad, renderer=r)
    for bad in (good[0], good[0, 0], np.zeros((2, 0, 300), np.float32), np.zeros((0, 3, 300), np.float32), np.zeros((2, 3, 0), np.float32),
                good.astype(np.int32)):
        for fn in (acoustics.ir_band_metrics, acoustics.ir_band_rows):
            with pytest.raises(ValueError):
                fn(bad, FS, renderer=r)
    for rate in (0, float("nan"), None, "16000", True):
        with pytest.raises(ValueError):
            acoustics.ir_band_metrics(good, rate, renderer=r)
    for cap in (-1, 1.5, True, None, "1G"):
        with pytest.raises(ValueError):
            acoustics.ir_band_metrics(good, FS, renderer=r, workspace_cap=cap)
    other = engine.Renderer(lib=r.lib, memory=type(r.mem)())
    theirs = shoebox.DeviceIRTensor(other, other.mem.upload(good.reshape(-1)), (3 * 300, 300), good.shape)
    for fn in (acoustics.ir_band_metrics, acoustics.ir_band_rows):
        with pytest.raises(ValueError, match="another renderer"):
            fn(theirs, FS, renderer=r)
    static = core.StaticIRState({"mic": good})
    with pytest.raises(ValueError):
        static.band_metrics(renderer=r)        # no sample rate anywhere
    with pytest.raises(KeyError):
        static.band_metrics("nobody", sample_rate=FS, renderer=r)
    m = acoustics.ir_band_metrics(good, FS, dict(centres=CENTRES[3], half=16), renderer=r)
    for b in (-1, 3, 1.0, True):
        with pytest.raises(IndexError):
            m.band(b)


def run_python_layer(r):
    """ir_band_metrics and ir_band_rows against the ABI: the rows are al_ir_band_split's, the tables the composition's; band(b) is the
    IRMetrics of band b; a workspace_cap of 0 (one row per pass) gives the same bits; the dictionary round trip with NaN present."""
    C, N, L, half, B = 2, 3, 1500, 16, 3
    rows = noise_rows(C, N, L, 33)
    rows[1, 1, 200] = np.inf
    bands = shoebox.ShoeboxBands(centres=CENTRES[B], half=half)
    table = shoebox.band_filters(bands.centres, FS, half)
    with np.errstate(invalid="ignore"):
        g = run_split(r, rows, table, half)
        want, want_knots = broadband.run_table(r, g.reshape(C * N, B, L))
    got_rows = acoustics.ir_band_rows(rows, FS, bands, renderer=r)
    assert got_rows.shape == (C, N, B, L) and got_rows.dtype == np.float32
    assert np.array_equal(bits32(got_rows.reshape(C * N, B, L)), bits32(g))
    m = acoustics.ir_band_metrics(rows, FS, bands.to_dict(), renderer=r, edc=True)
    assert m.centres == CENTRES[B] and m.half == half and m.sample_rate == FS and m.t30.shape == (C, N, B)
    assert m.edc_knots.shape == (C, N, B, acoustics.n_knots_of(L))
    same_bits(m.table().reshape(-1, 16), want, "ir_band_metrics against the composition: table")
    same_bits(m.edc_knots.reshape(C * N * B, -1), want_knots, "ir_band_metrics against the composition: knots")
    one = acoustics.ir_band_metrics(rows.astype(np.float64), FS, bands, renderer=r, edc=False, workspace_cap=0)
    assert one.edc_knots is None
    same_bits(one.table(), m.table(), "a float64 array, one row per pass, no knots")
    for b in range(B):
        mb = m.band(b)
        assert isinstance(mb, acoustics.IRMetrics) and mb.sample_rate == FS
        same_bits(mb.table(), m.table()[:, :, b], f"band({b})")
        same_bits(mb.edc_knots, m.edc_knots[:, :, b], f"band({b}): knots")
    assert np.isnan(m.t30).any() and (m.bad[1, 1] > 0).all()
    for src in (m, one):
        d = src.to_dict()
        text = json.dumps(d, allow_nan=False)
        assert all(v is None or type(v) is int for name in acoustics.INTEGER_COLUMNS for cap in d[name] for row in cap for v in row)
        back = acoustics.IRBandMetrics.from_dict(json.loads(text))
        assert back.centres == src.centres and back.half == src.half and back.sample_rate == src.sample_rate
        assert (back.edc_knots is None) == (src.edc_knots is None)
        for name in acoustics.COLUMNS + (("edc_knots",) if src.edc_knots is not None else ()):
            a, b2 = getattr(src, name), getattr(back, name)
            fin = np.isfinite(a)
            assert a.shape == b2.shape and np.array_equal(a[fin], b2[fin]) and np.all(np.isnan(b2[~fin])), name


def materials_state(r, table_path):
    st = core.ShoeboxIRState((5.2, 4.1, 2.7), materials=["Carpet", "Default", "Default", "Default", "Default", "Default"],
                             material_table=shoebox.load_materials(table_path), bands=shoebox.ShoeboxBands(half=64), ir_len=3000,
                             sample_rate=16000, max_order=6, renderer=r, tail=shoebox.ShoeboxTail(rt60=None, seed=0xC0FFEE1234567))
    st.add_microphone("pair", [[2.1, 1.9, 1.3], [2.3, 1.9, 1.3]])
    st.add_microphone("single", [[1.0, 3.0, 1.1]])
    st.add_emitters([[3.9, 3.0, 1.6], [0.9, 0.8, 1.0], [2.6, 2.2, 2.0]])
    st.simulate()
    return st


def run_state(r, table_path, monkeypatch):
    """A room with materials: band_metrics() comes back in the state's own bands, equals ir_band_metrics on the tensors bit for bit,
    round-trips under strict JSON, leaves to_dict() alone, and neither downloads nor uploads a tensor; a StaticIRState over the
    downloaded tensor gives the same bits."""
    st = materials_state(r, table_path)
    before = json.dumps(st.to_dict(), sort_keys=True)
    t = st.irs["pair"]
    assert isinstance(t, shoebox.DeviceIRTensor) and t._host is None
    B = len(st.bands.centres)

    def no_upload(*a, **k):
        raise AssertionError("band_metrics() uploaded a tensor")

    with monkeypatch.context() as mp:
        mp.setattr(engine.Renderer, "upload_irs", no_upload)
        by_state = st.band_metrics(edc=True)
        direct = acoustics.ir_band_metrics(t, 16000, st.bands, edc=True)
        assert list(st.band_metrics("single")) == ["single"] and st.band_metrics("single")["single"].edc_knots is None
        other = st.band_metrics("single", bands=dict(centres=CENTRES[3], half=16))["single"]
    assert all(v._host is None for v in st.irs.values()), "band_metrics() downloaded a tensor"
    assert list(by_state) == ["pair", "single"]
    m = by_state["pair"]
    assert m.centres == tuple(st.bands.centres) and m.half == st.bands.half == 64 and m.sample_rate == 16000.0
    assert m.t30.shape == (2, 3, B) and by_state["single"].t30.shape == (1, 3, B) and m.edc_knots.shape == (2, 3, B, acoustics.n_knots_of(3000))
    assert other.centres == CENTRES[3] and other.half == 16 and other.t30.shape == (1, 3, 3)
    same_bits(m.table(), direct.table(), "state.band_metrics() against ir_band_metrics")
    same_bits(m.edc_knots, direct.edc_knots, "state.band_metrics() against ir_band_metrics: knots")
    assert np.all(m.bad == 0) and np.all(np.isfinite(m.energy)) and np.all(m.energy > 0.0)
    text = json.dumps(m.to_dict(), allow_nan=False)
    back = acoustics.IRBandMetrics.from_dict(json.loads(text))
    fin = np.isfinite(m.table())
    assert np.array_equal(back.table()[fin], m.table()[fin]) and np.all(np.isnan(back.table()[~fin]))
    assert json.dumps(st.to_dict(), sort_keys=True) == before and "t30" not in before
    host = np.asarray(t)
    static = core.StaticIRState({"pair": host}, metadata={"sample_rate": 16000})
    got = static.band_metrics(bands=st.bands, edc=True, renderer=r)["pair"]
    same_bits(got.table(), m.table(), "StaticIRState.band_metrics()")
    same_bits(got.edc_knots, m.edc_knots, "StaticIRState.band_metrics(): knots")
    assert "t30" not in json.dumps(static.to_dict())


def run_formulas():
    """sabine_rt60_bands / eyring_rt60_bands: a column equals the broadband formula of that column; air shortens by the 8 m V term."""
    room = (6.0, 5.0, 3.0)
    betas = np.array([[0.9, 0.8], [0.9, 0.8], [0.85, 0.7], [0.85, 0.7], [0.95, 0.6], [0.7, 0.6]])
    sab, eyr = acoustics.sabine_rt60_bands(room, betas), acoustics.eyring_rt60_bands(room, betas)
    assert sab.shape == eyr.shape == (2,)
    for b in range(2):
        assert sab[b] == pytest.approx(acoustics.sabine_rt60(room, betas[:, b]), rel=1e-14)
        assert eyr[b] == pytest.approx(acoustics.eyring_rt60(room, betas[:, b]), rel=1e-14)
    V, c, m = 90.0, 343.0, np.array([0.0, 0.002])
    with_air = acoustics.sabine_rt60_bands(room, betas, air=m)
    assert with_air[0] == sab[0] and with_air[1] < sab[1]
    k = 24.0 * math.log(10.0) * V / c
    assert with_air[1] == pytest.approx(k / (k / sab[1] + 8.0 * m[1] * V), rel=1e-13)
    assert acoustics.eyring_rt60_bands(room, betas, air=0.002)[1] == pytest.approx(k / (k / eyr[1] + 8.0 * 0.002 * V), rel=1e-13)
    assert np.isposinf(acoustics.sabine_rt60_bands(room, np.ones((6, 1)))[0]) and acoustics.eyring_rt60_bands(room, np.zeros((6, 1)))[0] == 0.0
    assert np.isfinite(acoustics.sabine_rt60_bands(room, np.ones((6, 1)), air=0.001)[0])      # rigid walls: the air alone
    for bad in (np.ones(6), np.ones((5, 2))):
        with pytest.raises(ValueError):
            acoustics.sabine_rt60_bands(room, bad)
    with pytest.raises(ValueError):
        acoustics.eyring_rt60_bands(room, betas, air=[0.1, 0.2, 0.3])
