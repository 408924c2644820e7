"""Scenarios of the channel-pair IR metrics (al_ir_pair_metrics, acoustics.ir_pair_metrics / ir_pair_band_metrics, the states'
pair_metrics()) and the float64 numpy restatement of their definition (the header comment of al_ir_pair_metrics in
include/audiblelight_hip.h; no reference code computes this).  tests/test_hostemu_ir_pair_metrics.py runs them on the host-emulated
kernels, tests/test_gpu_ir_pair_metrics.py on the gfx950 build.

THE RESTATEMENT (restate_line).  t0 of a row is the first index of its largest |h| (as al_ir_metrics defines it, found here in numpy),
T0 the smaller of the pair's.  Every product x[t] y[t + j] of two float32 is exact in float64; r_W[j] is the sum of the window's
products in extended precision, added t ascending (at most |W| 2^-64 sum |x y| from the exact sum) and rounded once to float64; the
energies are math.fsum (the exact sum, rounded once).  Everything else is the definition, literally.

THE BOUND (derived from the summation order of csrc/al_irmetrics.h, third part; not tuned).  u = 2^-53.
  r_W[j].  The device adds the products of a tile in one chain of at most 1024 fused multiply-adds from +0 (the products are exact, so
  a step is one rounding of a partial sum no larger than S = sum |x[t]| |y[t + j]|), then the n_tiles tile partials in a chain from +0;
  the restatement's extended sum costs ceil(L / 2048) u S and its rounding one more:
      |r - r64| <= DEPTH u S,   DEPTH = 1024 + n_tiles + 1 + ceil(L / 2048).
  r_A = r_E + r_L is one more rounding on either side:  bound_A = bound_E + bound_L + 2 u |r_A|.
  exx_W, eyy_W: the same chain over terms >= 0, so relatively  g = (1024 + n_tiles + 1 (the addition of A) + 1 (fsum)) u.
  peak = r / sqrt(exx eyy): the product carries 2 g + u, the square root halves it and rounds (taken as 2 u on the device, u here),
  the quotient rounds once on either side:  |d peak| <= bound_r / sqrt(exx eyy) + |peak| (g + 8 u).
  ild_db = 10 log10(exx / eyy): as the levels of tests/ir_metrics_cases.py,  (10 / ln 10)(2 g + u) + 6 u |ild_db|  (dB, absolute).
  bad, t0, lag: exact.

THE CONDITION ON THE INPUTS (asserted on the restatement alone, before the device is asked): in every window that has a peak, the
largest |r_W| less its bound exceeds every other |r_W[j]| plus its bound, so the device, within the bound, finds the same lag.
"""
import json
import math

import numpy as np
import pytest

from audiblelight_amd import _hip, acoustics, core, engine, shoebox
from tests import ir_metrics_cases as broadband

FS = 16000.0
TILE = 1024                                # samples of a workgroup tile (csrc/al_irmetrics.h IRP_TILE)
U = 2.0 ** -53
DB = 10.0 / math.log(10.0)
COLS = acoustics.PAIR_COLUMNS
N_COLS = len(COLS)
AT = {name: i for i, name in enumerate(COLS)}
EXACT_COLS = ("bad", "t0", "lag_e", "lag_l", "lag_a")
ABSOLUTE_COLS = tuple(f"{name}_{w}" for w in "ela" for name in ("peak", "ild_db"))
LENGTHS = (1, 5, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2100, 3000)
LAGS = (0, 1, 48, 63, 64, 65, 300, 1024)
RATES = (1000.0, 16000.0)                  # w_80 = 80, below a tile, and 1280, above one
SENTINEL64 = np.array([0xFFF8DEADBEEF1234], dtype=np.uint64).view(np.float64)[0]      # a NaN no arithmetic here produces
WORST = {}

bits = broadband.bits
same_bits = broadband.same_bits


def w80_of(fs):
    return int(min(np.rint(0.08 * fs), 2.0 ** 31))


# ----------------------------------------------------------------------------- the restatement
def row_state(h):
    """(bad, energy > 0, t0) of a row as al_ir_metrics defines them."""
    bad = int(np.count_nonzero(~np.isfinite(h)))
    if bad:
        return bad, False, None
    peak = float(np.max(np.abs(h)))
    if peak == 0.0:
        return 0, False, None
    return 0, True, int(np.flatnonzero(np.abs(h) == peak)[0])


_RESTATED = {}


def restate_line(x, y, J, fs):
    """(columns (17,), curve (2, 2 J + 1), bounds (17,), curve bounds (2, 2 J + 1), conditioned) of one (pair, source); computed once
    per input and shared (read-only)."""
    x, y = np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(y, dtype=np.float32)
    key = (x.tobytes(), y.tobytes(), J, fs)
    if key not in _RESTATED:
        out = _restate_line(x.astype(np.float64), y.astype(np.float64), J, fs)
        for a in out[:4]:
            a.flags.writeable = False
        _RESTATED[key] = out
    return _RESTATED[key]


def _restate_line(x, y, J, fs):
    L, n_lags = len(x), 2 * J + 1
    col, bound = np.full(N_COLS, np.nan), np.zeros(N_COLS)
    curve, curve_bound = np.full((2, n_lags), np.nan), np.zeros((2, n_lags))
    (bad_x, live_x, t0_x), (bad_y, live_y, t0_y) = row_state(x), row_state(y)
    if bad_x or bad_y:
        col[0] = bad_x + bad_y
        return col, curve, bound, curve_bound, True
    col[0] = 0.0
    if not (live_x and live_y):
        return col, curve, bound, curve_bound, True
    T0 = min(t0_x, t0_y)
    col[1] = T0
    lo, hi = T0, min(L, T0 + w80_of(fs))
    n_tiles = -(-L // TILE)
    depth = TILE + n_tiles + 1 + -(-L // 2048)
    g = (TILE + n_tiles + 2) * U
    padded = np.zeros(L + 2 * J)
    padded[J: J + L] = y
    shifted = np.lib.stride_tricks.sliding_window_view(padded, n_lags)       # shifted[t, k] = y[t + k - J]
    r, r_bound, exx, eyy = [], [], [], []
    for first, last in ((lo, hi), (hi, L)):
        prod = x[first: last, None] * shifted[first: last]                    # exact
        r.append(prod.astype(np.longdouble).sum(axis=0).astype(np.float64))
        r_bound.append(depth * U * np.abs(prod).sum(axis=0))
        exx.append(math.fsum(x[first: last] ** 2))
        eyy.append(math.fsum(y[first: last] ** 2))
    curve[0], curve[1] = r
    curve_bound[0], curve_bound[1] = r_bound
    r.append(r[0] + r[1])
    r_bound.append(r_bound[0] + r_bound[1] + 2 * U * np.abs(r[2]))
    exx.append(exx[0] + exx[1])
    eyy.append(eyy[0] + eyy[1])
    conditioned = True
    for w, count in enumerate((hi - lo, L - hi, L - lo)):
        at = 2 + 5 * w
        with np.errstate(divide="ignore", invalid="ignore"):
            col[at + 2] = 10.0 * np.log10(np.float64(exx[w]) / np.float64(eyy[w]))
        col[at + 3], col[at + 4] = exx[w], eyy[w]
        bound[at + 3] = bound[at + 4] = g
        if np.isfinite(col[at + 2]):
            bound[at + 2] = DB * (2 * g + U) + 6 * U * abs(col[at + 2])
        den = exx[w] * eyy[w]
        if count > 0 and den != 0.0:
            mag = np.abs(r[w])
            k = int(np.argmax(mag))                                           # the first of the largest
            rivals = np.delete(mag + r_bound[w], k)
            if rivals.size and not mag[k] - r_bound[w][k] > rivals.max():
                conditioned = False
            col[at] = r[w][k] / math.sqrt(den)
            col[at + 1] = k - J
            bound[at] = r_bound[w][k] / math.sqrt(den) + abs(col[at]) * (g + 8 * U)
    return col, curve, bound, curve_bound, conditioned


def restate(rows, pairs, J, fs):
    """Every line of (pairs x sources): (table (P N, 17), curves (P N, 2, n_lags), bounds, curve bounds, conditioned (P N,)); a pair
    outside the capsules is a line of NaN."""
    C, N, L = rows.shape
    got = []
    for a, b in pairs:
        for n in range(N):
            if 0 <= a < C and 0 <= b < C:
                got.append(restate_line(rows[a, n], rows[b, n], J, fs))
            else:
                got.append((np.full(N_COLS, np.nan), np.full((2, 2 * J + 1), np.nan), np.zeros(N_COLS), np.zeros((2, 2 * J + 1)), True))
    return tuple(np.array([g[i] for g in got]) for i in range(5))


def same_kind(got, ref):
    return (np.isnan(got) == np.isnan(ref)) & (np.isposinf(got) == np.isposinf(ref)) & (np.isneginf(got) == np.isneginf(ref))


def assert_parity(table, curves, rows, pairs, J, fs=FS, what=""):
    """All 17 columns and the curves of every line against the restatement."""
    want, want_curves, bound, curve_bound, cond = restate(rows, pairs, J, fs)
    assert np.all(cond), f"{what}: lines {np.flatnonzero(~cond).tolist()} have two lags within the bound of each other: pick another seed"
    assert table.shape == want.shape, (what, table.shape, want.shape)
    for i, name in enumerate(COLS):
        got, ref, b = table[:, i], want[:, i], bound[:, i]
        assert np.all(same_kind(got, ref)), f"{what}: column {name}: {got} against {ref}"
        fin = np.isfinite(ref)
        if name in EXACT_COLS:
            assert np.array_equal(got[fin], ref[fin]), f"{what}: column {name}: {got} against {ref}"
            continue
        limit = 1e-8 if name in ABSOLUTE_COLS else 1e-9
        assert np.all(b[fin] < limit), f"{what}: column {name}: the derived bound {b[fin].max():.3g} is not below {limit:g}"
        err = np.abs(got[fin] - ref[fin]) / (1.0 if name in ABSOLUTE_COLS else np.where(ref[fin] == 0.0, 1.0, np.abs(ref[fin])))
        over = err > b[fin]
        assert not np.any(over), f"{what}: column {name}: error {err[over]} over the bound {b[fin][over]} (lines {np.flatnonzero(fin)[over]})"
        if np.any(b[fin] > 0):
            key = name[:-2] if name[-2:] in ("_e", "_l", "_a") else name
            WORST[key] = max(WORST.get(key, 0.0), float(np.max(err[b[fin] > 0] / b[fin][b[fin] > 0])))
    if curves is not None:
        assert curves.shape == want_curves.shape, (what, curves.shape, want_curves.shape)
        assert np.all(same_kind(curves, want_curves)), f"{what}: the curves' non-finite values"
        fin = np.isfinite(want_curves)
        err = np.abs(curves[fin] - want_curves[fin])
        assert np.all(err <= curve_bound[fin]), f"{what}: curves: worst error / bound {np.max(err / np.maximum(curve_bound[fin], 1e-300)):.3g}"
        if np.any(curve_bound[fin] > 0):
            pos = curve_bound[fin] > 0
            WORST["xcorr"] = max(WORST.get("xcorr", 0.0), float(np.max(err[pos] / curve_bound[fin][pos])))


# ----------------------------------------------------------------------------- inputs
def pair_rows(C, N, L, seed, lead=0):
    """(C, N, L) float32.  Per source one seeded noise under a decay from ``lead`` on; capsule c hears it (2 c + n) mod 5 samples late,
    a little weaker, beside noise of its own, behind silence and one direct tap (the row's largest sample: t0 = lead + delay, cut to
    the row)."""
    rng = np.random.default_rng(seed)
    t = np.arange(L)
    env = np.exp(-np.maximum(t - lead, 0) / max(4.0, L / 5.0))
    rows = np.zeros((C, N, L), dtype=np.float32)
    for n in range(N):
        common = 0.3 * rng.standard_normal(L)
        for c in range(C):
            d = (2 * c + n) % 5
            sig = np.zeros(L)
            if d < L:
                sig[d:] = common[: L - d]
            h = ((1.0 - 0.15 * c) * sig + 0.05 * rng.standard_normal(L)) * env
            at = min(lead + d, L - 1)
            h[:at] = 0.0
            h[at] = 2.0 if (c + n) % 2 == 0 else -1.75
            rows[c, n] = h
    return rows


def delayed_copy(L=3000, D=7, seed=11):
    """(2, 1, L): x is seeded noise under exp(-t / 400); y is x scaled by -0.5 and delayed by D whole samples, exactly."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(L) * np.exp(-np.arange(L) / 400.0)).astype(np.float32)
    y = np.zeros(L, dtype=np.float32)
    y[D:] = np.float32(-0.5) * x[: L - D]
    return np.stack([x, y]).reshape(2, 1, L)


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


def run_pairs(r, rows, pairs, J, fs=FS, pitch=None, stride_c=None, offset=0, curves=True, rows_table=None):
    """al_ir_metrics for the rows table (or ``rows_table``, (C N, 16), in its place), then al_ir_pair_metrics through the C ABI into
    tables filled with a sentinel, eight sentinels in front of each and eight behind, and a guard behind the workspace: the guards
    intact, no word of the tables left at the sentinel.  Returns (table (P N, 17), curves (P N, 2, n_lags) or None)."""
    C, N, L = rows.shape
    mem = r.mem
    buf, stride_c, pitch = lay_out(r, rows, pitch, stride_c, offset)
    irs = mem.ptr(buf) + 4 * offset
    if rows_table is None:
        table_dev, _ = acoustics.metrics_device(r, irs, C, N, stride_c, pitch, L, fs)
    else:
        table_dev = mem.upload(np.ascontiguousarray(rows_table, dtype=np.float64).reshape(-1))
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    P, n_lags = len(pairs), 2 * J + 1
    nbytes = r.lib.call("al_ir_pair_metrics_workspace_bytes", P, N, L, J)
    assert nbytes == P * N * -(-L // TILE) * (2 * n_lags + 4) * 8
    ws = mem.upload(np.full(nbytes // 8 + 8, SENTINEL64, dtype=np.float64))
    n_out, n_xc = P * N * N_COLS, P * N * 2 * n_lags
    out = mem.upload(np.full(n_out + 16, SENTINEL64, dtype=np.float64))
    xc = mem.upload(np.full(n_xc + 16, SENTINEL64, dtype=np.float64)) if curves else None
    r.lib.call("al_ir_pair_metrics", irs, C, N, stride_c, pitch, L, fs, mem.ptr(table_dev), mem.ptr(mem.upload(pairs.reshape(-1))), P, J,
               mem.ptr(ws), nbytes, mem.ptr(out) + 64, mem.ptr(xc) + 64 if curves else None, mem.stream())
    guard = bits(SENTINEL64)
    assert np.all(bits(np.array(mem.download(ws))[nbytes // 8: nbytes // 8 + 8]) == guard), "the guard behind the workspace was overwritten"
    found = []
    for name, dev, n in (("out", out, n_out), ("xcorr", xc, n_xc)):
        if dev is None:
            found.append(None)
            continue
        got = np.array(mem.download(dev))[: n + 16]
        assert np.all(bits(got[:8]) == guard) and np.all(bits(got[8 + n:]) == guard), f"a sentinel beside {name} was overwritten"
        assert not np.any(bits(got[8: 8 + n]) == guard), f"{np.count_nonzero(bits(got[8: 8 + n]) == guard)} words of {name} were not written"
        found.append(got[8: 8 + n].copy())
    return found[0].reshape(P * N, N_COLS), None if found[1] is None else found[1].reshape(P * N, 2, n_lags)


def run_length(r, L):
    """One row length at every max_lag (below, at and past a lane block of 64, past the row) and both window lengths: one pair, two
    sources, against the restatement."""
    rows = pair_rows(2, 2, L, 100 + L)
    for fs in RATES:
        for J in LAGS:
            table, curves = run_pairs(r, rows, [(0, 1)], J, fs)
            assert_parity(table, curves, rows, [(0, 1)], J, fs, f"ir_len {L}, max_lag {J}, fs {fs:g}")


def run_sizes(r):
    """1 x 1 and 3 pairs x 5 sources (a pair in either order, a capsule in two pairs), one and three tiles."""
    for L, J in ((TILE + 1, 65), (2100, 300)):
        for C, N, pairs in ((2, 1, [(0, 1)]), (4, 5, [(0, 1), (2, 3), (3, 1)])):
            rows = pair_rows(C, N, L, 7 * L + C)
            table, curves = run_pairs(r, rows, pairs, J)
            assert_parity(table, curves, rows, pairs, J, FS, f"{len(pairs)} pairs x {N} sources, ir_len {L}, max_lag {J}")


def run_windows(r):
    """T0 on and beside a tile boundary, and T0 + w_80 at L - 1 (a late window of one sample), at L and past L (an empty late window:
    NaN peak and lag, zero energies, NaN level)."""
    for lead in (0, TILE - 1, TILE):
        for fs in RATES:
            rows = pair_rows(2, 1, 2100, 300 + lead, lead=lead)
            table, curves = run_pairs(r, rows, [(0, 1)], 48, fs)
            assert table[0, AT["t0"]] == lead
            assert_parity(table, curves, rows, [(0, 1)], 48, fs, f"T0 {lead}, fs {fs:g}")
    L, fs = 257, 1000.0                                                       # w_80 = 80
    for lead, late in ((L - 1 - 80, 1), (L - 80, 0), (L - 57, 0)):
        rows = pair_rows(2, 1, L, 400 + lead, lead=lead)
        table, curves = run_pairs(r, rows, [(0, 1)], 5, fs)
        assert table[0, AT["t0"]] == lead
        assert_parity(table, curves, rows, [(0, 1)], 5, fs, f"T0 + w_80 = L {lead + 80 - L:+d}")
        if late:
            assert table[0, AT["exx_l"]] == float(rows[0, 0, L - 1]) ** 2 and np.isfinite(table[0, AT["lag_l"]])
        else:
            assert np.isnan(table[0, AT["peak_l"]]) and np.isnan(table[0, AT["lag_l"]]) and np.isnan(table[0, AT["ild_db_l"]])
            assert table[0, AT["exx_l"]] == 0.0 and table[0, AT["eyy_l"]] == 0.0 and not np.any(curves[0, 1])
            same_bits(table[0, 12:], table[0, 2:7], "an empty late window: the whole window is the early one")


def run_layouts(r):
    """A larger pitch (NaN in the pads: never read), a larger stride_c, an odd pitch at a base off 16-byte alignment, a second run,
    the call without curves: the bits of the tight layout.  A pair alone, and a source alone, against the same among many."""
    C, N, L, J = 4, 5, TILE + 1, 65
    pairs = [(0, 1), (2, 3), (3, 1)]
    rows = pair_rows(C, N, L, 77)
    table, curves = run_pairs(r, rows, pairs, J)
    assert_parity(table, curves, rows, pairs, J, FS, "layouts, tight")
    tight = (L + 3) // 4 * 4
    for name, kw in (("a larger pitch", dict(pitch=tight + 8)), ("a larger stride_c", dict(stride_c=N * tight + 16)),
                     ("an odd pitch at an unaligned base", dict(pitch=tight + 3, stride_c=N * (tight + 3) + 5, offset=1)),
                     ("a second run", dict())):
        t2, c2 = run_pairs(r, rows, pairs, J, **kw)
        same_bits(t2, table, f"{name}: table")
        same_bits(c2, curves, f"{name}: curves")
    t3, c3 = run_pairs(r, rows, pairs, J, curves=False)
    assert c3 is None
    same_bits(t3, table, "without curves: table")
    for p, pair in enumerate(pairs):
        t1, c1 = run_pairs(r, rows, [pair], J, pitch=tight + 20)
        same_bits(t1, table[p * N: (p + 1) * N], f"pair {pair} alone: table")
        same_bits(c1, curves[p * N: (p + 1) * N], f"pair {pair} alone: curves")
    for n in (0, 3):
        t1, c1 = run_pairs(r, np.ascontiguousarray(rows[:, n: n + 1]), pairs, J)
        same_bits(t1, table[n::N], f"source {n} alone: table")
        same_bits(c1, curves[n::N], f"source {n} alone: curves")


def run_exact(r):
    """Ties that need no bound.  A row against itself: peak exactly 1, lag 0, level 0 in all three windows.  A copy scaled by -0.5 and
    delayed by 7 whole samples: lag 7 in the early and the whole window, a negative peak."""
    rows = pair_rows(2, 2, 3000, 5)
    table, _ = run_pairs(r, rows, [(0, 0), (1, 1)], 48)
    for w in "ela":
        assert np.all(table[:, AT["peak_" + w]] == 1.0), (w, table[:, AT["peak_" + w]] - 1.0)
        assert np.all(table[:, AT["lag_" + w]] == 0.0) and np.all(table[:, AT["ild_db_" + w]] == 0.0)
        assert np.array_equal(table[:, AT["exx_" + w]], table[:, AT["eyy_" + w]]) and np.all(table[:, AT["exx_" + w]] > 0.0)
    rows = delayed_copy()
    want = restate(rows, [(0, 1)], 48, FS)[0]
    assert want[0, AT["lag_e"]] == 7 and want[0, AT["lag_a"]] == 7 and want[0, AT["peak_e"]] < -0.9
    table, curves = run_pairs(r, rows, [(0, 1)], 48)
    assert table[0, AT["lag_e"]] == 7.0 and table[0, AT["lag_a"]] == 7.0 and table[0, AT["peak_e"]] < 0.0 and table[0, AT["peak_a"]] < 0.0
    assert_parity(table, curves, rows, [(0, 1)], 48, FS, "a delayed, inverted copy")
    back, _ = run_pairs(r, rows[::-1].copy(), [(0, 1)], 48)                   # the pair the other way round: the sound reaches b first
    assert back[0, AT["lag_e"]] == -7.0 and back[0, AT["ild_db_e"]] < 0.0 < table[0, AT["ild_db_e"]]


def run_meaning(r):
    """What the numbers mean, by construction: the delayed copy with the late part of y replaced by independent noise is coherent in
    the early window and incoherent in the late one.  The two limits are conditions on the INPUTS (asserted on the restatement), not
    tolerances of the kernel, which is then held to the restatement.  THE SEED: the window starts at x's largest sample, and the 7
    samples of x in front of it that y's window holds pull |peak_e| 1 to 3 % under 1; of the seeds 10 .. 20 put through the
    restatement, 10, 13 and 15 give |peak_e| > 0.99 (0.9924, 0.9924, 0.9905) and every one |peak_l| < 0.2; 10 is used."""
    rows = delayed_copy(seed=10)
    L = rows.shape[-1]
    t0 = min(row_state(rows[0, 0])[2], row_state(rows[1, 0])[2])
    late = t0 + w80_of(FS)
    rng = np.random.default_rng(2024)
    rows[1, 0, late:] = (0.5 * rng.standard_normal(L - late) * np.exp(-np.arange(late, L) / 400.0)).astype(np.float32)
    want = restate(rows, [(0, 1)], 48, FS)[0]
    assert want[0, AT["t0"]] == t0
    print(f"\n[pair metrics] coherent early, independent late: peak_e {want[0, AT['peak_e']]:.7f}, peak_l {want[0, AT['peak_l']]:.4f}")
    assert abs(want[0, AT["peak_l"]]) < 0.25 and abs(want[0, AT["peak_e"]]) > 0.99
    table, curves = run_pairs(r, rows, [(0, 1)], 48)
    assert_parity(table, curves, rows, [(0, 1)], 48, FS, "coherent early, independent late")


def run_states(r):
    """A NaN sample, a silent row, pair indices outside the capsules (a line of NaN, the neighbours' bits unchanged), and a rows table
    with absurd t0 values: t0 is only compared, so the call completes and every column is finite or NaN."""
    C, N, L, J = 4, 3, 1500, 48
    rows = pair_rows(C, N, L, 21)
    rows[1, 1, 700] = np.nan
    rows[2, 0] = 0.0
    pairs = [(0, 1), (-1, 0), (2, 3), (0, C), (0, 3)]
    with np.errstate(invalid="ignore"):
        table, curves = run_pairs(r, rows, pairs, J)
        assert_parity(table, curves, rows, pairs, J, FS, "states")
    assert table[1, 0] == 1.0 and np.all(np.isnan(table[1, 1:])) and np.all(np.isnan(curves[1]))                  # (0, 1), source 1: a NaN
    assert table[2 * N, 0] == 0.0 and np.all(np.isnan(table[2 * N, 1:])) and np.all(np.isnan(curves[2 * N]))       # (2, 3), source 0: silent
    for p in (1, 3):
        assert np.all(np.isnan(table[p * N: (p + 1) * N])) and np.all(np.isnan(curves[p * N: (p + 1) * N]))
    inside = [0, 2, 4]
    with np.errstate(invalid="ignore"):
        t2, c2 = run_pairs(r, rows, [pairs[p] for p in inside], J)
    keep = np.concatenate([np.arange(p * N, (p + 1) * N) for p in inside])
    same_bits(t2, table[keep], "beside the pairs outside the capsules: table")
    same_bits(c2, curves[keep], "beside the pairs outside the capsules: curves")
    assert np.all(np.isfinite(table[[0, 2, 4 * N, 4 * N + 2]][:, [AT["peak_e"], AT["lag_e"], AT["peak_a"]]]))
    good = pair_rows(2, 6, L, 22)
    buf, stride_c, pitch = lay_out(r, good)
    honest = np.array(r.mem.download(acoustics.metrics_device(r, r.mem.ptr(buf), 2, 6, stride_c, pitch, L, FS)[0]))[: 12 * 16]
    absurd = honest.reshape(12, 16).copy()
    absurd[:, 2] = [1e300, -1e300, -5.0, 3.5, np.nan, 2.0 ** 40, np.inf, -np.inf, 1e300, 7.0, np.nan, -2.0 ** 62]
    table, curves = run_pairs(r, good, [(0, 1), (1, 0)], J, rows_table=absurd)
    assert not np.any(np.isinf(table)) and not np.any(np.isinf(curves))
    assert np.all(table[:, 0] == 0.0)
    assert np.isnan(table[0, AT["peak_a"]]) and table[0, AT["exx_a"]] == 0.0          # min(1e300, inf): both windows empty
    assert np.isnan(table[1, AT["peak_e"]]) and np.isfinite(table[1, AT["peak_l"]])   # min(-1e300, -inf): everything is late
    assert table[3, AT["t0"]] == 3.5 and np.isfinite(table[3, AT["peak_a"]])          # min(3.5, 7): from sample 4 on


# ----------------------------------------------------------------------------- the layers
def run_abi_refusals(r):
    C, N, L, J = 2, 3, 300, 5
    rows = pair_rows(C, N, L, 9)
    pitch = L
    buf = r.mem.upload(rows.reshape(-1))
    table, _ = acoustics.metrics_device(r, r.mem.ptr(buf), C, N, N * pitch, pitch, L, FS)
    pairs = r.mem.upload(np.array([0, 1, 1, 0], dtype=np.int32))
    nbytes = r.lib.call("al_ir_pair_metrics_workspace_bytes", 2, N, L, J)
    assert nbytes == 2 * N * (2 * (2 * J + 1) + 4) * 8
    ws = r.mem.empty(nbytes // 8 + 2, np.float64)
    n_out, n_xc = 2 * N * N_COLS, 2 * N * 2 * (2 * J + 1)
    out = r.mem.upload(np.full(n_out, SENTINEL64, dtype=np.float64))
    xc = r.mem.upload(np.full(n_xc, SENTINEL64, dtype=np.float64))
    good = dict(irs=r.mem.ptr(buf), C=C, N=N, stride_c=N * pitch, pitch=pitch, L=L, fs=FS, rows=r.mem.ptr(table), pairs=r.mem.ptr(pairs),
                P=2, J=J, ws=r.mem.ptr(ws), nbytes=nbytes, out=r.mem.ptr(out), xc=r.mem.ptr(xc))

    def call(**kw):
        a = {**good, **kw}
        return r.lib._al_ir_pair_metrics(a["irs"], a["C"], a["N"], a["stride_c"], a["pitch"], a["L"], a["fs"], a["rows"], a["pairs"], a["P"],
                                         a["J"], a["ws"], a["nbytes"], a["out"], a["xc"], r.mem.stream())

    null = "irs, out and workspace must not be null"
    extent = "n_capsules, n_sources and ir_len must be >= 1"
    rate = "fs must be finite and positive"
    tables = "rows and pairs must not be null"
    lag = "max_lag must be in 0 .. 1024"
    for kw, text in ((dict(irs=None), null), (dict(out=None), null), (dict(ws=None), null),
                     (dict(C=0), extent), (dict(N=0), extent), (dict(L=0), extent), (dict(N=-1), extent),
                     (dict(pitch=L - 1), "pitch < ir_len"), (dict(stride_c=N * pitch - 1), "stride_c < n_sources * pitch"),
                     (dict(C=1 << 16, N=1 << 15, stride_c=(1 << 15) * pitch), "more than 2^31 - 1 rows"),
                     (dict(C=1 << 15, N=1 << 15, L=3 * TILE, pitch=3 * TILE, stride_c=(1 << 15) * 3 * TILE),
                      "more than 2^31 - 1 (row, tile) pairs"),
                     (dict(fs=0.0), rate), (dict(fs=-1.0), rate), (dict(fs=float("nan")), rate), (dict(fs=float("inf")), rate),
                     (dict(ws=good["ws"] + 8), "workspace must be 16-byte aligned"),
                     (dict(rows=None), tables), (dict(pairs=None), tables),
                     (dict(P=0), "n_pairs must be >= 1"), (dict(P=-3), "n_pairs must be >= 1"),
                     (dict(J=-1), lag), (dict(J=1025), lag),
                     (dict(P=(1 << 31) - 1), "more than 2^31 - 1 (pair x source, tile) workgroups"),
                     (dict(nbytes=nbytes - 1), "workspace_bytes < al_ir_pair_metrics_workspace_bytes(...)")):
        assert call(**kw) == _hip.AL_E_BADARG, kw
        assert r.lib.last_error().startswith("al_ir_pair_metrics: " + text), (kw, r.lib.last_error())
    assert np.all(bits(np.array(r.mem.download(out))[:n_out]) == bits(SENTINEL64)), "a refused al_ir_pair_metrics wrote to out"
    assert np.all(bits(np.array(r.mem.download(xc))[:n_xc]) == bits(SENTINEL64)), "a refused al_ir_pair_metrics wrote to xcorr"
    for args, text in (((0, N, L, J), "n_pairs must be >= 1"), ((2, 0, L, J), "n_sources and ir_len must be >= 1"),
                       ((2, N, 0, J), "n_sources and ir_len must be >= 1"), ((2, N, L, -1), lag), ((2, N, L, 1025), lag),
                       (((1 << 31) - 1, N, L, J), "more than 2^31 - 1 (pair x source, tile) workgroups")):
        assert r.lib.call("al_ir_pair_metrics_workspace_bytes", *args) == _hip.AL_E_BADARG, args
        assert r.lib.last_error().startswith("al_ir_pair_metrics_workspace_bytes: " + text), (args, r.lib.last_error())
    assert call() == 0
    assert not np.any(bits(np.array(r.mem.download(out))[:n_out]) == bits(SENTINEL64))


def run_python_errors(r, monkeypatch):
    good = pair_rows(4, 3, 300, 9)

    def no_upload(*a, **k):
        raise AssertionError("a refused call uploaded the tensor")

    with monkeypatch.context() as mp:
        mp.setattr(engine.Renderer, "upload_irs", no_upload)
        for fn in (acoustics.ir_pair_metrics, acoustics.ir_pair_band_metrics):
            for bad in ("some", "ALL", 3, [0, 1], [[0, 1, 2]], np.zeros((0, 2), np.int32), [[0.0, 1.0]], [[0, -1]], [[4, 0]], [[0, 1], [1, 4]],
                        [["a", "b"]]):
                with pytest.raises(ValueError):
                    fn(good, FS, pairs=bad, renderer=r)
            with pytest.raises(ValueError, match="odd"):
                fn(good[:3], FS, renderer=r)
            with pytest.raises(ValueError):
                fn(good[:1], FS, pairs="all", renderer=r)
            for lag in (-1, 1025, 1.5, True, "48"):
                with pytest.raises(ValueError):
                    fn(good, FS, max_lag=lag, renderer=r)
            with pytest.raises(ValueError):
                fn(good, 2.0e6, renderer=r)                                    # the default of 1 ms is 2000 samples there
            for rate in (0, float("nan"), None, "16000", True):
                with pytest.raises(ValueError):
                    fn(good, rate, renderer=r)
            for cap in (-1, 1.5, True, None, "1G"):
                with pytest.raises(ValueError):
                    fn(good, FS, renderer=r, workspace_cap=cap)
            for bad in (good[0], good[0, 0], np.zeros((2, 0, 300), np.float32), np.zeros((0, 3, 300), np.float32), np.zeros((2, 3, 0), np.float32)):
                with pytest.raises(ValueError):
                    fn(bad, FS, renderer=r)
        for bad in ("octaves", 3, dict(centres=(500.0, 250.0)), dict(half=0)):
            with pytest.raises(ValueError):
                acoustics.ir_pair_band_metrics(good, FS, bad, renderer=r)
    with pytest.raises(ValueError):
        acoustics.ir_pair_metrics(good.astype(np.int32), FS, renderer=r)
    static = core.StaticIRState({"mic": good})
    with pytest.raises(ValueError):
        static.pair_metrics(renderer=r)              # no sample rate anywhere
    with pytest.raises(KeyError):
        static.pair_metrics("nobody", sample_rate=FS, renderer=r)


def assert_round_trip(m):
    d = m.to_dict()
    text = json.dumps(d, allow_nan=False)
    flat = lambda v: [x for y in v for x in flat(y)] if isinstance(v, list) else [v]      # noqa: E731
    assert all(v is None or type(v) is int for name in acoustics.PAIR_INTEGER_COLUMNS for v in flat(d[name]))
    back = acoustics.IRPairMetrics.from_dict(json.loads(text))
    assert np.array_equal(back.pairs, m.pairs) and back.pairs.dtype == np.int32
    assert (back.sample_rate, back.max_lag, back.centres, back.half) == (m.sample_rate, m.max_lag, m.centres, m.half)
    assert (back.xcorr is None) == (m.xcorr is None)
    for name in COLS + (("xcorr",) if m.xcorr is not None else ()):
        a, b = getattr(m, name), getattr(back, name)
        fin = np.isfinite(a)
        assert a.shape == b.shape and np.array_equal(a[fin], b[fin]) and np.all(np.isnan(b[~fin])), name


def run_python_layer(r):
    """ir_pair_metrics against the ABI; the default pairs and lag; pairs="all" on four capsules; a workspace_cap that forces one pair
    per call against an ample one, on bits; a float64 array; the properties; the dictionary round trip with NaN present."""
    C, N, L = 4, 3, 1500
    rows = pair_rows(C, N, L, 33)
    rows[3, 1, 200] = np.inf
    with np.errstate(invalid="ignore"):
        m = acoustics.ir_pair_metrics(rows, FS, pairs="all", max_lag=65, renderer=r, curves=True)
        assert m.pairs.tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]] and m.max_lag == 65 and m.sample_rate == FS
        want, want_curves = run_pairs(r, rows, m.pairs, 65)
        assert_parity(want, want_curves, rows, m.pairs, 65, FS, 'pairs="all"')
        assert m.peak_e.shape == (6, N) and m.xcorr.shape == (6, N, 2, 131) and m.table().shape == (6, N, N_COLS)
        same_bits(m.table().reshape(-1, N_COLS), want, "ir_pair_metrics against the ABI: table")
        same_bits(m.xcorr.reshape(-1, 2, 131), want_curves, "ir_pair_metrics against the ABI: curves")
        one = acoustics.ir_pair_metrics(rows.astype(np.float64), FS, pairs="all", max_lag=65, renderer=r, curves=True, workspace_cap=0)
        same_bits(one.table(), m.table(), "a float64 array, one pair per call: table")
        same_bits(one.xcorr, m.xcorr, "a float64 array, one pair per call: curves")
        plain = acoustics.ir_pair_metrics(rows, FS, renderer=r)
    assert plain.pairs.tolist() == [[0, 1], [2, 3]] and plain.max_lag == 16 and plain.xcorr is None and plain.centres is None
    same_bits(plain.table()[0, :, [0, 1]], m.table()[0, :, [0, 1]], "bad and t0 do not depend on max_lag")
    assert np.array_equal(bits(m.iacc_e), bits(np.abs(m.peak_e))) and np.array_equal(bits(m.iacc_l), bits(np.abs(m.peak_l)))
    assert np.array_equal(bits(m.iacc_a), bits(np.abs(m.peak_a))) and np.array_equal(bits(m.itd_a), bits(m.lag_a / FS))
    assert np.array_equal(bits(m.itd_e), bits(m.lag_e / FS)) and np.array_equal(bits(m.itd_l), bits(m.lag_l / FS))
    assert np.all(m.bad[[2, 4, 5], 1] == 1.0) and np.isnan(m.peak_e[2, 1]) and np.all(np.isfinite(m.peak_e[:, 0]))
    for src in (m, plain):
        assert_round_trip(src)


def binaural_state(r):
    st = core.ShoeboxIRState((5.2, 4.1, 2.7), rt60=0.25, ir_len=3000, sample_rate=16000, max_order=6, renderer=r,
                             tail=shoebox.ShoeboxTail(rt60=0.1, seed=0xC0FFEE1234567))
    st.add_binaural_listener("head", [2.1, 1.9, 1.3])
    st.add_microphone("quad", [[2.1, 1.9, 1.3], [2.3, 1.9, 1.3], [2.1, 2.1, 1.3], [2.1, 1.9, 1.5]])
    st.add_emitters([[3.9, 3.0, 1.6], [0.9, 0.8, 1.0], [2.6, 2.2, 2.0]])
    st.simulate()
    return st


def run_state(r, monkeypatch):
    """A room with a binaural listener: pair_metrics() measures the tensors where they lie (no upload, no download), equals
    ir_pair_metrics on them bit for bit and the restatement applied to the downloaded tensor, leaves to_dict() of state and scene
    alone; a StaticIRState over the downloaded tensor gives the same bits."""
    st = binaural_state(r)
    scene = core.Scene(duration=1.0, state=st, sample_rate=16000)
    scene_dict = lambda: json.dumps({k: v for k, v in scene.to_dict().items() if k != "creation_time"}, sort_keys=True)      # noqa: E731
    before, scene_before = json.dumps(st.to_dict(), sort_keys=True), scene_dict()
    t = st.irs["head"]
    assert isinstance(t, shoebox.DeviceIRTensor) and t._host is None and t.shape == (2, 3, 3000)

    def no_upload(*a, **k):
        raise AssertionError("pair_metrics() uploaded a tensor")

    with monkeypatch.context() as mp:
        mp.setattr(engine.Renderer, "upload_irs", no_upload)
        by_state = st.pair_metrics(curves=True)
        direct = acoustics.ir_pair_metrics(t, 16000, curves=True)
        only = st.pair_metrics("quad", pairs="all", max_lag=5)
        banded = st.pair_metrics("head", bands=dict(centres=(500.0, 2000.0), half=16))["head"]
        own = st.pair_metrics("head", bands=True, max_lag=3)["head"]
    assert all(v._host is None for v in st.irs.values()), "pair_metrics() downloaded a tensor"
    assert list(by_state) == ["head", "quad"] and list(only) == ["quad"]
    m = by_state["head"]
    assert m.pairs.tolist() == [[0, 1]] and m.max_lag == 16 and m.sample_rate == 16000.0 and m.peak_e.shape == (1, 3)
    assert by_state["quad"].pairs.tolist() == [[0, 1], [2, 3]] and only["quad"].peak_a.shape == (6, 3) and only["quad"].xcorr is None
    assert banded.centres == (500.0, 2000.0) and banded.half == 16 and banded.peak_e.shape == (1, 3, 2)
    assert own.centres == tuple(shoebox.ShoeboxBands().centres) and own.lag_a.shape == (1, 3, len(own.centres))
    same_bits(m.table(), direct.table(), "state.pair_metrics() against ir_pair_metrics")
    same_bits(m.xcorr, direct.xcorr, "state.pair_metrics() against ir_pair_metrics: curves")
    assert np.all(m.bad == 0) and np.all(np.isfinite(m.table())) and np.all(np.abs(m.lag_e) <= 16)
    host = np.asarray(t)
    assert_parity(m.table().reshape(-1, N_COLS), m.xcorr.reshape(-1, 2, 33), host, [(0, 1)], 16, 16000.0, "state: head")
    print(f"\n[pair metrics] binaural listener: IACC early {np.round(m.iacc_e[0], 3).tolist()}, late {np.round(m.iacc_l[0], 3).tolist()}, "
          f"ITD {np.round(1e6 * m.itd_e[0]).tolist()} us, ILD {np.round(m.ild_db_e[0], 2).tolist()} dB")
    assert_round_trip(m)
    assert json.dumps(st.to_dict(), sort_keys=True) == before and "iacc" not in before and "peak_e" not in before
    assert scene_dict() == scene_before and "peak_e" not in scene_before
    static = core.StaticIRState({"head": host}, metadata={"sample_rate": 16000})
    got = static.pair_metrics(curves=True, renderer=r)["head"]
    same_bits(got.table(), m.table(), "StaticIRState.pair_metrics()")
    same_bits(got.xcorr, m.xcorr, "StaticIRState.pair_metrics(): curves")
    assert "peak_e" not in json.dumps(static.to_dict())


def run_band_composition(r):
    """ir_pair_band_metrics against its contract composed by hand: (pair, n, b) carries the bits al_ir_pair_metrics gives for the pair
    at source n B + b of the tensor ir_band_rows returns.  Two bands, half 16, a 2 x 3 tensor; one source per pass against all at once."""
    C, N, L, J = 2, 3, 1500, 48
    rows = pair_rows(C, N, L, 55)
    bands = shoebox.ShoeboxBands(centres=(500.0, 2000.0), half=16)
    band_rows = acoustics.ir_band_rows(rows, FS, bands, renderer=r)
    assert band_rows.shape == (C, N, 2, L)
    want, want_curves = run_pairs(r, band_rows.reshape(C, N * 2, L), [(0, 1)], J)
    m = acoustics.ir_pair_band_metrics(rows, FS, bands, max_lag=J, renderer=r, curves=True)
    assert m.centres == (500.0, 2000.0) and m.half == 16 and m.max_lag == J and m.pairs.tolist() == [[0, 1]]
    assert m.peak_e.shape == (1, N, 2) and m.xcorr.shape == (1, N, 2, 2, 2 * J + 1)
    same_bits(m.table().reshape(-1, N_COLS), want, "ir_pair_band_metrics against the composition: table")
    same_bits(m.xcorr.reshape(-1, 2, 2 * J + 1), want_curves, "ir_pair_band_metrics against the composition: curves")
    one = acoustics.ir_pair_band_metrics(rows, FS, bands.to_dict(), max_lag=J, renderer=r, curves=True, workspace_cap=0)
    same_bits(one.table(), m.table(), "one source per pass: table")
    same_bits(one.xcorr, m.xcorr, "one source per pass: curves")
    assert np.all(np.isfinite(m.table()))
    assert_round_trip(m)


# ----------------------------------------------------------------------------- schedule independence (the gfx950 builds)
def run_shake_rows(r):
    """What the schedule-perturbed builds must reproduce bit for bit: the table and the curves of one call, 3 pairs x 5 sources, three
    tiles, max_lag 300 (held to the restatement first)."""
    C, N, L, J = 4, 5, 2100, 300
    pairs = [(0, 1), (2, 3), (3, 1)]
    rows = pair_rows(C, N, L, 41)
    table, curves = run_pairs(r, rows, pairs, J)
    assert_parity(table, curves, rows, pairs, J, FS, "schedule independence")
    return {"table": table, "curves": curves}
