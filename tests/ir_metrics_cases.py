"""Scenarios of the room-acoustic metrics of an IR tensor (al_ir_metrics, acoustics.ir_metrics, the states' metrics()) and the
float64 numpy restatement of their definition (the header comment of al_ir_metrics in include/audiblelight_hip.h; no reference code
computes this).  tests/test_hostemu_ir_metrics.py runs them on the host-emulated kernels, tests/test_gpu_ir_metrics.py on the gfx950
build.

THE RESTATEMENT (restate_row).  e = float64(h)^2 exactly; E(t) by a backward cumulative sum in extended precision rounded once to
float64 (at most 2^-53 E from the exact sum); D, the early windows, sum (t - t0) e and the five sums of each fit by math.fsum
(the exact sum, rounded once).  Everything else is the definition, literally.

THE BOUND (derived from the summation order of csrc/al_irmetrics.h, not tuned).  u = 2^-53.
  E(t).  Every term is >= 0, so a sum tree of depth d is within d u of the exact sum, relatively.  The device's tree for E(t) has at
  most 22 additions inside a tile plus one per tile (the head comment of al_irmetrics.h counts them); the restatement adds one
  rounding:                                  g_E = (23 + n_tiles) u.
  The direct sums (D, early_50, early_80): a lane adds its at most 16 samples, a shuffle tree of 6, the waves (at most 3), then the tiles:
  ceil(n_tiles / 64) lane-strided additions and a tree of 6; the restatement's rounding:
                                             g_S = (16 + 6 + 3 + ceil(n_tiles / 64) + 6 + 1) u = DEPTH u.
  sum (t - t0) e has one more rounding per term (the product): g_S + u.
  A level 10 log10(a / b) of two such quantities: the quotient carries g_a + g_b + u; log10 turns a relative error into
  (10 / ln 10) of it in dB; the device's log10 is taken as within 2 ulp of a result of magnitude |y| / 10 and the product with 10
  rounds once, the restatement's the same:   |delta y| <= (10 / ln 10) (g_a + g_b + u) + 6 u |y|           (dB, absolute).
  d50 = early_50 / E(t0): g_S + g_E + u.  ts = sum / (fs E(t0)): g_S + u + g_E + 2 u.  energy: g_E.  peak, t0, bad, the counts: exact.
  THE FITS.  y_t = 10 log10(E(t) / E(t0)) is off by at most dy = (10 / ln 10)(2 g_E + u) + 6 u max|y|.  All y_t <= 0 and all u_t >= 0, so
  each of the five sums is a sum of terms of one sign and its tree adds a relative DEPTH u (one more for the products):
    |d S_y|  <= n dy + DEPTH u |S_y|,   |d S_uy| <= S_u dy + (DEPTH + 1) u |S_uy|,   S_u, S_uu: relative DEPTH u (exact while below 2^53,
    which the bound does not use).
  The slope is a = num / den with num = n S_uy - S_u S_y and den = n S_uu - S_u^2, the two normal-equation differences:
    |d num| <= n |d S_uy| + S_u |d S_y| + DEPTH u S_u |S_y| + 2 u (n |S_uy| + S_u |S_y|) + u |num|
    |d den| <= (2 DEPTH + 2) u (n S_uu + S_u^2) + u |den|
    |d a| / |a| <= |d num| / |num| + |d den| / |den| + u,       RT = -60 / (a fs):  |d RT| / |RT| <= |d a| / |a| + 2 u.
  The cancellation in num and den is what the quotients |d num| / |num| and |d den| / |den| measure; they are evaluated per row from
  the restatement's own sums.  The parity check asserts that every bound it uses is below 1e-9 relative (1e-8 dB for the levels):
  with float64 sums over at most about 1e4 terms anything larger means the derivation or the kernel is wrong.

THE CONDITION ON THE INPUTS (assert_conditioned, on the restatement alone, before the device is asked): the membership sets S of the
three fits, and the validity test E(L - 1) <= threshold, are unchanged when all four thresholds are scaled by 1 +- 1e-12: then the
device's E(t), within g_E < 1e-14 of the restatement's, puts every sample into the same sets, and the integer columns compare
exactly.  Seeds are chosen so that every row of every scenario meets it; none is left out.
"""
import json
import math

import numpy as np
import pytest

from audiblelight_amd import _hip, acoustics, core, shoebox

FS = 16000.0
W_D, W_50, W_80 = 40, 800, 1280            # rint(0.0025 fs), rint(0.05 fs), rint(0.08 fs)
TILE = 1024                                # samples of a workgroup tile (csrc/al_irmetrics.h IRM_TILE)
U = 2.0 ** -53
DB = 10.0 / math.log(10.0)
COLS = acoustics.COLUMNS
INT_COLS = ("bad", "t0", "n_edt", "n_t20", "n_t30")
DB_COLS = ("drr_db", "c50_db", "c80_db", "dyn_db")
FITS = (("edt", 0.0, -10.0), ("t20", -5.0, -25.0), ("t30", -5.0, -35.0))
WORST = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def windows(fs):
    return tuple(int(min(np.rint(s * fs), 2.0 ** 31)) for s in (0.0025, 0.05, 0.08))


# ----------------------------------------------------------------------------- the restatement
def edc_of(h):
    """E(t), t < L, float64: the backward cumulative sum in extended precision, rounded once."""
    e = np.asarray(h, dtype=np.float32).astype(np.float64) ** 2
    with np.errstate(invalid="ignore", over="ignore"):
        return np.cumsum(e[::-1].astype(np.longdouble))[::-1].astype(np.float64), e


def membership(E, t0, e_t0, hi, lo, scale=1.0):
    t = np.arange(len(E))
    keep = (t >= t0) & (E > e_t0 * 10.0 ** (lo / 10.0) * scale)
    if hi != 0.0:
        keep &= E <= e_t0 * 10.0 ** (hi / 10.0) * scale
    return keep


def restate_row(h, fs=FS):
    """(columns dict, knots, bounds dict, conditioned flag) of one row."""
    h = np.asarray(h, dtype=np.float32)
    L = len(h)
    w_d, w_50, w_80 = windows(fs)
    n_tiles = -(-L // TILE)
    g_e = (23 + n_tiles) * U
    depth = 16 + 6 + 3 + -(-n_tiles // 64) + 6 + 1
    g_s = depth * U
    E, e = edc_of(h)
    at = lambda t: float(E[t]) if t < L else 0.0                                                      # noqa: E731
    n_knots = (L - 1) // 256 + 2
    knots = np.array([at(256 * k) for k in range(n_knots)])
    nan = float("nan")
    col = dict.fromkeys(COLS, nan)
    bound = dict.fromkeys(COLS, 0.0)
    col["bad"] = float(np.count_nonzero(~np.isfinite(h)))
    if col["bad"] > 0:
        return col, knots, bound, True
    peak = float(np.max(np.abs(h)))
    if peak == 0.0:
        col.update(energy=0.0, t0=0.0, peak=0.0)
        return col, knots, bound, True
    t0 = int(np.flatnonzero(np.abs(h) == np.float32(peak))[0])
    e_t0 = at(t0)
    col.update(energy=at(0), t0=float(t0), peak=peak)
    bound["energy"] = g_e
    level = lambda a, b: float("inf") if b == 0.0 else 10.0 * math.log10(a / b)                       # noqa: E731
    level_bound = lambda y, ga, gb: 0.0 if not np.isfinite(y) else DB * (ga + gb + U) + 6 * U * abs(y)      # noqa: E731
    D = math.fsum(e[max(0, t0 - w_d): min(L - 1, t0 + w_d) + 1])
    col["drr_db"] = level(D, at(t0 + w_d + 1))
    bound["drr_db"] = level_bound(col["drr_db"], g_s, g_e)
    early = {}
    for name, w in (("c50_db", w_50), ("c80_db", w_80)):
        early[name] = math.fsum(e[t0: min(L, t0 + w)])
        col[name] = level(early[name], at(t0 + w))
        bound[name] = level_bound(col[name], g_s, g_e)
    col["d50"] = early["c50_db"] / e_t0
    bound["d50"] = g_s + g_e + U
    t = np.arange(L)
    col["ts"] = math.fsum(((t - t0) * e)[t0:]) / (fs * e_t0)
    bound["ts"] = g_s + g_e + 3 * U
    with np.errstate(divide="ignore"):
        col["dyn_db"] = 10.0 * math.log10(at(L - 1) / e_t0) if at(L - 1) > 0.0 else float("-inf")
    bound["dyn_db"] = level_bound(col["dyn_db"], 0.0, g_e)
    conditioned = True
    for name, hi, lo in FITS:
        keep = membership(E, t0, e_t0, hi, lo)
        thr = e_t0 * 10.0 ** (lo / 10.0)
        for scale in (1.0 - 1e-12, 1.0 + 1e-12):
            conditioned &= bool(np.array_equal(membership(E, t0, e_t0, hi, lo, scale), keep))
            conditioned &= (at(L - 1) <= thr * scale) == (at(L - 1) <= thr)
        n = int(keep.sum())
        col["n_" + name] = float(n)
        if n < 2 or not at(L - 1) <= thr:
            continue
        u = (t[keep] - t0).astype(np.float64)
        y = 10.0 * np.log10(E[keep] / e_t0)
        s_u, s_uu, s_y, s_uy = math.fsum(u), math.fsum(u * u), math.fsum(y), math.fsum(u * y)
        num, den = n * s_uy - s_u * s_y, n * s_uu - s_u * s_u
        a = num / den
        col[name] = float("nan") if a == 0.0 else -60.0 / (a * fs)
        dy = DB * (2 * g_e + U) + 6 * U * float(np.max(np.abs(y)))
        d_sy = n * dy + depth * U * abs(s_y)
        d_suy = s_u * dy + (depth + 1) * U * abs(s_uy)
        d_num = n * d_suy + s_u * d_sy + depth * U * s_u * abs(s_y) + 2 * U * (n * abs(s_uy) + s_u * abs(s_y)) + U * abs(num)
        d_den = (2 * depth + 2) * U * (n * s_uu + s_u * s_u) + U * abs(den)
        bound[name] = d_num / abs(num) + d_den / abs(den) + 3 * U
    return col, knots, bound, conditioned


_RESTATED = {}


def restate(rows, fs=FS):
    """The restatement of every row of a (C, N, L) tensor, computed once per tensor and shared (read-only): (table (C N, 16), knots
    (C N, n_knots), bounds (C N, 16), conditioned (C N,))."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    key = (rows.tobytes(), rows.shape, fs)
    if key not in _RESTATED:
        flat = rows.reshape(-1, rows.shape[-1])
        got = [restate_row(h, fs) for h in flat]
        out = tuple(np.array(x) for x in ([[g[0][c] for c in COLS] for g in got], [g[1] for g in got],
                                          [[g[2][c] for c in COLS] for g in got], [g[3] for g in got]))
        for a in out:
            a.flags.writeable = False
        _RESTATED[key] = out
    return _RESTATED[key]


def assert_conditioned(rows, fs=FS, what=""):
    cond = restate(rows, fs)[3]
    assert np.all(cond), f"{what}: rows {np.flatnonzero(~cond).tolist()} have a sample within 1e-12 of a fit threshold: pick another seed"


def assert_parity(table, knots, rows, fs=FS, what=""):
    """All 16 columns and the knots of every row against the restatement."""
    assert_conditioned(rows, fs, what)
    want, want_knots, bound, _ = restate(rows, fs)
    assert table.shape == want.shape, (what, table.shape, want.shape)
    for i, name in enumerate(COLS):
        got, ref, b = table[:, i], want[:, i], bound[:, i]
        same_kind = (np.isnan(got) == np.isnan(ref)) & (np.isposinf(got) == np.isposinf(ref)) & (np.isneginf(got) == np.isneginf(ref))
        assert np.all(same_kind), f"{what}: column {name}: {got} against {ref}"
        fin = np.isfinite(ref)
        if name in INT_COLS or name == "peak":
            assert np.array_equal(got[fin], ref[fin]), f"{what}: column {name}: {got} against {ref}"
            continue
        limit = 1e-8 if name in DB_COLS else 1e-9
        assert np.all(b[fin] < limit), f"{what}: column {name}: the derived bound {b[fin].max():.3g} is not below {limit:g}"
        err = np.abs(got[fin] - ref[fin]) / (1.0 if name in DB_COLS else np.where(ref[fin] == 0.0, 1.0, np.abs(ref[fin])))
        over = err > b[fin]
        assert not np.any(over), f"{what}: column {name}: error {err[over]} over the bound {b[fin][over]} (rows {np.flatnonzero(fin)[over]})"
        if fin.any() and np.any(b[fin] > 0):
            frac = float(np.max(err[b[fin] > 0] / b[fin][b[fin] > 0]))
            WORST[name] = max(WORST.get(name, 0.0), frac)
    if knots is not None:
        assert knots.shape == want_knots.shape, (what, knots.shape, want_knots.shape)
        n_tiles = -(-rows.shape[-1] // TILE)
        fin = np.isfinite(want_knots)
        assert np.array_equal(np.isnan(knots), np.isnan(want_knots)) and np.array_equal(np.isposinf(knots), np.isposinf(want_knots)), what
        assert np.all(np.abs(knots[fin] - want_knots[fin]) <= (23 + n_tiles) * U * want_knots[fin]), f"{what}: knots"
        ok = ~np.isnan(want_knots[:, -1])
        assert not np.any(bits(knots[ok, -1])), f"{what}: the last knot must be +0"


# ----------------------------------------------------------------------------- inputs
def decay_row(L, rt, lead, seed, spike=2.0, sigma=0.25, fs=FS):
    """Seeded Gaussian noise under 10^(-3 (t - lead) / (rt fs)) from ``lead`` on, silence in front of it, one direct spike at ``lead``."""
    rng = np.random.default_rng(seed)
    t = np.arange(L)
    lead = min(lead, L - 1)
    h = sigma * rng.standard_normal(L) * 10.0 ** (-3.0 * (t - lead) / (rt * fs))
    h[:lead] = 0.0
    h[lead] = spike
    return h.astype(np.float32)


def generic_rows(L, seed):
    """(2, 3, L): the peak at sample 0, a third in, and at the last sample; a slow decay; two equal maxima; a fast decay at the end."""
    rows = [decay_row(L, 0.05, 0, seed), decay_row(L, 0.08, L // 3, seed + 1), decay_row(L, 0.05, L - 1, seed + 2),
            decay_row(L, 0.6, min(7, L - 1), seed + 3), decay_row(L, 0.1, L // 5, seed + 4), decay_row(L, 0.03, L // 2, seed + 5)]
    if L >= 3:
        rows[4][min(L - 1, L // 5 + 1 + L // 4)] = -rows[4][L // 5]        # an equal maximum further on: the first must win
    return np.stack(rows).reshape(2, 3, L)


def tiled_rows(seed=100):
    """(2, 3, 9001), nine tiles: the peak in the last tile; on a tile boundary (4096) and just in front of it (4095); thresholds
    crossed in a later tile than the peak's (at 3900 with 0.3 s: -25 dB about 2000 samples on); a decay that reaches -25 dB but not
    -35 dB (the last sample holds -30 dB of the row's energy); two equal maxima on either side of a tile boundary."""
    L = 9001
    rows = [decay_row(L, 0.05, 8500, seed), decay_row(L, 0.2, 4096, seed + 1), decay_row(L, 0.2, 4095, seed + 2),
            decay_row(L, 0.3, 3900, seed + 3), decay_row(L, 0.15, 500, seed + 4), decay_row(L, 0.1, 4000, seed + 5)]
    total = float(np.sum(rows[4].astype(np.float64) ** 2))
    rows[4][L - 1] = np.float32(math.sqrt(1e-3 * total))
    rows[5][4100] = rows[5][4000]
    return np.stack(rows).reshape(2, 3, L)


def special_rows(L=1500, seed=200):
    """(2, 3, L): a silent row, a row with a NaN and a row with an Inf among good rows."""
    rows = generic_rows(L, seed).reshape(6, L)
    rows[1] = 0.0
    rows[2, 700] = np.nan
    rows[4, 3] = np.inf
    rows[4, 900] = -np.inf
    return rows.reshape(2, 3, L)


LENGTHS = (1, 2, 255, 256, 257, TILE - 1, TILE, TILE + 1)
SEEDS = {1: 1, 2: 2, 255: 3, 256: 4, 257: 5, TILE - 1: 6, TILE: 7, TILE + 1: 8}


# ----------------------------------------------------------------------------- the device
def put(buf, off, values):
    values = np.ascontiguousarray(values, dtype=np.float32)
    if isinstance(buf, np.ndarray):
        buf[off: off + len(values)] = values
    else:
        import torch

        buf[off: off + len(values)].copy_(torch.from_numpy(values))


def run_table(r, rows, fs=FS, pitch=None, stride_c=None, offset=0, edc=True, buf=None):
    """The tensor laid out at the given pitch, stride and element offset, every float that is no sample a NaN (a sentinel: read into
    any sum it would show in every column), through al_ir_metrics: (table (C N, 16), knots or None)."""
    C, N, L = rows.shape
    pitch = (L + 3) // 4 * 4 if pitch is None else pitch
    stride_c = N * pitch if stride_c is None else stride_c
    if buf is None:
        host = np.full(offset + C * stride_c + 8, np.nan, dtype=np.float32)
        for c in range(C):
            for n in range(N):
                at = offset + c * stride_c + n * pitch
                host[at: at + L] = rows[c, n]
        buf = r.mem.upload(host)
    else:
        for c in range(C):
            for n in range(N):
                put(buf, offset + c * stride_c + n * pitch, rows[c, n])
    out, knots = acoustics.metrics_device(r, r.mem.ptr(buf) + 4 * offset, C, N, stride_c, pitch, L, fs, edc)
    table = np.array(r.mem.download(out))[: C * N * 16].reshape(C * N, 16)
    if edc:
        k = acoustics.n_knots_of(L)
        return table, np.array(r.mem.download(knots))[: C * N * k].reshape(C * N, k)
    return table, None


def same_bits(a, b, what):
    assert np.array_equal(bits(a), bits(b)), f"{what}: {np.argwhere(bits(a) != bits(b)).tolist()[:8]}"


def check_layouts(r, rows, what):
    """Parity at the tight pitch; then a larger pitch, a larger stride_c, the odd pitch at an unaligned base (the scalar arm), a second
    run and the call without knots: the same bits each."""
    C, N, L = rows.shape
    table, knots = run_table(r, rows)
    assert_parity(table, knots, rows, what=what)
    tight = (L + 3) // 4 * 4
    for name, kw in (("a larger pitch", dict(pitch=tight + 8)), ("a larger stride_c", dict(stride_c=N * tight + 16)),
                     ("an odd pitch at an unaligned base", dict(pitch=tight + 3, stride_c=N * (tight + 3) + 5, offset=1)),
                     ("a second run", dict())):
        t2, k2 = run_table(r, rows, **kw)
        same_bits(t2, table, f"{what}: {name}: table")
        same_bits(k2, knots, f"{what}: {name}: knots")
    t3, _ = run_table(r, rows, edc=False)
    same_bits(t3, table, f"{what}: without knots")
    return table, knots


def run_length(r, L):
    check_layouts(r, generic_rows(L, SEEDS[L]), f"ir_len {L}")


def run_tiled(r):
    rows = tiled_rows()
    table, _ = check_layouts(r, rows, "nine tiles")
    col = {name: table[:, i] for i, name in enumerate(COLS)}
    assert col["t0"].tolist() == [8500.0, 4096.0, 4095.0, 3900.0, 500.0, 4000.0]
    assert np.isfinite(col["t20"][4]) and np.isnan(col["t30"][4]) and -35.0 < col["dyn_db"][4] < -25.0      # reaches -25, not -35 dB
    assert np.all(np.isfinite(table[[1, 2, 3, 5]][:, 9:12]))                                                # every fit of the long rows
    assert col["t0"][3] + col["n_t30"][3] > 4096                                                            # crossed in a later tile
    assert np.isposinf(col["c50_db"][0]) and np.isposinf(col["c80_db"][0]) and np.isfinite(col["drr_db"][0])     # 8500 + 800 > 9001


def run_features(r):
    """What the short rows must show: first of two equal maxima, a row too short for any fit, the windows past the row's end."""
    L = 257
    rows = generic_rows(L, SEEDS[L])
    table, _ = run_table(r, rows)
    col = {name: table[:, i] for i, name in enumerate(COLS)}
    assert col["t0"][4] == L // 5 and rows[0, 0, 0] == 2.0
    assert np.all(np.isposinf(col["c50_db"])) and np.all(np.isposinf(col["c80_db"]))        # w_50 = 800 is past the end of every row
    assert np.all(np.isnan(table[2, 9:12])) and col["dyn_db"][2] == 0.0 and np.isposinf(col["drr_db"][2])     # the peak at the last sample
    two, _ = run_table(r, generic_rows(2, SEEDS[2]))
    assert np.all(np.isnan(two[:, 9:12])) and np.all(two[:, 12] == 1.0)                      # two samples: no fit has room
    one, _ = run_table(r, generic_rows(1, SEEDS[1]))
    assert np.all(one[:, 12] == 1.0) and np.all(np.isnan(one[:, 9:12])) and np.all(one[:, 15] == 0.0)


def run_special(r):
    rows = special_rows()
    table, knots = check_layouts(r, rows, "silent and non-finite rows")
    assert table[1, :4].tolist() == [0.0, 0.0, 0.0, 0.0] and np.all(np.isnan(table[1, 4:])) and not np.any(bits(knots[1]))
    assert table[2, 0] == 1.0 and np.all(np.isnan(table[2, 1:])) and table[4, 0] == 2.0 and np.all(np.isnan(table[4, 1:]))
    assert np.all(np.isnan(knots[2, :3])) and np.all(np.isfinite(knots[2, 3:])) and np.all(np.isposinf(knots[4, :4]))
    assert np.all(np.isfinite(table[[0, 3, 5]][:, :5]))


def run_identity(r):
    """A row alone against the row among others, at two pitches and in two runs: identical bits of the 16 columns and the knots."""
    for rows in (tiled_rows(), generic_rows(TILE + 1, SEEDS[TILE + 1])):
        C, N, L = rows.shape
        table, knots = run_table(r, rows)
        for c, n in ((0, 0), (1, 1), (1, 2)):
            for pitch in ((L + 3) // 4 * 4, (L + 3) // 4 * 4 + 20):
                for _ in range(2):
                    t1, k1 = run_table(r, rows[c: c + 1, n: n + 1], pitch=pitch)
                    same_bits(t1[0], table[c * N + n], f"row ({c}, {n}) alone, pitch {pitch}: table")
                    same_bits(k1[0], knots[c * N + n], f"row ({c}, {n}) alone, pitch {pitch}: knots")


def run_wide(r, position, reserve, need):
    """The second capsule's rows past element 2^31 ("i31") or past byte 2^32 ("b32") through stride_c, in an untouched buffer: bit for
    bit the rows at a small stride."""
    rows = generic_rows(TILE + 1, SEEDS[TILE + 1])
    C, N, L = rows.shape
    pitch = (L + 3) // 4 * 4
    stride_c = {"i31": (1 << 31) + 16, "b32": (1 << 30) + 16}[position]
    want, want_knots = run_table(r, rows)
    total = stride_c + N * pitch + 8
    need(r, 4 * total)
    buf = reserve(r, total)
    got, got_knots = run_table(r, rows, stride_c=stride_c, buf=buf)
    same_bits(got, want, f"{position}: table")
    same_bits(got_knots, want_knots, f"{position}: knots")


def run_shake_rows(r):
    """What the schedule-perturbed builds must reproduce bit for bit: the tables and knots of the tiled and the special scenario."""
    out = {}
    for name, rows in (("tiled", tiled_rows()), ("special", special_rows()), ("tile + 1", generic_rows(TILE + 1, SEEDS[TILE + 1]))):
        table, knots = run_table(r, rows)
        assert_parity(table, knots, rows, what=name)
        out[name + ": table"], out[name + ": knots"] = table, knots
    return out


# ----------------------------------------------------------------------------- the layers
def run_abi_refusals(r):
    rows = generic_rows(300, 9)
    C, N, L = rows.shape
    pitch = 300
    buf = r.mem.upload(rows.reshape(-1))
    nbytes = r.lib.call("al_ir_metrics_workspace_bytes", C, N, L)
    assert nbytes > 0 and r.lib.call("al_ir_metrics_workspace_bytes", 0, N, L) == 0 and r.lib.call("al_ir_metrics_workspace_bytes", C, N, 0) == 0
    ws = r.mem.empty(nbytes // 8 + 2, np.float64)
    out = r.mem.empty(C * N * 16, np.float64)
    good = dict(irs=r.mem.ptr(buf), C=C, N=N, stride_c=N * pitch, pitch=pitch, L=L, fs=FS, ws=r.mem.ptr(ws), nbytes=nbytes, out=r.mem.ptr(out))

    def call(**kw):
        a = {**good, **kw}
        return r.lib._al_ir_metrics(a["irs"], a["C"], a["N"], a["stride_c"], a["pitch"], a["L"], a["fs"], a["ws"], a["nbytes"], a["out"], None,
                                    r.mem.stream())

    assert call() == 0
    null = "al_ir_metrics: irs, out and workspace must not be null"
    extent = "al_ir_metrics: n_capsules, n_sources and ir_len must be >= 1"
    rate = "al_ir_metrics: fs must be finite and positive"
    for kw, text in ((dict(irs=None), null), (dict(out=None), null), (dict(ws=None), null),
                     (dict(C=0), extent), (dict(N=0), extent), (dict(L=0), extent), (dict(N=-1), extent),
                     (dict(pitch=L - 1), "al_ir_metrics: pitch < ir_len"),
                     (dict(stride_c=N * pitch - 1), "al_ir_metrics: stride_c < n_sources * pitch"),
                     (dict(C=1 << 16, N=1 << 15, stride_c=(1 << 15) * pitch), "al_ir_metrics: more than 2^31 - 1 rows"),
                     (dict(C=1 << 15, N=1 << 15, L=3 * TILE, pitch=3 * TILE, stride_c=(1 << 15) * 3 * TILE),
                      "al_ir_metrics: more than 2^31 - 1 (row, tile) pairs"),
                     (dict(fs=0.0), rate), (dict(fs=-1.0), rate), (dict(fs=float("nan")), rate), (dict(fs=float("inf")), rate),
                     (dict(nbytes=nbytes - 1), "al_ir_metrics: workspace_bytes < al_ir_metrics_workspace_bytes(...)"),
                     (dict(ws=r.mem.ptr(ws) + 8), "al_ir_metrics: workspace must be 16-byte aligned")):
        assert call(**kw) == _hip.AL_E_BADARG, kw
        assert r.lib.last_error() == text, (kw, r.lib.last_error())


def run_python_errors(r):
    good = generic_rows(300, 9)
    for bad in (good[0], good[0, 0], good[None], np.zeros((2, 0, 300), np.float32), np.zeros((0, 3, 300), np.float32),
                np.zeros((2, 3, 0), np.float32), good.astype(np.int32)):
        with pytest.raises(ValueError):
            acoustics.ir_metrics(bad, FS, renderer=r)
    for rate in (0, -16000.0, float("nan"), float("inf"), None, "16000", True):
        with pytest.raises(ValueError):
            acoustics.ir_metrics(good, rate, renderer=r)
    empty = shoebox.DeviceIRTensor(r, r.mem.empty(16), (0, 300), (2, 0, 300))
    with pytest.raises(ValueError):
        acoustics.ir_metrics(empty, FS)
    st = core.ShoeboxIRState((4.0, 3.0, 2.5), rt60=0.3, ir_len=512, sample_rate=16000, renderer=r)
    st.add_microphone("mic", [[1.0, 1.0, 1.0]])
    st.add_emitters([[2.0, 2.0, 1.5]])
    with pytest.raises(AttributeError):
        st.metrics()                      # as .irs before simulate()
    static = core.StaticIRState({"mic": good})
    with pytest.raises(ValueError):
        static.metrics(renderer=r)        # no sample rate anywhere
    with pytest.raises(KeyError):
        static.metrics("nobody", sample_rate=FS, renderer=r)


def small_state(r):
    st = core.ShoeboxIRState((5.2, 4.1, 2.7), rt60=0.25, ir_len=3000, sample_rate=16000, max_order=6, renderer=r,
                             tail=shoebox.ShoeboxTail(rt60=0.1, seed=0xC0FFEE1234567))
    st.add_microphone("pair", [[2.1, 1.9, 1.3], [2.3, 1.9, 1.3]])
    st.add_microphone("single", [[1.0, 3.0, 1.1]])
    st.add_emitters([[3.9, 3.0, 1.6], [0.9, 0.8, 1.0], [2.6, 2.2, 2.0]])
    st.simulate()
    return st


def table_of(m):
    return m.table().reshape(-1, 16)


def run_state(r):
    """ir_metrics on the DeviceIRTensor of a small ShoeboxIRState equals the restatement applied to the downloaded tensor, and has not
    downloaded it; the same through state.metrics() and through a host float64 array."""
    st = small_state(r)
    t = st.irs["pair"]
    assert isinstance(t, shoebox.DeviceIRTensor) and t._host is None
    m = acoustics.ir_metrics(t, 16000, edc=True)
    assert t._host is None, "ir_metrics downloaded the tensor"
    assert m.sample_rate == 16000.0 and m.t30.shape == (2, 3) and m.edc_knots.shape == (2, 3, acoustics.n_knots_of(3000))
    by_state = st.metrics(edc=True)
    assert list(by_state) == ["pair", "single"] and all(v._host is None for v in st.irs.values())
    assert list(st.metrics("single")) == ["single"] and st.metrics("single")["single"].edc_knots is None
    host = np.asarray(t)
    assert_parity(table_of(m), m.edc_knots.reshape(6, -1), host, 16000.0, "state: pair")
    assert_parity(table_of(by_state["single"]), by_state["single"].edc_knots.reshape(3, -1), np.asarray(st.irs["single"]), 16000.0, "state: single")
    same_bits(table_of(by_state["pair"]), table_of(m), "state.metrics() against ir_metrics")
    same_bits(by_state["pair"].edc_knots, m.edc_knots, "state.metrics() against ir_metrics: knots")
    assert np.all(np.isfinite(m.t30)) and np.all(m.bad == 0)
    m64 = acoustics.ir_metrics(host.astype(np.float64), 16000.0, renderer=r, edc=True)
    same_bits(table_of(m64), table_of(m), "a host float64 array")
    same_bits(m64.edc_knots, m.edc_knots, "a host float64 array: knots")
    static = core.StaticIRState({"pair": host}, metadata={"sample_rate": 16000})
    same_bits(table_of(static.metrics(renderer=r)["pair"]), table_of(m), "StaticIRState.metrics()")
    assert "metrics" not in json.dumps(st.to_dict()) and "t30" not in json.dumps(st.to_dict())


def run_round_trip(r):
    """to_dict / from_dict with NaN and inf present: strict JSON, integers for the integer columns, None for what is not finite."""
    m = acoustics.ir_metrics(special_rows(), FS, renderer=r, edc=True)
    assert np.isnan(m.t30).any() and np.isposinf(m.edc_knots).any()
    short = acoustics.ir_metrics(generic_rows(257, SEEDS[257]), FS, renderer=r)
    assert np.isposinf(short.c50_db).all() and short.edc_knots is None
    for src in (m, short):
        d = src.to_dict()
        text = json.dumps(d, allow_nan=False)
        assert all(v is None or type(v) is int for name in INT_COLS for row in d[name] for v in row)
        back = acoustics.IRMetrics.from_dict(json.loads(text))
        assert back.sample_rate == src.sample_rate and (back.edc_knots is None) == (src.edc_knots is None)
        for name in COLS + (("edc_knots",) if src.edc_knots is not None else ()):
            a, b = getattr(src, name), getattr(back, name)
            fin = np.isfinite(a)
            assert a.shape == b.shape and np.array_equal(a[fin], b[fin]) and np.all(np.isnan(b[~fin])), name
