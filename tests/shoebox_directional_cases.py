"""Scenarios of the directional receivers of the device shoebox IR generator (al_ism_shoebox_dir, al_ism_shoebox_dir_tail,
shoebox.first_order / cardioid / foa_patterns, core.ShoeboxIRState.add_microphone(patterns=...) / add_foa_listener) and the float64
numpy oracle of their definition (DESIGN.md "Shoebox IRs: directional receivers"; no reference code computes this).
tests/test_hostemu_shoebox_directional.py runs them on the host-emulated kernels, tests/test_gpu_shoebox_directional.py on the gfx950
build.

THE ORACLE is shoebox_cases.oracle_pair with the amplitude a of every image replaced by a (w + v . R / d), R the image's offset from
the receiver and d = |R|.

THE BOUND (derived as shoebox_cases' is, not tuned), every sample, none excluded:
    |y - y64| <= 2^-24 |y64| + 2^-30 A_k[t],     A_k[t] = sum over the images with a tap at t of |a| (|w| + |v|_2).
|w + v . u| <= |w| + |v|_2 for a unit u, so A_k is the sum of the largest magnitudes the channel's taps can have: it does not shrink
where the gain cancels (a dipole seen side on), which is where the float64 rounding of w + v . u is large relative to the gain
itself.  The gain adds three roundings of 2^-53 (|w| + |v|_2) to shoebox_cases' error budget, twenty-three binary orders below
2^-30.  The tail's bound is shoebox_tail_cases' with A_k in place of A.
"""
import ctypes as ct
import functools
import json

import numpy as np
import pytest

from audiblelight_amd import core, engine, shoebox
from tests import noise_draw_cases as nd
from tests import shoebox_cases as sc
from tests import shoebox_tail_cases as tc

bits = sc.bits
OBLIQUE = (0.48, -0.6, 0.64)          # a unit vector with three different components


def mixed4():
    """Four patterns that share nothing: a cardioid, alpha = 0.25 along OBLIQUE, a negative w, a dipole off axis."""
    return np.array([shoebox.cardioid((1.0, 0.0, 0.0)), shoebox.first_order(0.25, OBLIQUE), shoebox.first_order(-0.3, (-0.2, 0.5, 0.1)),
                     shoebox.first_order(0.0, (0.3, 0.4, -0.5))])


# ----------------------------------------------------------------------------- the oracle: the definition, in float64
def oracle_point(room, betas, s, r, patterns, ir_len, fs, c=sc.C_SOUND, max_order=None):
    """(y64[K, ir_len], A[K, ir_len], n_images) of one source at one receiver position with K patterns: shoebox_cases.oracle_pair
    with a (w + v . R / d) for a."""
    patterns = np.asarray(patterns, dtype=np.float64).reshape(-1, 4)
    reach = c * (ir_len + sc.HALF) / fs
    ax = [sc._axis(s[i], r[i], room[i], betas[2 * i], betas[2 * i + 1], reach) for i in range(3)]
    Rx, Ry, Rz = np.meshgrid(ax[0][0], ax[1][0], ax[2][0], indexing="ij")
    order = ax[0][1][:, None, None] + ax[1][1][None, :, None] + ax[2][1][None, None, :]
    gain = ax[0][2][:, None, None] * ax[1][2][None, :, None] * ax[2][2][None, None, :]
    d = np.sqrt(Rx * Rx + Ry * Ry + Rz * Rz)
    tau = d * fs / c
    keep = (tau - sc.HALF < ir_len) & (gain > 0.0)
    if max_order is not None:
        keep &= order <= max_order
    R = np.stack([Rx[keep], Ry[keep], Rz[keep]], axis=1)
    d, tau, gain = d[keep], tau[keep], gain[keep]
    a = gain / (4.0 * np.pi * d)
    u = R / d[:, None]
    a_k = a[:, None] * (patterns[None, :, 0] + u @ patterns[:, 1:].T)                                  # (images, K)
    a_abs = np.abs(a)[:, None] * (np.abs(patterns[:, 0]) + np.sqrt((patterns[:, 1:] ** 2).sum(axis=1)))[None, :]
    K = len(patterns)
    y, A, used = np.zeros((K, ir_len)), np.zeros((K, ir_len)), 0
    for i, ti in enumerate(tau):
        lo, hi = int(np.ceil(ti - sc.HALF)), int(np.floor(ti + sc.HALF))
        t = np.arange(max(lo, 0), min(hi, ir_len - 1) + 1)
        x = t - ti
        t, x = t[np.abs(x) < sc.HALF], x[np.abs(x) < sc.HALF]
        if t.size == 0:
            continue
        used += 1
        shape = 0.5 * (1.0 + np.cos(2.0 * np.pi * x / sc.TAPS)) * np.sinc(x)
        for k in range(K):
            y[k, t] += a_k[i, k] * shape
            A[k, t] += a_abs[i, k]
    return y, A, used


@functools.lru_cache(maxsize=None)
def _oracle_cached(room, betas, sources, positions, patterns, ir_len, fs, c, max_order):
    P, N = len(positions), len(sources)
    pat = np.array(patterns)
    K = pat.shape[1]
    y, A, used = np.zeros((P * K, N, ir_len)), np.zeros((P * K, N, ir_len)), np.zeros((P, N), dtype=np.int64)
    for p in range(P):
        for n in range(N):
            y[p * K:(p + 1) * K, n], A[p * K:(p + 1) * K, n], used[p, n] = oracle_point(room, betas, sources[n], positions[p], pat[p], ir_len,
                                                                                       fs, c, max_order)
    for arr in (y, A, used):
        arr.flags.writeable = False
    return y, A, used


def oracle(room, betas, sources, positions, patterns, ir_len, fs, c=sc.C_SOUND, max_order=None):
    """(y64, A) of shape (P K, N, ir_len) and the image counts (P, N); computed once per scenario and shared (read-only)."""
    as_t = lambda v: tuple(float(x) for x in np.ravel(v))                                   # noqa: E731
    pts = lambda v: tuple(tuple(float(x) for x in row) for row in np.atleast_2d(v))           # noqa: E731
    pat = tuple(tuple(tuple(float(x) for x in ch) for ch in pos) for pos in np.asarray(patterns, dtype=np.float64))
    return _oracle_cached(as_t(room), as_t(betas), pts(sources), pts(positions), pat, int(ir_len), float(fs), float(c), max_order)


# ----------------------------------------------------------------------------- running the entry points
def _tables(r, sources, positions, patterns):
    sources = np.ascontiguousarray(np.atleast_2d(sources), dtype=np.float64)
    positions = np.ascontiguousarray(np.atleast_2d(positions), dtype=np.float64)
    patterns = np.ascontiguousarray(patterns, dtype=np.float64)
    assert patterns.ndim == 3 and patterns.shape[0] == len(positions) and patterns.shape[2] == 4
    return sources, positions, patterns


def run_abi(r, room, betas, sources, positions, patterns, ir_len, fs, c=sc.C_SOUND, max_order=None, pitch=None):
    """al_ism_shoebox_dir into a buffer with sc.GUARD sentinels on either side: the (P K, N, pitch) rows, the guards checked."""
    mem, lib = r.mem, r.lib
    sources, positions, patterns = _tables(r, sources, positions, patterns)
    n, n_pos, K = len(sources), len(positions), patterns.shape[1]
    pitch = shoebox.pitch_of(ir_len) if pitch is None else pitch
    total = n_pos * K * n * pitch
    out = mem.upload(np.full(total + 2 * sc.GUARD, sc.SENTINEL, dtype=np.float32))
    src_dev, pos_dev, pat_dev = mem.upload(sources.reshape(-1)), mem.upload(positions.reshape(-1)), mem.upload(patterns.reshape(-1))
    L, beta = (ct.c_double * 3)(*room), (ct.c_double * 6)(*betas)
    lib.call("al_ism_shoebox_dir", mem.ptr(src_dev), n, mem.ptr(pos_dev), n_pos, mem.ptr(pat_dev), K, L, beta, float(c), float(fs),
             -1 if max_order is None else int(max_order), int(ir_len), int(pitch), mem.ptr(out) + 4 * sc.GUARD, mem.stream())
    host = np.asarray(mem.download(out))
    assert np.all(host[:sc.GUARD] == sc.SENTINEL) and np.all(host[sc.GUARD + total:] == sc.SENTINEL), "guard overwritten"
    assert not np.any(host[sc.GUARD: sc.GUARD + total] == sc.SENTINEL), "a sample was not written"
    return host[sc.GUARD: sc.GUARD + total].reshape(n_pos * K, n, pitch).copy()


def channel_tables(patterns, ir_len, M, room=tc.ROOM, betas=tc.BETAS, fs=tc.FS, c=sc.C_SOUND, rt60=None):
    """The knot table of every channel, (P K, n_knots)."""
    return np.stack([shoebox.tail_envelope(room, betas, ir_len, fs, min(M, ir_len), c, rt60, pattern=p)
                     for p in np.asarray(patterns, dtype=np.float64).reshape(-1, 4)])


def run_tail_abi(r, sources, positions, patterns, ir_len, M, F, seed=tc.SEED, sid0=0, cid0=0, ln_env=None, max_order=None, pitch=None,
                 room=tc.ROOM, betas=tc.BETAS, fs=tc.FS, c=sc.C_SOUND):
    """al_ism_shoebox_dir_tail into a guarded buffer: the (P K, N, pitch) rows and the (P K, n_knots) tables."""
    mem, lib = r.mem, r.lib
    sources, positions, patterns = _tables(r, sources, positions, patterns)
    n, n_pos, K = len(sources), len(positions), patterns.shape[1]
    pitch = shoebox.pitch_of(ir_len) if pitch is None else pitch
    total = n_pos * K * n * pitch
    if ln_env is None:
        ln_env = channel_tables(patterns, ir_len, M, room, betas, fs, c)
    ln_env = np.ascontiguousarray(ln_env, dtype=np.float64)
    assert ln_env.shape == (n_pos * K, shoebox.n_knots_of(ir_len))
    out = mem.upload(np.full(total + 2 * sc.GUARD, sc.SENTINEL, dtype=np.float32))
    src_dev, pos_dev, pat_dev = mem.upload(sources.reshape(-1)), mem.upload(positions.reshape(-1)), mem.upload(patterns.reshape(-1))
    env_dev = mem.upload(ln_env.reshape(-1))
    L, beta = (ct.c_double * 3)(*room), (ct.c_double * 6)(*betas)
    lib.call("al_ism_shoebox_dir_tail", mem.ptr(src_dev), n, mem.ptr(pos_dev), n_pos, mem.ptr(pat_dev), K, L, beta, float(c), float(fs),
             -1 if max_order is None else int(max_order), int(ir_len), int(pitch), int(M), int(F), int(seed), int(sid0), int(cid0),
             mem.ptr(env_dev), ln_env.shape[1], mem.ptr(out) + 4 * sc.GUARD, mem.stream())
    host = np.asarray(mem.download(out))
    assert np.all(host[:sc.GUARD] == sc.SENTINEL) and np.all(host[sc.GUARD + total:] == sc.SENTINEL), "guard overwritten"
    assert not np.any(host[sc.GUARD: sc.GUARD + total] == sc.SENTINEL), "a sample was not written"
    return host[sc.GUARD: sc.GUARD + total].reshape(n_pos * K, n, pitch).copy(), ln_env


def check_against_oracle(r, room, betas, sources, positions, patterns, ir_len, fs, c=sc.C_SOUND, max_order=None, what=None):
    rows = run_abi(r, room, betas, sources, positions, patterns, ir_len, fs, c, max_order)
    assert np.all(bits(rows[:, :, ir_len:]) == 0), "pad samples must be +0"
    y64, A, used = oracle(room, betas, sources, positions, patterns, ir_len, fs, c, max_order)
    sc.assert_within_bound(rows[:, :, :ir_len], y64, A, what)
    return rows[:, :, :ir_len], y64, A, used


# ----------------------------------------------------------------------------- 1. anechoic
def run_anechoic(r):
    room, fs, ir_len = (5.0, 4.0, 3.0), 16000.0, 700
    s, m = np.array([1.3, 2.9, 1.1]), np.array([3.7, 0.8, 1.9])
    R = s - m
    d = np.linalg.norm(R)
    u = R / d
    side = np.cross(u, (0.0, 0.0, 1.0))
    side /= np.linalg.norm(side)                      # a dipole along it sees the source side on
    sets = {"foa": shoebox.foa_patterns()[None], "mixed": mixed4()[None],
            "side-on": np.array([[shoebox.omni(), shoebox.first_order(0.0, side)]])}
    tau = d * fs / sc.C_SOUND
    t = np.arange(ir_len)
    inside = np.abs(t - tau) < sc.HALF
    assert inside.sum() in (80, 81)
    a = 1.0 / (4.0 * np.pi * d)
    x = t[inside] - tau
    taps = a * 0.5 * (1.0 + np.cos(2.0 * np.pi * x / sc.TAPS)) * np.sinc(x)
    for name, pats in sets.items():
        y, y64, A, used = check_against_oracle(r, room, np.zeros(6), s, m, pats, ir_len, fs, what=f"anechoic {name}")
        assert used[0, 0] == 1
        for k, p in enumerate(pats[0]):
            g = p[0] + p[1:] @ u
            assert np.all(bits(y[k, 0][~inside]) == 0), "everything outside the 81 taps must be exactly +0"
            assert np.abs(y[k, 0][inside] - g * taps).max() <= 2.0 ** -23 * a, (name, k)
    # (the loop's last set) the side-on dipole is zero to the bound: its oracle is 1e-17 a, its bound 2^-30 a
    assert np.abs(y[1, 0]).max() <= 2.0 ** -30 * a and np.abs(y[0, 0]).max() > 0.5 * a
    # FOA "wyzx": the four peaks are (1, uy, uz, ux) times the omni peak
    y = run_abi(r, room, np.zeros(6), s, m, sets["foa"], ir_len, fs)
    peak = int(round(tau))
    assert np.allclose(y[:, 0, peak] / y[0, 0, peak], [1.0, u[1], u[2], u[0]], rtol=0, atol=1e-6)


# ----------------------------------------------------------------------------- 2. general parity
def _parity_patterns(kind):
    """(positions, patterns (P, K, 4)) of a parity configuration."""
    foa = shoebox.foa_patterns()
    if kind == "foa-P1":
        return sc.CAPSULES_3[:1], foa[None]
    if kind == "foa-P3":
        return sc.CAPSULES_3, np.stack([foa, shoebox.foa_patterns("wxyz"), foa])
    if kind == "K2-P3":     # omni plus an oblique cardioid, another direction at every position
        dirs = (OBLIQUE, (-0.3, 0.2, 0.9), (0.7, 0.7, -0.1))
        return sc.CAPSULES_3, np.stack([np.stack([shoebox.omni(), shoebox.cardioid(v)]) for v in dirs])
    if kind == "K1-P2":     # alpha = 0.25 along OBLIQUE; a pattern with negative w
        return sc.CAPSULES_3[:2], np.stack([shoebox.first_order(0.25, OBLIQUE)[None], np.array([[-0.4, 0.3, -0.8, 0.2]])])
    raise KeyError(kind)


PARITY_KINDS = ("foa-P1", "foa-P3", "K2-P3", "K1-P2")
PARITY = ([(room, order, kind, n, 16000) for room in sc.ROOMS for order in (0, 1, 3, None) for kind in PARITY_KINDS for n in (1, 5)]
          + [("oblong", None, "foa-P1", 1, 48000)])


def run_parity(r, room, order, kind, n, fs):
    L = sc.ROOMS[room]
    src = sc.SOURCES_5 if n == 5 else sc.SOURCES_5[1:2]
    positions, patterns = _parity_patterns(kind)
    ir_len = sc.parity_ir_len(order, fs)
    y, y64, A, used = check_against_oracle(r, L, sc.UNEQUAL_BETAS, src, positions, patterns, ir_len, fs, max_order=order,
                                           what=f"{room} order={order} {kind} N={n} fs={fs}")
    if order == 0:
        assert np.all(used == 1)
    elif order is None:
        assert 100 < used.max() < 8000, used.max()
    assert np.all(np.abs(y).max(axis=2) > 0), "a channel is silent"


# ----------------------------------------------------------------------------- 3. edges
def run_edge_length(r, ir_len):
    """shoebox_cases.run_edge_length with K = 4 at both positions: row lengths around the tap count and the tile."""
    room, fs = (2.4, 2.0, 1.7), 16000.0
    src = np.array([[0.5, 0.6, 0.7], [2.0, 1.5, 1.1]])
    pos = np.array([[1.9, 1.2, 0.9], [0.52, 0.63, 0.74]])     # the second position is 5 cm from the first source
    pats = np.stack([shoebox.foa_patterns(), mixed4()])
    y, y64, A, used = check_against_oracle(r, room, (0.8, 0.7, 0.9, 0.6, 0.5, 0.95), src, pos, pats, ir_len, fs,
                                           what=f"edge ir_len={ir_len}")
    assert np.abs(y).max() > 0
    if ir_len >= 256:
        assert np.all(A[:, :, min(255, ir_len - 1)] > 0) and np.all(A[:, :, ir_len - 1] > 0)


def run_close_receiver(r):
    """A receiver 1 cm from the source: tau = 0.47 samples, the taps at t < 0 are dropped; the direct path comes from -x."""
    room, fs, ir_len = (3.0, 2.5, 2.2), 16000.0, 300
    s = np.array([1.0, 1.2, 1.1])
    m = s + np.array([0.01, 0.0, 0.0])
    y, y64, A, used = check_against_oracle(r, room, np.full(6, 0.7), s, m, shoebox.foa_patterns()[None], ir_len, fs, max_order=2,
                                           what="receiver at 1 cm")
    assert y[0, 0, 0] > 1.0 / (4 * np.pi * 0.01) * 0.5 and y[3, 0, 0] < -1.0 / (4 * np.pi * 0.01) * 0.5     # W, and X = -W


def run_crowded_tile(r):
    """shoebox_cases.run_crowded_tile with K = 4: more than 2000 images, several windows of the LDS list in the last tile."""
    room, fs, ir_len = (2.0, 1.6, 1.2), 16000.0, 600
    y, y64, A, used = check_against_oracle(r, room, (0.9, 0.95, 0.85, 0.9, 0.97, 0.8), np.array([0.7, 0.5, 0.4]),
                                           np.array([1.4, 1.1, 0.8]), shoebox.foa_patterns()[None], ir_len, fs, what="crowded tile")
    assert used[0, 0] > 2000, used
    assert (A[:, 0, 512:] > 0).all()


# ----------------------------------------------------------------------------- 4. determinism
def run_determinism(r):
    L, fs, ir_len = sc.ROOMS["oblong"], 16000.0, 520
    pats = np.stack([shoebox.foa_patterns(), mixed4(), shoebox.foa_patterns("xyzw")])
    run = lambda src, pos, p, **k: run_abi(r, L, sc.UNEQUAL_BETAS, src, pos, p, ir_len, fs, max_order=5, **k)      # noqa: E731
    one = run(sc.SOURCES_5, sc.CAPSULES_3, pats)
    assert one.shape == (12, 5, 520)
    assert np.array_equal(bits(one), bits(run(sc.SOURCES_5, sc.CAPSULES_3, pats))), "two runs differ"
    for p, n in ((0, 0), (1, 3), (2, 4)):      # a position generated alone, with one source
        alone = run(sc.SOURCES_5[n], sc.CAPSULES_3[p], pats[p:p + 1])
        assert np.array_equal(bits(alone[:, 0]), bits(one[4 * p: 4 * p + 4, n])), (p, n)
    wide = run(sc.SOURCES_5[:2], sc.CAPSULES_3[:2], pats[:2], pitch=768 + 8)
    assert np.array_equal(bits(wide[:, :, :ir_len]), bits(one[:8, :2, :ir_len])) and np.all(bits(wide[:, :, ir_len:]) == 0)
    # an omni pattern at K = 1 and the omnidirectional entry: both within the bound of the same oracle
    omni = np.tile(shoebox.omni(), (3, 1, 1))
    y64, A, _ = sc.oracle(L, sc.UNEQUAL_BETAS, sc.SOURCES_5, sc.CAPSULES_3, ir_len, fs, max_order=5)
    y64_dir, A_dir, _ = oracle(L, sc.UNEQUAL_BETAS, sc.SOURCES_5, sc.CAPSULES_3, omni, ir_len, fs, max_order=5)
    assert np.abs(y64_dir - y64).max() <= 1e-15 * np.abs(y64).max() and np.array_equal(A_dir, A)
    sc.assert_within_bound(run(sc.SOURCES_5, sc.CAPSULES_3, omni), y64, A, "omni pattern, K = 1")
    sc.assert_within_bound(sc.run_abi(r, L, sc.UNEQUAL_BETAS, sc.SOURCES_5, sc.CAPSULES_3, ir_len, fs, max_order=5), y64, A, "al_ism_shoebox")


# ----------------------------------------------------------------------------- 5. the tail
def _tail_setup(kind):
    pairs = "3x5" if kind.endswith("P3") else "1x1"
    src, pos = tc.points(pairs)
    if kind.startswith("foa"):
        pats = np.stack([shoebox.foa_patterns(), mixed4(), shoebox.foa_patterns("zyxw")])[: len(pos)]
    else:
        pats = np.stack([np.stack([shoebox.omni(), shoebox.cardioid(v)]) for v in (OBLIQUE, (-0.3, 0.2, 0.9), (0.7, 0.7, -0.1))])[: len(pos)]
    return src, pos, pats


def assert_tail_rows(rows, y64, A, ln_env, ir_len, M, F, seed, sid0, cid0, what):
    """shoebox_tail_cases.assert_rows with a table per row."""
    for c in range(rows.shape[0]):
        tc.assert_rows(rows[c:c + 1], y64[c:c + 1], A[c:c + 1], ln_env[c], ir_len, M, F, seed, sid0, cid0 + c, (what, "row", c))


#            M    F    ir_len kind      order pitch sid0        cid0
TAIL_PARITY = [(0, 1, 1100, "foa-P1", None, None, 0, 0), (0, 100, 1100, "K2-P1", None, None, 0, 0),        # M at 0
               (400, 100, 1100, "foa-P1", None, None, 0, 0), (400, 112, 1100, "K2-P1", None, None, 0, 0),     # mid-tile; M + F = 512
               (256, 100, 1100, "foa-P1", None, None, 0, 0), (256, 1, 700, "K2-P1", 1, 1024 + 8, 0, 0),       # on a tile edge
               (100, 50, 256 + 4096 + 5, "foa-P1", 1, None, 0xFFFFFFF0, 9),                                  # two k_ism_tail workgroups per row
               (400, 100, 1100, "foa-P3", None, None, 7, 3), (255, 1, 900, "K2-P3", 1, 1200, 1, 0xFFFFFFF0)]


def run_tail_parity(r, M, F, ir_len, kind, order, pitch, sid0, cid0):
    src, pos, pats = _tail_setup(kind)
    y64, A, _ = oracle(tc.ROOM, tc.BETAS, src, pos, pats, tc.Y_LEN, tc.FS, max_order=order)
    rows, ln_env = run_tail_abi(r, src, pos, pats, ir_len, M, F, sid0=sid0, cid0=cid0, max_order=order, pitch=pitch)
    assert_tail_rows(rows, y64, A, ln_env, ir_len, M, F, tc.SEED, sid0, cid0, (M, F, ir_len, kind, order, pitch))
    assert np.all(rows[:, :, M + F: ir_len] != 0.0), "a tail sample is zero"


def run_no_tail_is_the_plain_entry(r):
    """M >= ir_len: the bits of al_ism_shoebox_dir."""
    src, pos, pats = _tail_setup("foa-P3")
    ir_len = 520
    for pitch in (None, 768 + 8):
        want = run_abi(r, tc.ROOM, tc.BETAS, src, pos, pats, ir_len, tc.FS, max_order=3, pitch=pitch)
        for M, F in ((ir_len, 1), (ir_len + 1000, 7), (1 << 40, 1), ((1 << 62), (1 << 62))):
            got, _ = run_tail_abi(r, src, pos, pats, ir_len, M, F, max_order=3, pitch=pitch)
            assert np.array_equal(bits(got), bits(want)), ("a tail with mix >= ir_len differs from al_ism_shoebox_dir", M, F, pitch)


def run_tail_identity(r):
    """Rows of P = 3 made in one call equal three calls with the right id offsets; the four channels of a point draw four streams;
    two runs agree; a wider pitch moves nothing."""
    src, pos, pats = _tail_setup("foa-P3")
    ir_len, M, F, sid0, cid0 = 700, 100, 50, 7, 3
    run = lambda m=pos, p=pats, **k: run_tail_abi(r, src, m, p, ir_len, M, F, **dict(dict(sid0=sid0, cid0=cid0, max_order=2), **k))[0]   # noqa: E731
    one = run()
    assert one.shape == (12, 5, 700)
    assert np.array_equal(bits(one), bits(run())), "two runs differ"
    wide = run(pitch=1024 + 256 + 4)
    assert np.array_equal(bits(wide[:, :, :ir_len]), bits(one)) and np.all(bits(wide[:, :, ir_len:]) == 0)
    for p in range(3):
        part = run(pos[p:p + 1], pats[p:p + 1], cid0=cid0 + 4 * p)
        assert np.array_equal(bits(part), bits(one[4 * p: 4 * p + 4])), ("split call", p)
    tails = one[:, :, M + F:].reshape(60, -1)
    for a in range(60):
        for b in range(a + 1, 60):
            assert np.all(tails[a] != tails[b]), ("two rows of one call share noise", a, b)
    # the streams of the four channels of point 0 are those of capsules cid0 .. cid0 + 3: unit-envelope draws, restated
    flat = np.zeros((4, shoebox.n_knots_of(ir_len)))
    rows, _ = run_tail_abi(r, src[:1], pos[:1], pats[:1], ir_len, 0, 1, sid0=sid0, cid0=cid0, ln_env=flat, max_order=0)
    for k in range(4):
        g = tc.restated_g(tc.SEED, sid0, cid0 + k, ir_len)
        assert np.all(np.abs(rows[k, 0, 1:] - g[1:]) <= nd.RTOL * np.abs(g[1:]) + nd.ATOL + 2.0 ** -24 * np.abs(g[1:])), k


# ----------------------------------------------------------------------------- 6. envelope tables
LAW_PATTERNS = {"omni": (1.0, 0.0, 0.0, 0.0), "dipole x": (0.0, 1.0, 0.0, 0.0), "dipole y": (0.0, 0.0, 1.0, 0.0),
                "dipole z": (0.0, 0.0, 0.0, 1.0), "cardioid +x": (0.5, 0.5, 0.0, 0.0), "cardioid -z": (0.5, 0.0, 0.0, -0.5),
                "cardioid oblique": (0.5, 0.24, -0.3, 0.32), "alpha 0.25 oblique": (0.25, 0.36, -0.45, 0.48)}


def run_envelope_tables():
    ir_len, fs, M = 3000, 16000.0, 700
    for room, betas in ((tc.ROOM, tc.BETAS), ((6.0, 5.0, 3.0), (0.877,) * 6)):
        for rt60 in (None, 0.3):
            env = lambda p: shoebox.tail_envelope(room, betas, ir_len, fs, M, rt60=rt60, pattern=p)      # noqa: E731
            today = shoebox.tail_envelope(room, betas, ir_len, fs, M, rt60=rt60)
            assert np.array_equal(env(None).view(np.uint64), today.view(np.uint64))
            assert np.array_equal(env(shoebox.omni()).view(np.uint64), today.view(np.uint64)), "the omni pattern changes today's table"
            e_omni = np.exp(2.0 * today)
            dip = [np.exp(2.0 * env(shoebox.foa_patterns("wxyz")[i])) for i in (1, 2, 3)]
            if rt60 is None:      # the energies add at every knot (with rt60 they add at the mixing sample, where the lines are matched)
                assert np.abs(dip[0] + dip[1] + dip[2] - e_omni).max() <= 1e-12 * e_omni.max()
                assert np.all(np.abs(dip[0] + dip[1] + dip[2] - e_omni) <= 1e-12 * e_omni)
                for name in ("cardioid +x", "cardioid -z", "cardioid oblique", "alpha 0.25 oblique"):
                    w, vx, vy, vz = LAW_PATTERNS[name]
                    want = w * w * e_omni + vx * vx * dip[0] + vy * vy * dip[1] + vz * vz * dip[2]
                    assert np.all(np.abs(np.exp(2.0 * env(LAW_PATTERNS[name])) - want) <= 1e-12 * want), name
            else:
                law = lambda p: np.exp(shoebox.tail_energy_law(room, betas, fs, pattern=p)(M / fs))       # noqa: E731
                axes = shoebox.foa_patterns("wxyz")
                assert abs(law(axes[1]) + law(axes[2]) + law(axes[3]) - law(None)) <= 1e-12 * law(None)
                step = -(3.0 * np.log(10.0) / rt60) * 256.0 / fs
                assert np.allclose(np.diff(env(LAW_PATTERNS["cardioid oblique"])), step, rtol=0, atol=1e-12)
    # the walls of the oblong room absorb most on z: a z dipole decays faster than an x dipole there
    ism = [shoebox.tail_envelope(tc.ROOM, tc.BETAS, ir_len, fs, M, pattern=shoebox.foa_patterns("wxyz")[i]) for i in (1, 3)]
    assert ism[1][-1] - ism[1][0] < ism[0][-1] - ism[0][0]
    for bad in ((0.0, 0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (np.nan, 0.0, 0.0, 1.0)):
        with pytest.raises(ValueError):
            shoebox.tail_envelope(tc.ROOM, tc.BETAS, ir_len, fs, M, pattern=bad)


def image_rows(room, betas, s, r, patterns, ir_len, fs, c=sc.C_SOUND):
    """y64 (K, ir_len) of oracle_point, vectorised over the images (shoebox_tail_cases.image_row with the gains)."""
    reach = c * (ir_len + sc.HALF) / fs
    ax = [sc._axis(s[i], r[i], room[i], betas[2 * i], betas[2 * i + 1], reach) for i in range(3)]
    Rx, Ry, Rz = np.meshgrid(ax[0][0], ax[1][0], ax[2][0], indexing="ij")
    gain = ax[0][2][:, None, None] * ax[1][2][None, :, None] * ax[2][2][None, None, :]
    d = np.sqrt(Rx * Rx + Ry * Ry + Rz * Rz)
    tau = d * fs / c
    keep = (tau - sc.HALF < ir_len) & (gain > 0.0)
    u = np.stack([Rx[keep], Ry[keep], Rz[keep]], axis=1) / d[keep][:, None]
    d, tau, gain = d[keep], tau[keep], gain[keep]
    a = gain / (4.0 * np.pi * d)
    t = np.ceil(tau - sc.HALF)[:, None] + np.arange(sc.TAPS + 1)[None, :]
    x = t - tau[:, None]
    ok = (np.abs(x) < sc.HALF) & (t >= 0) & (t < ir_len)
    taps = a[:, None] * 0.5 * (1.0 + np.cos(2.0 * np.pi * x / sc.TAPS)) * np.sinc(x)
    index = t[ok].astype(np.int64)
    rows = []
    for p in np.asarray(patterns, dtype=np.float64):
        g = p[0] + u @ p[1:]
        rows.append(np.bincount(index, weights=(taps * g[:, None])[ok], minlength=ir_len))
    return np.array(rows)


def run_envelope_law_against_images():
    """shoebox_tail_cases.run_envelope_law_against_images through eight patterns: a sanity band on the MODEL (not a tolerance on the
    kernel), the same two rooms, four pairs, 65-sample high-pass and four windows; every ratio within a factor of 2."""
    t = np.arange(tc.LAW_LEN)
    names, pats = list(LAW_PATTERNS), np.array(list(LAW_PATTERNS.values()))
    ratios = {}
    for room_name, (room, betas) in tc.LAW_ROOMS.items():
        pts = tc.LAW_UNIT_POINTS * np.asarray(room)[None, :]
        energy = np.zeros((len(pats), tc.LAW_LEN))
        for i in range(4):
            y = image_rows(room, betas, pts[2 * i], pts[2 * i + 1], pats, tc.LAW_LEN, tc.LAW_FS)
            if i == 0:     # the vectorised sum is the oracle's
                y_ref = oracle_point(room, betas, pts[0], pts[1], pats, 300, tc.LAW_FS)[0]
                assert np.abs(y[:, :300] - y_ref).max() <= 1e-12 * np.abs(y_ref).max()
            for k in range(len(pats)):
                hp = y[k] - np.convolve(y[k], np.ones(65) / 65.0, mode="same")
                energy[k] += hp * hp / 4.0
        for k, name in enumerate(names):
            law = shoebox.tail_energy_law(room, betas, tc.LAW_FS, pattern=pats[k])
            model = np.exp([law(ti / tc.LAW_FS) for ti in t])
            got = [float(energy[k, int(a * 8): int(b * 8)].sum() / model[int(a * 8): int(b * 8)].sum()) for a, b in tc.LAW_WINDOWS_MS]
            ratios[room_name, name] = got
            print(f"directional envelope law [{room_name}, {name}]: image energy / weighted sigma^2 D in {tc.LAW_WINDOWS_MS} ms = "
                  + ", ".join(f"{v:.3f}" for v in got))
    for key, got in ratios.items():
        for v in got:
            assert 0.5 <= v <= 2.0, (key, got)
    return ratios


# ----------------------------------------------------------------------------- 7. refusals
def run_abi_refusals(r):
    mem, lib = r.mem, r.lib
    src, pos = mem.upload(np.array([1.0, 1.0, 1.0])), mem.upload(np.array([2.0, 1.5, 1.2]))
    pat = mem.upload(shoebox.foa_patterns().reshape(-1))
    out = mem.upload(np.full(4 * 32 + 32, sc.SENTINEL, dtype=np.float32))
    env = mem.upload(np.full(8, -3.0))
    good = dict(sources=mem.ptr(src), n=1, receivers=mem.ptr(pos), n_pos=1, patterns=mem.ptr(pat), K=4, L=(3.0, 2.5, 2.0), beta=(0.5,) * 6,
                c=343.0, fs=16000.0, order=-1, ir_len=30, pitch=32, mix=10, fade=5, seed=1, sid0=0, cid0=0, env=mem.ptr(env), n_knots=2,
                out=mem.ptr(out))

    def call(entry, **change):
        a = dict(good, **change)
        L = None if a["L"] is None else (ct.c_double * 3)(*a["L"])
        beta = None if a["beta"] is None else (ct.c_double * 6)(*a["beta"])
        head = (a["sources"], a["n"], a["receivers"], a["n_pos"], a["patterns"], a["K"], L, beta, a["c"], a["fs"], a["order"], a["ir_len"],
                a["pitch"])
        if entry == "al_ism_shoebox_dir":
            return lib.call(entry, *head, a["out"], mem.stream())
        return lib.call(entry, *head, a["mix"], a["fade"], a["seed"], a["sid0"], a["cid0"], a["env"], a["n_knots"], a["out"], mem.stream())

    old = [dict(L=(0.0, 2.5, 2.0)), dict(L=(3.0, 2.5, float("inf"))), dict(c=0.0), dict(c=float("nan")), dict(fs=-1.0),
           dict(beta=(0.5, 0.5, 1.01, 0.5, 0.5, 0.5)), dict(beta=(-0.01,) + (0.5,) * 5), dict(n=0), dict(n_pos=0), dict(ir_len=0),
           dict(pitch=28), dict(pitch=34, ir_len=33), dict(order=-2), dict(sources=None), dict(receivers=None), dict(out=None),
           dict(L=None), dict(beta=None)]
    new = [(dict(K=0), "n_channels must be in 1 .. 4"), (dict(K=5), "n_channels must be in 1 .. 4"), (dict(K=-1), "n_channels must be in 1 .. 4"),
           (dict(patterns=None), "null pattern table"), (dict(n_pos=(1 << 31) - 1, K=2), "more than 2^31 - 1 rows")]
    tail = [(dict(mix=-1), "mix must be >= 0"), (dict(fade=0), "fade must be >= 1"), (dict(sid0=-1), "must be >= 0"),
            (dict(cid0=-1), "must be >= 0"), (dict(sid0=1 << 32), "must not exceed 2^32"),
            (dict(cid0=(1 << 32) - 3), "must not exceed 2^32"),          # the ids run over the P K = 4 rows
            (dict(cid0=(1 << 32) - 1, K=2), "must not exceed 2^32"), (dict(n_knots=1), "n_knots must be"), (dict(n_knots=3), "n_knots must be"),
            (dict(env=None), "null envelope table"), (dict(out=mem.ptr(out) + 4), "out must be 16-byte aligned")]
    for entry in ("al_ism_shoebox_dir", "al_ism_shoebox_dir_tail"):
        for change in old:
            nd.raises_badarg(lambda: call(entry, **change), f"{entry} failed", "al_ism_shoebox: ")
        for change, needle in new:
            nd.raises_badarg(lambda: call(entry, **change), f"{entry} failed", needle)
    for change, needle in tail:
        nd.raises_badarg(lambda: call("al_ism_shoebox_dir_tail", **change), "al_ism_shoebox_tail: ", needle)
    assert np.all(np.asarray(mem.download(out)) == sc.SENTINEL), "a refused call wrote"
    assert call("al_ism_shoebox_dir") == 0 and call("al_ism_shoebox_dir_tail") == 0
    assert call("al_ism_shoebox_dir_tail", cid0=(1 << 32) - 4, sid0=(1 << 32) - 1, seed=(1 << 64) - 1, mix=0, fade=1) == 0      # the last id is valid
    assert call("al_ism_shoebox_dir", K=1) == 0 and call("al_ism_shoebox_dir_tail", K=3) == 0


def run_python_errors(r):
    room, s, m = (3.0, 2.5, 2.0), [[1.0, 1.0, 1.0]], [[2.0, 1.5, 1.2], [0.5, 0.6, 0.7]]
    ok = dict(room=room, betas=(0.5,) * 6, sources=s, capsules=m, ir_len=64, sample_rate=16000, patterns=np.tile(shoebox.foa_patterns(), (2, 1, 1)))
    nan = np.tile(shoebox.foa_patterns(), (2, 1, 1))
    nan[1, 2, 3] = np.nan
    dead = np.tile(shoebox.foa_patterns(), (2, 1, 1))
    dead[0, 1] = 0.0
    bad = [dict(patterns=shoebox.foa_patterns()), dict(patterns=np.ones((1, 4, 4))), dict(patterns=np.ones((3, 4, 4))),
           dict(patterns=np.ones((2, 4, 3))), dict(patterns=np.ones((2, 5, 4))), dict(patterns=np.ones((2, 0, 4))), dict(patterns=nan),
           dict(patterns=dead), dict(patterns="wyzx"), dict(patterns=np.ones((2, 4, 4)), tail=shoebox.ShoeboxTail(), capsule_id0=(1 << 32) - 7)]
    for change in bad:
        with pytest.raises(ValueError):
            shoebox.shoebox_irs_device(r, **dict(ok, **change))
    buf, strides, n = shoebox.shoebox_irs_device(r, **ok)
    assert strides == (64, 64) and n == 64 and len(np.asarray(r.mem.download(buf))) >= 8 * 64
    shoebox.shoebox_irs_device(r, **dict(ok, tail=shoebox.ShoeboxTail(), capsule_id0=(1 << 32) - 8))
    for call in (lambda: shoebox.first_order(0.5, (0.0, 0.0, 0.0)), lambda: shoebox.first_order(0.5, (1.0, 0.0)),
                 lambda: shoebox.first_order(np.nan, (1.0, 0.0, 0.0)), lambda: shoebox.first_order(0.5, (np.inf, 0.0, 0.0)),
                 lambda: shoebox.cardioid((0.0, 0.0, 0.0)), lambda: shoebox.foa_patterns("wxy"), lambda: shoebox.foa_patterns("wxyy"),
                 lambda: shoebox.foa_patterns("acn"), lambda: shoebox.foa_patterns(None), lambda: shoebox.foa_patterns("wxyzw")):
        with pytest.raises(ValueError):
            call()
    assert np.array_equal(shoebox.omni(), [1.0, 0.0, 0.0, 0.0])
    assert np.allclose(shoebox.first_order(0.25, (0.0, 3.0, -4.0)), [0.25, 0.0, 0.45, -0.6], rtol=0, atol=1e-16)
    assert np.array_equal(shoebox.cardioid((0.0, 0.0, -2.0)), [0.5, 0.0, 0.0, -0.5])
    assert np.array_equal(shoebox.foa_patterns(), [[1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [0, 1, 0, 0]])      # AmbiX: W, Y, Z, X
    assert np.array_equal(shoebox.foa_patterns("WXYZ"), np.eye(4))
    st = core.ShoeboxIRState(room, betas=(0.5,) * 6, ir_len=64, sample_rate=16000, renderer=r)
    for call in (lambda: st.add_microphone("a", m, patterns=np.ones((3, 4))), lambda: st.add_microphone("a", m, patterns=np.ones((2, 3))),
                 lambda: st.add_microphone("a", m, patterns=np.zeros((2, 4))), lambda: st.add_microphone("a", m, patterns=np.ones((2, 1, 4))),
                 lambda: st.add_microphone("a", m, capsule_names=["one"]),
                 lambda: st.add_microphone("a", m, patterns=np.ones((2, 4)), capsule_names=["l", "r", "c"]),
                 lambda: st.add_foa_listener("a", m[0], order="wxy"), lambda: st.add_foa_listener("a", m),
                 lambda: st.add_foa_listener("a", [4.0, 1.0, 1.0])):
        with pytest.raises(ValueError):
            call()
    assert len(st.microphones) == 0


# ----------------------------------------------------------------------------- 8. the state and the scene
DIR_MIC = np.array([[2.0, 1.6, 1.2], [2.05, 1.6, 1.2]])
FOA_POINT = np.array([1.31, 1.42, 1.2])


def _dir_patterns():
    return np.array([shoebox.cardioid((-1.0, 0.0, 0.0)), shoebox.first_order(0.25, OBLIQUE)])


def _state(r, tail=None, ir_len=520, max_order=3, betas=tc.BETAS, order="wyzx"):
    st = core.ShoeboxIRState(tc.ROOM, betas=betas, ir_len=ir_len, sample_rate=sc.SR, max_order=max_order, renderer=r, tail=tail)
    st.add_microphone("dir", DIR_MIC, patterns=_dir_patterns(), capsule_names=["left", "right"])
    st.add_foa_listener("foa", FOA_POINT, order=order)
    st.add_emitters([[0.8, 0.9, 1.0]], alias="static")
    st.add_emitters(np.linspace([3.2, 0.6, 1.5], [3.4, 2.8, 1.1], 3), alias="moving")
    return st


def run_state(r):
    st = _state(r, order="wxyz")
    mic, foa = st.microphones["dir"], st.microphones["foa"]
    assert (mic.n_capsules, mic.n_listeners, mic.metadata["capsule_names"]) == (2, 2, ["left", "right"])
    assert (foa.n_capsules, foa.n_listeners, foa.metadata["capsule_names"]) == (4, 1, ["w", "x", "y", "z"])
    assert foa.metadata["micarray_type"] == "FOAListener" and foa.metadata["channel_layout_type"] == "foa"
    assert foa.metadata["coordinates_absolute"] == [FOA_POINT.tolist()]
    st.simulate()
    sources = st.emitter_positions
    t_dir, t_foa = st.irs["dir"], st.irs["foa"]
    assert t_dir.shape == (2, 4, 520) and t_foa.shape == (4, 4, 520) and isinstance(t_foa, shoebox.DeviceIRTensor)
    y64, A, _ = oracle(tc.ROOM, tc.BETAS, sources, DIR_MIC, _dir_patterns()[:, None, :], 520, float(sc.SR), max_order=3)
    sc.assert_within_bound(np.asarray(t_dir), y64, A, "state, directional microphone")
    y64, A, _ = oracle(tc.ROOM, tc.BETAS, sources, FOA_POINT, shoebox.foa_patterns("wxyz")[None], 520, float(sc.SR), max_order=3)
    sc.assert_within_bound(np.asarray(t_foa), y64, A, "state, FOA listener")
    # JSON round trip: one coordinate row serves the listener's four channels
    d = json.loads(json.dumps(st.to_dict()))
    assert d["microphones"]["foa"]["n_capsules"] == 4 and len(d["microphones"]["foa"]["coordinates_absolute"]) == 1
    assert d["microphones"]["foa"]["patterns"] == np.eye(4).tolist() and d["microphones"]["dir"]["patterns"] == _dir_patterns().tolist()
    assert core.ShoeboxIRState.describes(d)
    again = core.ShoeboxIRState.from_dict(d, renderer=r)
    for alias in ("dir", "foa"):
        a, b = again.microphones[alias], st.microphones[alias]
        assert (a.n_capsules, a.n_listeners) == (b.n_capsules, b.n_listeners)
        assert {k: v for k, v in a.metadata.items() if k != "name"} == b.metadata
    assert json.loads(json.dumps(again.to_dict())) == d
    again.simulate()
    for alias in ("dir", "foa"):
        assert np.array_equal(bits(np.asarray(again.irs[alias])), bits(np.asarray(st.irs[alias]))), alias
    # a dictionary without patterns loads as today: omnidirectional capsules, the plain entry's bits
    for md in d["microphones"].values():
        md.pop("patterns"), md.pop("capsule_names")
    plain = core.ShoeboxIRState.from_dict(d, renderer=r)
    assert plain.microphones["foa"].n_capsules == 1 and plain._patterns == {"dir": None, "foa": None}
    plain.simulate()
    want = sc.run_abi(r, tc.ROOM, tc.BETAS, sources, DIR_MIC, 520, sc.SR, max_order=3)
    assert np.array_equal(bits(np.asarray(plain.irs["dir"])), bits(want[:, :, :520]))
    # with a tail: channels are numbered through the microphones (dir: 0, 1; foa: 2 .. 5), each under its own pattern's envelope
    tailed = _state(r, tail=tc.STATE_TAIL, ir_len=900, max_order=None)
    tailed.simulate()
    M, F = shoebox.tail_samples(tailed.tail, tc.ROOM, sc.SR)
    for alias, pos, pats, cid0 in (("dir", DIR_MIC, _dir_patterns()[:, None, :], 0), ("foa", FOA_POINT, shoebox.foa_patterns()[None], 2)):
        y64, A, _ = oracle(tc.ROOM, tc.BETAS, sources, pos, pats, tc.Y_LEN, float(sc.SR))
        ln_env = channel_tables(pats, 900, M, fs=float(sc.SR))
        assert_tail_rows(np.asarray(tailed.irs[alias]), y64, A, ln_env, 900, M, F, tc.STATE_TAIL["seed"], 0, cid0, f"state tail {alias}")


def run_end_to_end(r, monkeypatch, tmp_path):
    """A static and a moving event on a state with a directional microphone and an FOA listener: rendered with every host-to-device
    path of an IR tensor patched to raise, equal bit for bit to the same scene on StaticIRState(np.asarray(tensor)) and to the scene
    rebuilt from its JSON."""
    state = _state(r, ir_len=1203, max_order=4, betas=(0.8, 0.9, 0.75, 0.85, 0.6, 0.7))
    scene = sc._add_events(core.Scene(1.2, state, sample_rate=sc.SR))

    def refuse(*a, **k):
        raise AssertionError("an IR tensor went through the host")

    real_upload = engine.Renderer.upload_irs
    monkeypatch.setattr(engine.Renderer, "upload_irs", refuse)
    got = sc._render(scene)
    assert all(t._host is None for t in state.irs.values()), "the render downloaded an IR tensor"
    path = tmp_path / "shoebox_directional_scene.json"
    scene.to_json(str(path))
    clips = {a: e._raw for a, e in scene.events.items()}
    again = core.Scene.from_json(str(path), clips)
    assert isinstance(again.state, core.ShoeboxIRState) and again.state.microphones["foa"].n_capsules == 4
    again.state.renderer = r
    got_again = sc._render(again)
    monkeypatch.setattr(engine.Renderer, "upload_irs", real_upload)

    host = {alias: np.asarray(t) for alias, t in state.irs.items()}
    want = sc._render(sc._add_events(core.Scene(1.2, core.StaticIRState(host), sample_rate=sc.SR)))
    assert want["foa"].shape == (4, round(1.2 * sc.SR)) and want["dir"].shape == (2, round(1.2 * sc.SR))
    for alias in ("dir", "foa"):
        assert np.abs(want[alias]).max() > 0
        assert np.array_equal(bits(got[alias]), bits(want[alias])), alias
        assert np.array_equal(bits(got_again[alias]), bits(want[alias])), alias


def run_direction_end_to_end(r):
    """No reflections, one static event, an AmbiX listener: x / w, y / w and z / w of the rendered scene are the direction cosines
    of the source (the render's parity contract is 1e-4 relative per channel and the level law one scalar per event, so the
    ratios survive to about 3e-4: 1e-3 leaves a margin and is far below any wrong axis, sign or channel order)."""
    st = core.ShoeboxIRState(tc.ROOM, betas=(0.0,) * 6, ir_len=400, sample_rate=sc.SR, renderer=r)
    source = np.array([0.8, 2.9, 0.6])
    st.add_foa_listener("foa", FOA_POINT, order="wyzx")
    st.add_emitters([source], alias="static")
    scene = core.Scene(0.6, st, sample_rate=sc.SR)
    scene.add_event(core.Event("static", sc._clip(6000, 1), sc.SR, snr=12.0, scene_start=0.1, n_emitters=1))
    audio = sc._render(scene)["foa"].astype(np.float64)
    u = (source - FOA_POINT) / np.linalg.norm(source - FOA_POINT)
    w = audio[0]
    assert (w * w).sum() > 0
    for channel, axis in ((1, 1), (2, 2), (3, 0)):      # W Y Z X
        ratio = float((audio[channel] * w).sum() / (w * w).sum())
        print(f"direction end to end: channel {channel} / W = {ratio:.6f}, direction cosine {u[axis]:.6f}")
        assert abs(ratio - u[axis]) <= 1e-3, (channel, ratio, u[axis])
