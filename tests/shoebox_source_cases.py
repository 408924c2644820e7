"""Scenarios of the directional sources and the air absorption of the device shoebox IR generator (al_ism_shoebox_src,
al_ism_shoebox_bands_src, shoebox.shoebox_irs_device(source_patterns=..., air=...), shoebox.air_absorption,
core.ShoeboxIRState(air=...).add_emitters(patterns=...)) and the float64 numpy restatement of their definition (DESIGN.md "Shoebox IRs:
directional sources and air"; no reference code computes this).  tests/test_hostemu_shoebox_source.py runs them on the host-emulated
kernels, tests/test_gpu_shoebox_source.py on the gfx950 build.

THE DEFINITION.  Everything of shoebox_cases, shoebox_tail_cases, shoebox_directional_cases and shoebox_bands_cases stands.  Image
(qx, qy, qz), q_i = 2 m_i - p_i, with offset R (image minus receiver), d = |R|, u = R / d: the ray leaves the real source along e,
e_i = -(-1)^{q_i} u_i = -(1 - 2 p_i) u_i.  Source n has spat[n] = (w, vx, vy, vz) and the gain gs = w + v . e; the call has an air
coefficient m >= 0 in Np/m (the band entry one m_b per band).  The amplitude of the image in row c is a gs exp(-m d) gr_c, gr_c the
receiver's w + v . u (1 for an omni capsule); in the band entry the image of band b carries a_b gs exp(-m_b d).  With a tail the pair
(row c, source n) reads the knot table ln_env[c, n], in the band entry (source n, band b) the table ln_env[n, b].

THE BOUND (derived as shoebox_cases' and shoebox_directional_cases' are, not tuned), every sample, none excluded:
    |y - y64| <= 2^-24 |y64| + 2^-30 A[t],   A[t] = sum over the images with a tap at t of |a| exp(-m d) (|ws| + |vs|_2) (|wr| + |vr|_2).
|ws + vs . e| <= |ws| + |vs|_2 for a unit e, so A sums the largest magnitude each tap can have and does not shrink where a gain
cancels.  Beside what shoebox_cases' budget holds (float64 tau against a tap slope of about pi, libm differences in the tap), the new
work per image is one dot product of three terms (three roundings of 2^-53 (|ws| + |vs|_2) on gs, as the receiver's), two
multiplications (2^-53 relative each) and one exp whose argument sum k ln beta - m d is formed with one more rounding: with
|sum k ln beta - m d| < 745 (else the image is below the float64 range) that is 745 * 2^-53 = 2^-43.5 relative on the amplitude, at
most thirteen binary orders below 2^-30.  The band and tail bounds are shoebox_bands_cases' and shoebox_tail_cases' with A so widened.
"""
import ctypes as ct
import functools
import json

import numpy as np
import pytest
from scipy import sparse

from audiblelight_amd import core, shoebox
from tests import noise_draw_cases as nd
from tests import shoebox_bands_cases as bc
from tests import shoebox_cases as sc
from tests import shoebox_directional_cases as dc
from tests import shoebox_tail_cases as tc

bits = sc.bits
FS = 16000.0
AIR = 3.4e-3                                     # Np/m: the air at 4 kHz, 20 degrees and 50 % (29.7 dB/km)
LAW = dc.LAW_PATTERNS
# a different pattern per source of SOURCES_5: the three dipoles, the oblique cardioid, alpha = 0.25
SPATS_5 = np.array([LAW["dipole x"], LAW["dipole y"], LAW["dipole z"], LAW["cardioid oblique"], LAW["alpha 0.25 oblique"]])
OMNI_5 = np.tile(shoebox.omni(), (5, 1))
WORST = {"fraction": 0.0}


def rising_air(n_bands):
    """An air coefficient per band, rising about as f^2 does from band to band and reaching AIR in the top one."""
    return AIR * 4.0 ** (np.arange(n_bands) - (n_bands - 1.0))


def _norm(p):
    p = np.asarray(p, dtype=np.float64)
    return np.abs(p[..., 0]) + np.sqrt((p[..., 1:] ** 2).sum(axis=-1))


# ----------------------------------------------------------------------------- the restatement: the definition, in float64
def images(room, s, r, hi, fs, c, max_order):
    """Every image of source s at receiver r with a tap below sample hi, of order <= max_order: (R (n, 3), d, tau, sign (n, 3) =
    (-1)^q per axis, k (n, 6): the reflections by the walls x0, x1, y0, y1, z0, z1)."""
    reach = c * (hi + sc.HALF) / fs
    ax = []
    for i in range(3):
        M = int(np.ceil(reach / room[i])) + 1
        m, p = np.repeat(np.arange(-M, M + 1), 2), np.tile(np.array([0, 1]), 2 * M + 1)
        ax.append(((1 - 2 * p) * s[i] + 2.0 * m * room[i] - r[i], np.abs(m - p), np.abs(m), 1 - 2 * p))
    grid = lambda j: [v.ravel() for v in np.meshgrid(ax[0][j], ax[1][j], ax[2][j], indexing="ij")]      # noqa: E731
    Rx, Ry, Rz = grid(0)
    k0, k1, sign = grid(1), grid(2), np.stack(grid(3), axis=1)
    d = np.sqrt(Rx * Rx + Ry * Ry + Rz * Rz)
    tau = d * fs / c
    k = np.stack([k0[0], k1[0], k0[1], k1[1], k0[2], k1[2]], axis=1)
    keep = tau - sc.HALF < hi
    if max_order is not None:
        keep &= k.sum(axis=1) <= max_order
    return np.stack([Rx, Ry, Rz], axis=1)[keep], d[keep], tau[keep], sign[keep], k[keep]


def source_gain(spat, sign, u):
    """gs = w + v . e of every image, e_i = -(-1)^{q_i} u_i; None: 1."""
    if spat is None:
        return np.ones(len(u))
    spat = np.asarray(spat, dtype=np.float64)
    return spat[0] + (-sign * u) @ spat[1:]


def pair_rows(room, beta, air, s, r, spat, rpats, lo, hi, fs, c=sc.C_SOUND, max_order=None):
    """(y, A, n_images) of one source at one receiver position, y and A of shape (B, K, hi - lo) with index i at sample lo + i:
    beta (6, B) with air (B,) (B = 1: a broadband call), rpats (K, 4) or None (an omni capsule, K = 1)."""
    beta, air = np.asarray(beta, dtype=np.float64).reshape(6, -1), np.asarray(air, dtype=np.float64).reshape(-1)
    R, d, tau, sign, k = images(room, s, r, hi, fs, c, max_order)
    u = R / d[:, None]
    gs = source_gain(spat, sign, u)
    ws = 1.0 if spat is None else _norm(spat)
    if rpats is None:
        gr, wr = np.ones((len(d), 1)), np.ones(1)
    else:
        rpats = np.asarray(rpats, dtype=np.float64).reshape(-1, 4)
        gr, wr = rpats[None, :, 0] + u @ rpats[:, 1:].T, _norm(rpats)
    t = np.ceil(tau - sc.HALF)[:, None] + np.arange(sc.TAPS + 1)[None, :]
    x = t - tau[:, None]
    ok = (np.abs(x) < sc.HALF) & (t >= lo) & (t < hi)
    shape = 0.5 * (1.0 + np.cos(2.0 * np.pi * x / sc.TAPS)) * np.sinc(x)
    B, K = beta.shape[1], gr.shape[1]
    y, A = np.zeros((B, K, hi - lo)), np.zeros((B, K, hi - lo))
    used = 0
    for b in range(B):
        with np.errstate(divide="ignore"):
            gain = np.prod(beta[None, :, b] ** k, axis=1)                 # numpy: 0.0 ** 0 == 1.0
        a = gain / (4.0 * np.pi * d) * np.exp(-air[b] * d)
        live = ok & (gain > 0.0)[:, None]                                 # a wall of beta = 0 in its path: no image in this band
        used = max(used, int(live.any(axis=1).sum()))
        idx = (t[live] - lo).astype(np.int64)
        for kk in range(K):
            y[b, kk] = np.bincount(idx, weights=((a * gs * gr[:, kk])[:, None] * shape)[live], minlength=hi - lo)
            A[b, kk] = np.bincount(idx, weights=np.broadcast_to((np.abs(a) * ws * wr[kk])[:, None], t.shape)[live], minlength=hi - lo)
    return y, A, used


_t = lambda v: None if v is None else tuple(float(x) for x in np.ravel(v))                               # noqa: E731
_pts = lambda v: tuple(tuple(float(x) for x in row) for row in np.atleast_2d(v))                         # noqa: E731
_pat3 = lambda v: None if v is None else tuple(tuple(tuple(float(x) for x in ch) for ch in pos) for pos in np.asarray(v, dtype=np.float64))  # noqa: E731


@functools.lru_cache(maxsize=None)
def _oracle_cached(room, betas, air, sources, spats, positions, rpats, ir_len, fs, c, max_order):
    P, N = len(positions), len(sources)
    K = 1 if rpats is None else len(rpats[0])
    y, A, used = np.zeros((P * K, N, ir_len)), np.zeros((P * K, N, ir_len)), np.zeros((P, N), dtype=np.int64)
    for p in range(P):
        for n in range(N):
            yy, AA, used[p, n] = pair_rows(room, betas, [air], sources[n], positions[p], None if spats is None else spats[n],
                                           None if rpats is None else rpats[p], 0, ir_len, fs, c, max_order)
            y[p * K:(p + 1) * K, n], A[p * K:(p + 1) * K, n] = yy[0], AA[0]
    for arr in (y, A, used):
        arr.flags.writeable = False
    return y, A, used


def oracle(room, betas, air, sources, spats, positions, rpats, ir_len, fs, c=sc.C_SOUND, max_order=None):
    """(y64, A) of shape (P K, N, ir_len) and the image counts (P, N) of al_ism_shoebox_src; computed once per scenario and shared
    (read-only).  spats (N, 4) or None, rpats (P, K, 4) or None."""
    return _oracle_cached(_t(room), _t(betas), float(air), _pts(sources), None if spats is None else _pts(spats), _pts(positions),
                          _pat3(rpats), int(ir_len), float(fs), float(c), max_order)


def _band_image_part(room, beta, air, phi, half, s, r, spat, y_end, fs, c, max_order):
    """(sum_b phi_b * y_b, sum_b |phi_b| * A_b) at t in [0, y_end) of one pair."""
    y, A, _ = pair_rows(room, beta, air, s, r, spat, None, -half, y_end + half, fs, c, max_order)
    img = sum(np.convolve(y[b, 0], phi[b])[2 * half: 2 * half + y_end] for b in range(len(phi)))
    spread = sum(np.convolve(A[b, 0], np.abs(phi[b]))[2 * half: 2 * half + y_end] for b in range(len(phi)))
    return img, spread


@functools.lru_cache(maxsize=None)
def _restate_bands_cached(room, beta, n_bands, air, centres, half, sources, spats, capsules, ir_len, fs, c, max_order):
    beta = np.array(beta).reshape(6, n_bands)
    phi = shoebox.band_filters(centres, fs, half)
    h, bound = np.zeros((len(capsules), len(sources), ir_len)), np.zeros((len(capsules), len(sources), ir_len))
    for ci in range(len(capsules)):
        for ni in range(len(sources)):
            h[ci, ni], bound[ci, ni] = _band_image_part(room, beta, air, phi, half, sources[ni], capsules[ci],
                                                        None if spats is None else spats[ni], ir_len, fs, c, max_order)
    bound = 2.0 ** -24 * np.abs(h) + 2.0 ** -30 * bound
    h.flags.writeable = bound.flags.writeable = False
    return h, bound


def restate_bands(room, beta, air, centres, half, sources, spats, capsules, ir_len, fs, c=sc.C_SOUND, max_order=None):
    """(h64, bound) of shape (C, N, ir_len) of al_ism_shoebox_bands_src without a tail (shoebox_bands_cases.restate with the two
    factors)."""
    beta = np.asarray(beta, dtype=np.float64)
    return _restate_bands_cached(_t(room), tuple(beta.reshape(-1)), beta.shape[1], _t(air), _t(centres), int(half), _pts(sources),
                                 None if spats is None else _pts(spats), _pts(capsules), int(ir_len), float(fs), float(c), max_order)


def restate_bands_tail(room, beta, air, centres, half, sources, spats, capsules, ir_len, fs, M, F, ln_env, seed, sid0, cid0, c=sc.C_SOUND,
                       max_order=None):
    """(h64, bound) of al_ism_shoebox_bands_src with a tail: shoebox_bands_cases.restate_tail with the two factors in the image
    part and the knot tables ln_env (N, B, n_knots) of source n."""
    beta, ln_env = np.asarray(beta, dtype=np.float64), np.asarray(ln_env, dtype=np.float64)
    sources, capsules = np.atleast_2d(sources), np.atleast_2d(capsules)
    n_bands, n_taps = beta.shape[1], 2 * half + 1
    phi = shoebox.band_filters(centres, fs, half)
    y_end = min(ir_len, M + F)
    w_e, w_l = tc.weights(ir_len, M, F)
    t = np.arange(ir_len)
    k, p = t // 256, (t % 256) / 256.0
    lerp = lambda table: np.where(p == 0.0, table[k, t], (1.0 - p) * table[k, t] + p * table[np.minimum(k + 1, len(table) - 1), t])   # noqa: E731
    fir = lambda x, taps: np.convolve(x, taps)[half: half + ir_len]                                       # noqa: E731
    h, bound = np.zeros((len(capsules), len(sources), ir_len)), np.zeros((len(capsules), len(sources), ir_len))
    for ni in range(len(sources)):
        with np.errstate(over="ignore"):
            e = np.exp(ln_env[ni])                                         # (B, n_knots)
        psi = np.einsum("bk,bj->kj", e, phi)
        for ci in range(len(capsules)):
            img, img_bound = np.zeros(ir_len), np.zeros(ir_len)
            img[:y_end], img_bound[:y_end] = _band_image_part(room, beta, air, phi, half, sources[ni], capsules[ci],
                                                              None if spats is None else spats[ni], y_end, fs, c, max_order)
            g = tc.restated_g(seed, sid0 + ni, cid0 + ci, ir_len)
            tol = nd.RTOL * np.abs(g) + nd.ATOL
            noise = lerp(np.stack([fir(g, psi[kk]) for kk in range(len(psi))]))
            draw = lerp(np.stack([fir(tol, np.abs(psi[kk])) for kk in range(len(psi))]))
            spread = np.stack([fir(np.abs(g), np.abs(phi[b])) for b in range(n_bands)])
            accum = (n_taps + n_bands + 16) * 2.0 ** -53 * lerp(np.einsum("bk,bt->kt", e, spread))
            h[ci, ni] = w_e * img + np.where(w_l > 0.0, w_l * noise, 0.0)
            bound[ci, ni] = (w_e * 2.0 ** -30 * img_bound + np.where(w_l > 0.0, w_l * (draw + accum), 0.0) + 2.0 ** -24 * np.abs(h[ci, ni])
                             + 2.0 ** -150)
    return h, bound


def assert_within(rows, y64, bound, what):
    rows = np.asarray(rows, dtype=np.float64)
    assert np.all(np.isfinite(rows)), what
    err = np.abs(rows - y64)
    frac = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)))
    WORST["fraction"] = max(WORST["fraction"], frac)
    print(f"shoebox source bound [{what}]: max err {err.max():.3e}, max err / bound {frac:.3f} (so far {WORST['fraction']:.3f})")
    assert np.all(err <= bound), (what, "err / bound", frac, "at", np.unravel_index(np.argmax(err - bound), err.shape))


def assert_tail_rows(rows, y64, A, ln_env, ir_len, M, F, seed, sid0, cid0, what):
    """shoebox_tail_cases.assert_rows with a knot table per (row, source): ln_env (rows, N, n_knots)."""
    for c in range(rows.shape[0]):
        for n in range(rows.shape[1]):
            tc.assert_rows(rows[c:c + 1, n:n + 1], y64[c:c + 1, n:n + 1], A[c:c + 1, n:n + 1], ln_env[c, n], ir_len, M, F, seed, sid0 + n,
                           cid0 + c, (what, "row", c, "source", n))
    WORST["fraction"] = max(WORST["fraction"], tc.WORST["fraction"])


# ----------------------------------------------------------------------------- running the entry points
def _dev(mem, arr):
    return None if arr is None else mem.upload(np.ascontiguousarray(arr, dtype=np.float64).reshape(-1))


def _ptr(mem, buf):
    return None if buf is None else mem.ptr(buf)


def _guarded(mem, total):
    return mem.upload(np.full(total + 2 * sc.GUARD, sc.SENTINEL, dtype=np.float32))


def _unguard(mem, out, total, shape):
    host = np.asarray(mem.download(out))
    assert np.all(host[:sc.GUARD] == sc.SENTINEL) and np.all(host[sc.GUARD + total:] == sc.SENTINEL), "guard overwritten"
    assert not np.any(host[sc.GUARD: sc.GUARD + total] == sc.SENTINEL), "a sample was not written"
    return host[sc.GUARD: sc.GUARD + total].reshape(shape).copy()


def run_src(r, room, betas, sources, spats, positions, rpats, air, ir_len, fs, c=sc.C_SOUND, max_order=None, pitch=None, tail=None):
    """al_ism_shoebox_src into a buffer with sc.GUARD sentinels on either side: the (P K, N, pitch) rows, the guards checked.
    spats (N, 4) or None; rpats (P, K, 4) or None (omni capsules); tail: None (mix = -1) or a dictionary M, F, ln_env (rows, N,
    n_knots) and optionally seed, sid0, cid0."""
    mem, lib = r.mem, r.lib
    sources = np.ascontiguousarray(np.atleast_2d(sources), dtype=np.float64)
    positions = np.ascontiguousarray(np.atleast_2d(positions), dtype=np.float64)
    n, n_pos = len(sources), len(positions)
    K = 1 if rpats is None else np.asarray(rpats).shape[1]
    pitch = shoebox.pitch_of(ir_len) if pitch is None else pitch
    total = n_pos * K * n * pitch
    out = _guarded(mem, total)
    src_dev, pos_dev, spat_dev, pat_dev = _dev(mem, sources), _dev(mem, positions), _dev(mem, spats), _dev(mem, rpats)
    t = dict(M=-1, F=0, seed=tc.SEED, sid0=0, cid0=0, ln_env=None)
    t.update(tail or {})
    if t["ln_env"] is not None:
        assert np.shape(t["ln_env"]) == (n_pos * K, n, shoebox.n_knots_of(ir_len)), np.shape(t["ln_env"])
    env_dev = _dev(mem, t["ln_env"])
    L, beta = (ct.c_double * 3)(*room), (ct.c_double * 6)(*betas)
    lib.call("al_ism_shoebox_src", mem.ptr(src_dev), n, _ptr(mem, spat_dev), mem.ptr(pos_dev), n_pos, _ptr(mem, pat_dev), K, L, beta,
             float(air), float(c), float(fs), -1 if max_order is None else int(max_order), int(ir_len), int(pitch), int(t["M"]), int(t["F"]),
             int(t["seed"]), int(t["sid0"]), int(t["cid0"]), _ptr(mem, env_dev), 0 if t["ln_env"] is None else np.shape(t["ln_env"])[2],
             mem.ptr(out) + 4 * sc.GUARD, mem.stream())
    return _unguard(mem, out, total, (n_pos * K, n, pitch))


def run_bands_src(r, room, beta, centres, half, sources, spats, capsules, air, ir_len, fs, c=sc.C_SOUND, max_order=None, pitch=None,
                  pairs_per_pass=None, tail=None):
    """al_ism_shoebox_bands_src as shoebox_bands_cases.run_bands_abi runs the old entry: guarded output, a workspace of exactly
    pairs_per_pass pairs (None: all) with a guard behind it.  tail: as run_src, ln_env (N, B, n_knots)."""
    mem, lib = r.mem, r.lib
    sources = np.ascontiguousarray(np.atleast_2d(sources), dtype=np.float64)
    capsules = np.ascontiguousarray(np.atleast_2d(capsules), dtype=np.float64)
    beta = np.ascontiguousarray(beta, dtype=np.float64)
    air = np.ascontiguousarray(np.broadcast_to(np.asarray(air, dtype=np.float64), (beta.shape[1],)))
    n, n_cap, n_bands = len(sources), len(capsules), beta.shape[1]
    pitch = shoebox.pitch_of(ir_len) if pitch is None else pitch
    total = n_cap * n * pitch
    t = dict(M=-1, F=0, seed=bc.SEED, sid0=0, cid0=0, ln_env=None)
    t.update(tail or {})
    if t["ln_env"] is not None:
        assert np.shape(t["ln_env"]) == (n, n_bands, shoebox.n_knots_of(ir_len)), np.shape(t["ln_env"])
    per_pair = bc.per_pair_bytes(r, n_bands, half, ir_len, t["M"], t["F"])
    ws_bytes = per_pair * (n * n_cap if pairs_per_pass is None else pairs_per_pass)
    ws = mem.upload(np.full(ws_bytes // 8 + sc.GUARD, 7.5, dtype=np.float64))
    out = _guarded(mem, total)
    src_dev, cap_dev, spat_dev = _dev(mem, sources), _dev(mem, capsules), _dev(mem, spats)
    phi_dev, env_dev = _dev(mem, shoebox.band_filters(centres, fs, half)), _dev(mem, t["ln_env"])
    lib.call("al_ism_shoebox_bands_src", mem.ptr(src_dev), n, _ptr(mem, spat_dev), mem.ptr(cap_dev), n_cap, (ct.c_double * 3)(*room),
             beta.ctypes.data_as(ct.POINTER(ct.c_double)), n_bands, mem.ptr(phi_dev), int(half), air.ctypes.data_as(ct.POINTER(ct.c_double)),
             float(c), float(fs), -1 if max_order is None else int(max_order), int(ir_len), int(pitch), int(t["M"]), int(t["F"]),
             int(t["seed"]), int(t["sid0"]), int(t["cid0"]), _ptr(mem, env_dev), 0 if t["ln_env"] is None else np.shape(t["ln_env"])[2],
             mem.ptr(ws), ws_bytes, mem.ptr(out) + 4 * sc.GUARD, mem.stream())
    assert np.all(np.asarray(mem.download(ws))[ws_bytes // 8:] == 7.5), "the workspace's guard was overwritten"
    return _unguard(mem, out, total, (n_cap, n, pitch))


def check_src(r, room, betas, sources, spats, positions, rpats, air, ir_len, fs, max_order=None, what=None):
    rows = run_src(r, room, betas, sources, spats, positions, rpats, air, ir_len, fs, max_order=max_order)
    assert np.all(bits(rows[:, :, ir_len:]) == 0), "pad samples must be +0"
    y64, A, used = oracle(room, betas, air, sources, spats, positions, rpats, ir_len, fs, max_order=max_order)
    assert_within(rows[:, :, :ir_len], y64, 2.0 ** -24 * np.abs(y64) + 2.0 ** -30 * A, what)
    return rows[:, :, :ir_len], y64, A, used


def check_bands_src(r, room, beta, centres, half, sources, spats, capsules, air, ir_len, fs, max_order=None, what=None, **kw):
    rows = run_bands_src(r, room, beta, centres, half, sources, spats, capsules, air, ir_len, fs, max_order=max_order, **kw)
    assert np.all(bits(rows[:, :, ir_len:]) == 0), "pad samples must be +0"
    h64, bound = restate_bands(room, beta, np.broadcast_to(np.asarray(air, dtype=np.float64), (np.shape(beta)[1],)), centres, half, sources,
                               spats, capsules, ir_len, fs, max_order=max_order)
    assert_within(rows[:, :, :ir_len], h64, bound, what)
    return rows[:, :, :ir_len], h64


# ----------------------------------------------------------------------------- 1. parity with the restatement
def _receivers(kind):
    """(positions, rpats) of a broadband parity configuration."""
    if kind == "omni":
        return sc.CAPSULES_3, None
    if kind == "K1":      # a cardioid per position, another direction at each
        return sc.CAPSULES_3, np.stack([shoebox.cardioid(v)[None] for v in (dc.OBLIQUE, (-0.3, 0.2, 0.9), (0.7, 0.7, -0.1))])
    if kind == "foa":
        return sc.CAPSULES_3, np.stack([shoebox.foa_patterns(), shoebox.foa_patterns("wxyz"), dc.mixed4()])
    raise KeyError(kind)


PARITY = ([(room, order, kind, air) for room in sc.ROOMS for order in (0, 1, 3, None) for kind in ("omni", "K1", "foa") for air in ("0", "m")]
          + [(room, order, kind, air) for room in sc.ROOMS for order in (0, 1, 3, None) for kind in ("B3", "B5") for air in ("0", "m", "rising")])


def parity_ir_len(order):
    # no order limit: some 500 images per pair in 700 samples (15 m of path); with a limit the row reaches 21 m, past most of order 3
    return 700 if order is None else 1000


def run_parity(r, room, order, kind, air):
    """The 3 x 5 point set with a different pattern on every source, at every kind of receiver and wall."""
    L, ir_len = sc.ROOMS[room], parity_ir_len(order)
    what = f"{room} order={order} {kind} air={air}"
    if kind.startswith("B"):
        n_bands = int(kind[1:])
        m = {"0": 0.0, "m": AIR, "rising": rising_air(n_bands)}[air]
        rows, _ = check_bands_src(r, L, bc.BETA_8[:, :n_bands], bc.centres_of(n_bands, FS), 16, sc.SOURCES_5, SPATS_5, sc.CAPSULES_3, m, ir_len,
                                  FS, max_order=order, what=what)
        assert np.all(np.abs(rows).max(axis=2) > 0), "a row is silent"
        return
    positions, rpats = _receivers(kind)
    y, y64, A, used = check_src(r, L, sc.UNEQUAL_BETAS, sc.SOURCES_5, SPATS_5, positions, rpats, {"0": 0.0, "m": AIR}[air], ir_len, FS,
                                max_order=order, what=what)
    if order == 0:
        assert np.all(used == 1)
    elif order is None:
        assert 100 < used.max() < 8000, used.max()
    assert np.all(np.abs(y).max(axis=2) > 0), "a row is silent"


EDGE_LEN = (1, 81, 256, 257, 1000)


def run_edge_length(r, ir_len):
    """shoebox_cases.run_edge_length's room and points with patterned sources and air: FOA receivers, omni capsules and three bands
    at row lengths around the tap count and the tile."""
    room, betas = (2.4, 2.0, 1.7), (0.8, 0.7, 0.9, 0.6, 0.5, 0.95)
    src = np.array([[0.5, 0.6, 0.7], [2.0, 1.5, 1.1]])
    pos = np.array([[1.9, 1.2, 0.9], [0.52, 0.63, 0.74]])     # the second position is 5 cm from the first source
    spats = SPATS_5[3:]
    y, y64, A, used = check_src(r, room, betas, src, spats, pos, np.stack([shoebox.foa_patterns(), dc.mixed4()]), AIR, ir_len, FS,
                                what=f"edge ir_len={ir_len} foa")
    assert np.abs(y).max() > 0
    if ir_len >= 256:
        assert np.all(A[:, :, min(255, ir_len - 1)] > 0) and np.all(A[:, :, ir_len - 1] > 0)
    y, *_ = check_src(r, room, betas, src, spats, pos, None, AIR, ir_len, FS, what=f"edge ir_len={ir_len} omni")
    assert np.abs(y).max() > 0
    rows, _ = check_bands_src(r, room, bc.BETA_8[:, 3:6], bc.centres_of(3, FS), 16, src, spats, pos, rising_air(3), ir_len, FS,
                              what=f"edge ir_len={ir_len} B=3")
    assert np.abs(rows).max() > 0


def run_close_capsule(r):
    """A capsule 1 cm from its source, on the source's +x side: the direct ray leaves along +x (e = -u, u = (-1, 0, 0)), so a
    cardioid source facing +x gives the omni peak and one facing -x gives nothing but reflections."""
    room, ir_len = (3.0, 2.5, 2.2), 300
    s = np.array([1.0, 1.2, 1.1])
    m = s + np.array([0.01, 0.0, 0.0])
    a = 1.0 / (4 * np.pi * 0.01)
    for facing, sign in (("+x", 1.0), ("-x", -1.0)):
        spat = shoebox.cardioid((sign, 0.0, 0.0))[None]
        y, *_ = check_src(r, room, np.full(6, 0.7), s, spat, m, shoebox.foa_patterns()[None], AIR, ir_len, FS, max_order=2,
                          what=f"capsule at 1 cm, source facing {facing}")
        if sign > 0:
            assert y[0, 0, 0] > 0.5 * a and y[3, 0, 0] < -0.5 * a          # W, and X = -W: the image lies towards -x
        else:
            assert np.abs(y[:, 0, 0]).max() < 1e-3 * a
        rows, _ = check_bands_src(r, room, bc.BETA_8[:, 3:6], bc.centres_of(3, FS), 64, s, spat, m, rising_air(3), ir_len, FS, max_order=2,
                                  what=f"capsule at 1 cm, bands, source facing {facing}")
        assert (rows[0, 0, 0] > 0.5 * a) == (sign > 0)


# ----------------------------------------------------------------------------- 2. ties that do not use the restatement
def run_omni_ties(r):
    """Omni sources (a null table, and rows of (1, 0, 0, 0)) with air = 0 through the new entries: the bits of all six old ones."""
    room, ir_len, order = sc.ROOMS["oblong"], 520, 3
    src, cap = sc.SOURCES_5, sc.CAPSULES_3
    M, F = 300, 100
    n_knots = shoebox.n_knots_of(ir_len)
    foa = np.stack([shoebox.foa_patterns(), dc.mixed4(), shoebox.foa_patterns("zyxw")])
    for spats in (None, OMNI_5):
        name = "null" if spats is None else "omni rows"
        # al_ism_shoebox and al_ism_shoebox_tail (one table for every row)
        want = sc.run_abi(r, room, sc.UNEQUAL_BETAS, src, cap, ir_len, FS, max_order=order)
        assert np.array_equal(bits(run_src(r, room, sc.UNEQUAL_BETAS, src, spats, cap, None, 0.0, ir_len, FS, max_order=order)), bits(want)), name
        want, table = tc.run_tail_abi(r, src, cap, ir_len, M, F, max_order=order, sid0=7, cid0=3)
        tail = dict(M=M, F=F, seed=tc.SEED, sid0=7, cid0=3, ln_env=np.broadcast_to(table, (3, 5, n_knots)))
        got = run_src(r, tc.ROOM, tc.BETAS, src, spats, cap, None, 0.0, ir_len, tc.FS, max_order=order, tail=tail)
        assert np.array_equal(bits(got), bits(want)), (name, "al_ism_shoebox_tail")
        # al_ism_shoebox_dir and al_ism_shoebox_dir_tail (a table per row)
        want = dc.run_abi(r, room, sc.UNEQUAL_BETAS, src, cap, foa, ir_len, FS, max_order=order)
        assert np.array_equal(bits(run_src(r, room, sc.UNEQUAL_BETAS, src, spats, cap, foa, 0.0, ir_len, FS, max_order=order)), bits(want)), name
        want, table = dc.run_tail_abi(r, src, cap, foa, ir_len, M, F, max_order=order, sid0=7, cid0=3)
        tail = dict(M=M, F=F, seed=tc.SEED, sid0=7, cid0=3, ln_env=np.broadcast_to(table[:, None, :], (12, 5, n_knots)))
        got = run_src(r, tc.ROOM, tc.BETAS, src, spats, cap, foa, 0.0, ir_len, tc.FS, max_order=order, tail=tail)
        assert np.array_equal(bits(got), bits(want)), (name, "al_ism_shoebox_dir_tail")
        # al_ism_shoebox_bands and al_ism_shoebox_bands_tail (a table per band)
        beta, centres, half = bc.TAIL_BETA[:, :5], bc.centres_of(5, FS), 64
        want = bc.run_bands_abi(r, room, beta, centres, half, src[:3], cap[:2], ir_len, FS, max_order=order)
        got = run_bands_src(r, room, beta, centres, half, src[:3], None if spats is None else spats[:3], cap[:2], 0.0, ir_len, FS, max_order=order)
        assert np.array_equal(bits(got), bits(want)), (name, "al_ism_shoebox_bands")
        want, table = bc.run_bands_tail_abi(r, room, beta, centres, half, src[:3], cap[:2], ir_len, FS, M, F, max_order=order, sid0=7, cid0=3)
        tail = dict(M=M, F=F, seed=bc.SEED, sid0=7, cid0=3, ln_env=np.broadcast_to(table, (3, 5, n_knots)))
        got = run_bands_src(r, room, beta, centres, half, src[:3], None if spats is None else spats[:3], cap[:2], 0.0, ir_len, FS,
                            max_order=order, tail=tail, pairs_per_pass=4)
        assert np.array_equal(bits(got), bits(want)), (name, "al_ism_shoebox_bands_tail")


def run_order_zero(r):
    """Order 0: the new row is the old row times the closed form gs(direct) exp(-m d), e = -u.  One image, so the two bounds are
    2^-24 of the rows and 2^-30 of A = a W with W the pattern norms."""
    room, ir_len = sc.ROOMS["oblong"], 400
    src, cap = sc.SOURCES_5, sc.CAPSULES_3
    rpats = np.stack([shoebox.cardioid(v)[None] for v in (dc.OBLIQUE, (-0.3, 0.2, 0.9), (0.7, 0.7, -0.1))])
    R = src[None, :, :] - cap[:, None, :]
    d = np.sqrt((R * R).sum(axis=2))
    u = R / d[:, :, None]
    gs = SPATS_5[None, :, 0] + (-u * SPATS_5[None, :, 1:]).sum(axis=2)
    ws = _norm(SPATS_5)[None, :]
    for rp, old in ((None, sc.run_abi(r, room, sc.UNEQUAL_BETAS, src, cap, ir_len, FS, max_order=0)),
                    (rpats, dc.run_abi(r, room, sc.UNEQUAL_BETAS, src, cap, rpats, ir_len, FS, max_order=0))):
        wr = 1.0 if rp is None else _norm(rp[:, 0])[:, None]
        for air in (0.0, AIR):
            new = run_src(r, room, sc.UNEQUAL_BETAS, src, SPATS_5, cap, rp, air, ir_len, FS, max_order=0).astype(np.float64)
            f = gs * np.exp(-air * d)
            want = old.astype(np.float64) * f[:, :, None]
            A = (1.0 / (4.0 * np.pi * d) * wr)[:, :, None] * (old != 0.0)         # the one image, where it has a tap
            bound = 2.0 ** -24 * (np.abs(new) + np.abs(want)) + 2.0 ** -30 * A * (ws * np.exp(-air * d) + np.abs(f))[:, :, None]
            assert_within(new, want, bound, f"order 0 against the old row, receivers {'omni' if rp is None else 'cardioid'}, air={air}")
            assert np.abs(new).max() > 0 and np.abs(gs).min() > 1e-3


def run_reciprocity(r):
    """A patterned source at A heard by an omni capsule at B has the (d, amplitude) of an omni source at B heard at A through a K = 1
    receiver of that pattern: the ray that leaves A along e arrives, run backwards, at A from e.  The second is the OLD entry
    al_ism_shoebox_dir, so the sign convention is pinned without the restatement; the bound is the sum of both rows' bounds, its A
    from shoebox_cases' omni oracle times the pattern norm."""
    room, ir_len = sc.ROOMS["oblong"], 700
    for ia, ib, name in ((0, 0, "cardioid oblique"), (3, 2, "dipole z"), (1, 1, "alpha 0.25 oblique")):
        A_pt, B_pt, pat = sc.SOURCES_5[ia], sc.CAPSULES_3[ib], np.asarray(LAW[name])
        for air in (0.0,):
            new = run_src(r, room, sc.UNEQUAL_BETAS, A_pt, pat[None], B_pt, None, air, ir_len, FS)[0, 0].astype(np.float64)
            old = dc.run_abi(r, room, sc.UNEQUAL_BETAS, B_pt, A_pt, pat[None, None], ir_len, FS)[0, 0].astype(np.float64)
            _, A_ab, _ = sc.oracle(room, sc.UNEQUAL_BETAS, A_pt, B_pt, ir_len, FS)
            _, A_ba, _ = sc.oracle(room, sc.UNEQUAL_BETAS, B_pt, A_pt, ir_len, FS)
            bound = 2.0 ** -24 * (np.abs(new) + np.abs(old)) + 2.0 ** -30 * _norm(pat) * (A_ab[0, 0] + A_ba[0, 0])
            assert_within(new, old, bound, f"reciprocity {name}")
            assert np.abs(new).max() > 0
    # a wrong sign would not pass: the mirrored pattern differs from the row by far more than the bound
    flipped = run_src(r, room, sc.UNEQUAL_BETAS, A_pt, (pat * (1, -1, -1, -1))[None], B_pt, None, 0.0, ir_len, FS)[0, 0]
    assert np.abs(flipped - old).max() > 1e4 * bound.max()


def run_equal_bands(r):
    """Equal band columns with equal m_b: sum_b phi_b = delta, so the row is the broadband new entry's within both bounds (the
    restatement supplies the bounds' A alone)."""
    room, ir_len, half, order = sc.ROOMS["oblong"], 520, 64, 3
    src, cap, spats = sc.SOURCES_5[:2], sc.CAPSULES_3[:2], SPATS_5[3:]
    beta = np.repeat(np.asarray(sc.UNEQUAL_BETAS)[:, None], 3, axis=1)
    rows = run_bands_src(r, room, beta, bc.centres_of(3, FS), half, src, spats, cap, AIR, ir_len, FS, max_order=order)[:, :, :ir_len]
    wide = run_src(r, room, sc.UNEQUAL_BETAS, src, spats, cap, None, AIR, ir_len, FS, max_order=order)[:, :, :ir_len]
    _, bound = restate_bands(room, beta, np.full(3, AIR), bc.centres_of(3, FS), half, src, spats, cap, ir_len, FS, max_order=order)
    _, A, _ = oracle(room, sc.UNEQUAL_BETAS, AIR, src, spats, cap, None, ir_len, FS, max_order=order)
    assert_within(rows, wide.astype(np.float64), bound + 2.0 ** -24 * np.abs(wide) + 2.0 ** -30 * A, "equal bands against the broadband entry")
    assert np.abs(wide).max() > 0


# ----------------------------------------------------------------------------- 3. the tail
def constant_tables(shape):
    """A distinct constant knot table per leading index pair: a wrong stride reads a level that is off by at least 0.25 Np."""
    a, b, n_knots = shape
    return np.broadcast_to((-3.0 - 0.25 * (np.arange(a)[:, None] * b + np.arange(b)[None, :]))[:, :, None], shape).copy()


#              M    F    ir_len kind     order pitch sid0        cid0
TAIL_PARITY = [(M, F, 1000, kind, None, None, 0, 0) for M in (0, 300, 1000) for F in (1, 100) for kind in ("omni", "foa", "B3")] + [
    (300, 100, 900, "K1", 1, 1200, 7, 0xFFFFFFF0), (100, 50, 256 + 4096 + 5, "omni", 1, None, 0xFFFFFFF0, 9), (300, 100, 1000, "B5", 3, None, 7, 3)]


def _tail_points(kind):
    src, cap, spats = sc.SOURCES_5[:3], sc.CAPSULES_3[:2], SPATS_5[2:5]
    if kind in ("omni", "B3", "B5"):
        return src, spats, cap, None
    if kind == "K1":
        return src, spats, cap, np.stack([shoebox.cardioid(v)[None] for v in (dc.OBLIQUE, (-0.3, 0.2, 0.9))])
    return src, spats, cap[:1], dc.mixed4()[None]


def run_tail_parity(r, M, F, ir_len, kind, order, pitch, sid0, cid0):
    src, spats, cap, rpats = _tail_points(kind)
    n_knots = shoebox.n_knots_of(ir_len)
    what = f"tail M={M} F={F} ir_len={ir_len} {kind} order={order}"
    if kind.startswith("B"):
        n_bands, half = int(kind[1:]), 64
        beta, centres, air = bc.TAIL_BETA[:, :n_bands], bc.centres_of(n_bands, FS), rising_air(n_bands)
        ln_env = constant_tables((len(src), n_bands, n_knots))
        tail = dict(M=M, F=F, seed=bc.SEED, sid0=sid0, cid0=cid0, ln_env=ln_env)
        rows = run_bands_src(r, tc.ROOM, beta, centres, half, src, spats, cap, air, ir_len, FS, max_order=order, pitch=pitch, tail=tail)
        assert np.all(bits(rows[:, :, ir_len:]) == 0), "pad samples must be +0"
        h64, bound = restate_bands_tail(tc.ROOM, beta, air, centres, half, src, spats, cap, ir_len, FS, M, F, ln_env, bc.SEED, sid0, cid0,
                                        max_order=order)
        assert_within(rows[:, :, :ir_len], h64, bound, what)
        if M >= ir_len:
            plain = run_bands_src(r, tc.ROOM, beta, centres, half, src, spats, cap, air, ir_len, FS, max_order=order, pitch=pitch)
            assert np.array_equal(bits(rows), bits(plain)), "M >= ir_len differs from mix < 0"
        return
    K = 1 if rpats is None else rpats.shape[1]
    ln_env = constant_tables((len(cap) * K, len(src), n_knots))
    tail = dict(M=M, F=F, seed=tc.SEED, sid0=sid0, cid0=cid0, ln_env=ln_env)
    rows = run_src(r, tc.ROOM, tc.BETAS, src, spats, cap, rpats, AIR, ir_len, FS, max_order=order, pitch=pitch, tail=tail)
    y64, A, _ = oracle(tc.ROOM, tc.BETAS, AIR, src, spats, cap, rpats, min(ir_len, tc.Y_LEN if M + F <= tc.Y_LEN else ir_len), FS, max_order=order)
    assert_tail_rows(rows, y64, A, ln_env, ir_len, M, F, tc.SEED, sid0, cid0, what)
    if ir_len > M + F:
        assert np.all(rows[:, :, M + F: ir_len] != 0.0), "a tail sample is zero"
    if M >= ir_len:
        plain = run_src(r, tc.ROOM, tc.BETAS, src, spats, cap, rpats, AIR, ir_len, FS, max_order=order, pitch=pitch)
        assert np.array_equal(bits(rows), bits(plain)), "M >= ir_len differs from mix < 0"


def run_tail_identity(r):
    """A row alone, among many, at another pitch, with shifted ids and run twice is bit-identical; the band entry with one pair per
    pass against an ample workspace."""
    src, spats, cap = sc.SOURCES_5, SPATS_5, sc.CAPSULES_3
    ir_len, M, F, sid0, cid0 = 700, 100, 50, 7, 3
    n_knots = shoebox.n_knots_of(ir_len)
    foa = np.stack([shoebox.foa_patterns(), dc.mixed4(), shoebox.foa_patterns("zyxw")])
    for rpats in (None, foa):
        K = 1 if rpats is None else 4
        ln_env = constant_tables((3 * K, 5, n_knots))

        def run(ns=slice(0, 5), ps=slice(0, 3), pitch=None, **ids):
            rows = slice(ps.start * K, ps.stop * K)
            tail = dict(dict(M=M, F=F, seed=tc.SEED, sid0=sid0, cid0=cid0, ln_env=ln_env[rows, ns]), **ids)
            return run_src(r, tc.ROOM, tc.BETAS, src[ns], spats[ns], cap[ps], None if rpats is None else rpats[ps], AIR, ir_len, FS, max_order=2,
                           pitch=pitch, tail=tail)

        one = run()
        assert np.array_equal(bits(one), bits(run())), "two runs differ"
        wide = run(pitch=1024 + 256 + 4)
        assert np.array_equal(bits(wide[:, :, :ir_len]), bits(one)) and np.all(bits(wide[:, :, ir_len:]) == 0)
        for p, n in ((0, 0), (1, 3), (2, 4)):
            alone = run(slice(n, n + 1), slice(p, p + 1), sid0=sid0 + n, cid0=cid0 + K * p)
            assert np.array_equal(bits(alone[:, 0]), bits(one[K * p: K * p + K, n])), (K, p, n)
    beta, centres, half = bc.TAIL_BETA[:, :5], bc.centres_of(5, FS), 64
    ln_env = constant_tables((5, 5, n_knots))

    def run_b(ns=slice(0, 5), cs=slice(0, 3), **kw):
        ids = {k: kw.pop(k) for k in ("sid0", "cid0") if k in kw}
        tail = dict(dict(M=M, F=F, seed=bc.SEED, sid0=sid0, cid0=cid0, ln_env=ln_env[ns]), **ids)
        return run_bands_src(r, tc.ROOM, beta, centres, half, src[ns], spats[ns], cap[cs], rising_air(5), ir_len, FS, max_order=2, tail=tail, **kw)

    one = run_b()
    assert np.array_equal(bits(one), bits(run_b())), "two runs differ"
    for per_pass in (1, 4):
        assert np.array_equal(bits(run_b(pairs_per_pass=per_pass)), bits(one)), ("the bits depend on the workspace size", per_pass)
    wide = run_b(pitch=1024 + 256 + 4, pairs_per_pass=2)
    assert np.array_equal(bits(wide[:, :, :ir_len]), bits(one)) and np.all(bits(wide[:, :, ir_len:]) == 0)
    for ci, ni in ((0, 0), (2, 4)):
        alone = run_b(slice(ni, ni + 1), slice(ci, ci + 1), sid0=sid0 + ni, cid0=cid0 + ci)
        assert np.array_equal(bits(alone[0, 0]), bits(one[ci, ni])), (ci, ni)
    plain = run_bands_src(r, tc.ROOM, beta, centres, half, src, spats, cap, rising_air(5), 520, FS, max_order=2)
    assert np.array_equal(bits(run_bands_src(r, tc.ROOM, beta, centres, half, src, spats, cap, rising_air(5), 520, FS, max_order=2,
                                             pairs_per_pass=1)), bits(plain)), "one pair per pass, no tail"


# ----------------------------------------------------------------------------- 4. the envelope
def run_envelope_tables():
    ir_len, fs, M = 3000, 16000.0, 700
    u64 = lambda a: np.asarray(a).view(np.uint64)                                                          # noqa: E731
    for room, betas in ((tc.ROOM, tc.BETAS), ((6.0, 5.0, 3.0), (0.877,) * 6)):
        for rt60 in (None, 0.3):
            for pattern in (None, LAW["cardioid oblique"]):
                today = shoebox.tail_envelope(room, betas, ir_len, fs, M, rt60=rt60, pattern=pattern)
                env = lambda sp, m: shoebox.tail_envelope(room, betas, ir_len, fs, M, rt60=rt60, pattern=pattern, source_pattern=sp, air=m)   # noqa: E731
                for sp in (None, shoebox.omni()):
                    assert np.array_equal(u64(env(sp, 0.0)), u64(today)), "None / omni / 0 change today's table"
                knots = 256.0 * np.arange(shoebox.n_knots_of(ir_len))
                for sp in (None, LAW["dipole z"], LAW["alpha 0.25 oblique"]):
                    dry, wet = env(sp, 0.0), env(sp, AIR)
                    if rt60 is None:      # ln_env[k] -= m c 256 k / fs
                        assert np.abs(wet - (dry - AIR * sc.C_SOUND * knots / fs)).max() <= 1e-12
                    else:                 # matched at the mixing sample with the air in, the requested line kept
                        assert np.abs(wet - (dry - AIR * sc.C_SOUND * M / fs)).max() <= 1e-12
                        assert np.allclose(np.diff(wet), -(3.0 * np.log(10.0) / rt60) * 256.0 / fs, rtol=0, atol=1e-12)
            # the weight is the product of the two quadratic forms: along an axis it is the square of one form
            law = lambda p, sp: np.exp(shoebox.tail_energy_law(room, betas, fs, pattern=p, source_pattern=sp)(M / fs))     # noqa: E731
            axes = shoebox.foa_patterns("wxyz")
            assert abs(sum(law(axes[i], LAW["cardioid oblique"]) for i in (1, 2, 3)) - law(None, LAW["cardioid oblique"])) <= 1e-12 * law(None, None)
            assert abs(law(LAW["dipole x"], LAW["dipole z"]) - law(LAW["dipole z"], LAW["dipole x"])) <= 1e-15 * law(None, None)
            assert law(None, 2.0 * shoebox.omni()) == pytest.approx(4.0 * law(None, None), rel=1e-13)
    for bad in (dict(source_pattern=(0.0,) * 4), dict(source_pattern=(1.0, 0.0, 0.0)), dict(source_pattern=(np.nan, 0.0, 0.0, 1.0)), dict(air=-1e-3),
                dict(air=np.inf), dict(air=np.nan), dict(air="m")):
        with pytest.raises(ValueError):
            shoebox.tail_envelope(tc.ROOM, tc.BETAS, ir_len, fs, M, **bad)


LAW_RECEIVERS = {"omni": LAW["omni"], "cardioid oblique": LAW["cardioid oblique"], "dipole z": LAW["dipole z"]}


def run_envelope_law_against_images():
    """shoebox_directional_cases.run_envelope_law_against_images with its eight patterns as SOURCE patterns against three receivers
    and two air coefficients: a sanity band on the MODEL (not a tolerance on the kernel), the same two rooms, four pairs, 65-sample
    high-pass and four windows; all 384 ratios within the existing factor of 2.  Returns the ratios."""
    snames, spats = list(LAW), np.array(list(LAW.values()))
    rnames, rpats = list(LAW_RECEIVERS), np.array(list(LAW_RECEIVERS.values()))
    t = np.arange(tc.LAW_LEN)
    smooth = np.ones(65) / 65.0
    ratios = {}
    for room_name, (room, betas) in tc.LAW_ROOMS.items():
        pts = tc.LAW_UNIT_POINTS * np.asarray(room)[None, :]
        energy = {m: np.zeros((len(spats), len(rpats), tc.LAW_LEN)) for m in (0.0, AIR)}
        for i in range(4):
            R, d, tau, sign, k = images(room, pts[2 * i], pts[2 * i + 1], tc.LAW_LEN, tc.LAW_FS, sc.C_SOUND, None)
            u = R / d[:, None]
            a = np.prod(np.asarray(betas)[None, :] ** k, axis=1) / (4.0 * np.pi * d)
            tt = np.ceil(tau - sc.HALF)[:, None] + np.arange(sc.TAPS + 1)[None, :]
            x = tt - tau[:, None]
            ok = (np.abs(x) < sc.HALF) & (tt >= 0) & (tt < tc.LAW_LEN)
            shape = 0.5 * (1.0 + np.cos(2.0 * np.pi * x / sc.TAPS)) * np.sinc(x)
            taps = sparse.csr_matrix((shape[ok], (tt[ok].astype(np.int64), np.nonzero(ok)[0])), shape=(tc.LAW_LEN, len(d)))   # (samples, images)
            gs = spats[:, :1] + spats[:, 1:] @ (-sign * u).T                       # (S, images)
            gr = rpats[:, :1] + rpats[:, 1:] @ u.T                                 # (R, images)
            for m in energy:
                amp = (a * np.exp(-m * d))[None, None, :] * gs[:, None, :] * gr[None, :, :]
                y = (taps @ amp.reshape(-1, len(d)).T).T.reshape(len(spats), len(rpats), tc.LAW_LEN)
                if i == 0 and m == AIR:     # the sparse sum is the restatement's
                    y_ref = pair_rows(room, betas, [m], pts[0], pts[1], spats[6], rpats[1:2], 0, 300, tc.LAW_FS)[0][0, 0]
                    assert np.abs(y[6, 1, :300] - y_ref).max() <= 1e-12 * np.abs(y_ref).max()
                for si in range(len(spats)):
                    for ri in range(len(rpats)):
                        hp = y[si, ri] - np.convolve(y[si, ri], smooth, mode="same")
                        energy[m][si, ri] += hp * hp / 4.0
        for m in energy:
            for si, sname in enumerate(snames):
                for ri, rname in enumerate(rnames):
                    law = shoebox.tail_energy_law(room, betas, tc.LAW_FS, pattern=rpats[ri], source_pattern=spats[si], air=m)
                    model = np.exp([law(ti / tc.LAW_FS) for ti in t[::8]])           # the law is smooth: every 8th sample, 1 ms
                    got = [float(energy[m][si, ri, int(a_ * 8): int(b_ * 8)].sum() / (8.0 * model[int(a_): int(b_)].sum()))
                           for a_, b_ in tc.LAW_WINDOWS_MS]
                    ratios[room_name, sname, rname, m] = got
    flat = np.array(list(ratios.values()))
    assert flat.size == 384
    lo_key, hi_key = min(ratios, key=lambda q: min(ratios[q])), max(ratios, key=lambda q: max(ratios[q]))
    print(f"source envelope law: 384 window ratios image energy / law in {flat.min():.3f} .. {flat.max():.3f} "
          f"(lowest {lo_key}: {min(ratios[lo_key]):.3f}, highest {hi_key}: {max(ratios[hi_key]):.3f})")
    for m in (0.0, AIR):
        part = np.array([v for q, v in ratios.items() if q[3] == m])
        print(f"source envelope law, air = {m}: {part.min():.3f} .. {part.max():.3f}")
    for key, got in ratios.items():
        for v in got:
            assert 0.5 <= v <= 2.0, (key, got)
    return ratios


AIR_DB_KM_20C_50 = (0.43978998, 1.30974977, 2.72813413, 4.66473187, 9.88701559, 29.66552843, 105.29092572)
AIR_TABLE_10C_70 = (0.411, 1.04, 1.93, 3.66, 9.66, 32.8, 117.0)       # ISO 9613-1, table 1, dB/km at exact mid-band frequencies
AIR_FREQS = (125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0, 8000.0)


def run_air_absorption():
    to_db_km = 20.0 / np.log(10.0) * 1000.0
    got = shoebox.air_absorption(AIR_FREQS) * to_db_km
    assert got.shape == (7,) and np.all(np.abs(got - AIR_DB_KM_20C_50) <= 1e-7 * np.asarray(AIR_DB_KM_20C_50)), got
    assert np.array_equal(got, shoebox.air_absorption(AIR_FREQS, 20.0, 50.0, 101325.0) * to_db_km)
    cold = shoebox.air_absorption(AIR_FREQS, temperature_c=10.0, humidity=70.0) * to_db_km
    print("air_absorption at 10 C and 70 %, dB/km:", ", ".join(f"{v:.4g}" for v in cold))
    assert np.all(np.abs(cold - AIR_TABLE_10C_70) <= 0.02 * np.asarray(AIR_TABLE_10C_70)), cold
    assert abs(float(shoebox.air_absorption(4000.0)) - AIR) < 2e-5 and shoebox.air_absorption(0.0) == 0.0
    assert np.all(np.diff(shoebox.air_absorption(AIR_FREQS)) > 0)
    assert "above its centre" in shoebox.air_absorption.__doc__
    for bad in (dict(freqs=-1.0), dict(freqs=np.nan), dict(freqs="a"), dict(freqs=1000.0, temperature_c=-300.0), dict(freqs=1000.0, humidity=101.0),
                dict(freqs=1000.0, humidity=-1.0), dict(freqs=1000.0, pressure_pa=0.0), dict(freqs=1000.0, temperature_c=np.inf)):
        with pytest.raises(ValueError):
            shoebox.air_absorption(**bad)


# ----------------------------------------------------------------------------- 5. refusals and state
def run_abi_refusals(r):
    mem, lib = r.mem, r.lib
    src, pos = mem.upload(np.array([1.0, 1.0, 1.0])), mem.upload(np.array([2.0, 1.5, 1.2]))
    spat, pat = mem.upload(np.array(LAW["cardioid oblique"])), mem.upload(shoebox.foa_patterns().reshape(-1))
    out = mem.upload(np.full(4 * 32 + 32, sc.SENTINEL, dtype=np.float32))
    env = mem.upload(np.full(8, -3.0))
    good = dict(sources=mem.ptr(src), n=1, spat=mem.ptr(spat), receivers=mem.ptr(pos), n_pos=1, patterns=mem.ptr(pat), K=4, L=(3.0, 2.5, 2.0),
                beta=(0.5,) * 6, air=AIR, c=343.0, fs=16000.0, order=-1, ir_len=30, pitch=32, mix=10, fade=5, seed=1, sid0=0, cid0=0,
                env=mem.ptr(env), n_knots=2, out=mem.ptr(out))

    def call(**change):
        a = dict(good, **change)
        L = None if a["L"] is None else (ct.c_double * 3)(*a["L"])
        beta = None if a["beta"] is None else (ct.c_double * 6)(*a["beta"])
        return lib.call("al_ism_shoebox_src", a["sources"], a["n"], a["spat"], a["receivers"], a["n_pos"], a["patterns"], a["K"], L, beta,
                        a["air"], a["c"], a["fs"], a["order"], a["ir_len"], a["pitch"], a["mix"], a["fade"], a["seed"], a["sid0"], a["cid0"],
                        a["env"], a["n_knots"], a["out"], mem.stream())

    old = [dict(L=(0.0, 2.5, 2.0)), dict(L=(3.0, 2.5, float("inf"))), dict(c=0.0), dict(c=float("nan")), dict(fs=-1.0),
           dict(beta=(0.5, 0.5, 1.01, 0.5, 0.5, 0.5)), dict(beta=(-0.01,) + (0.5,) * 5), dict(n=0), dict(n_pos=0), dict(ir_len=0),
           dict(pitch=28), dict(pitch=34, ir_len=33), dict(order=-2), dict(sources=None), dict(receivers=None), dict(out=None),
           dict(L=None), dict(beta=None)]
    new = [(dict(K=0), "n_channels must be in 1 .. 4"), (dict(K=5), "n_channels must be in 1 .. 4"), (dict(n_pos=(1 << 31) - 1, K=2), "more than 2^31 - 1 rows"),
           (dict(patterns=None), "takes n_channels == 1"), (dict(patterns=None, K=0), "takes n_channels == 1"), (dict(air=-1e-9), "air must be"),
           (dict(air=float("inf")), "air must be"), (dict(air=float("nan")), "air must be"),
           (dict(fade=0), "fade must be >= 1"), (dict(sid0=-1), "must be >= 0"), (dict(cid0=(1 << 32) - 3), "must not exceed 2^32"),
           (dict(n_knots=1), "n_knots must be"), (dict(n_knots=3), "n_knots must be"), (dict(env=None), "null envelope table"),
           (dict(out=mem.ptr(out) + 4), "out must be 16-byte aligned")]
    for mix in (10, -1):       # everything the old entries refuse, with a tail and without
        for change in old:
            nd.raises_badarg(lambda: call(mix=mix, **change), "al_ism_shoebox_src failed", "al_ism_shoebox: ")
    for change, needle in new:
        nd.raises_badarg(lambda: call(**change), "al_ism_shoebox_src failed", needle)
    assert np.all(np.asarray(mem.download(out)) == sc.SENTINEL), "a refused call wrote"
    assert call() == 0 and call(spat=None) == 0 and call(patterns=None, K=1) == 0 and call(air=0.0) == 0
    # mix < 0: no tail, and the tail's arguments are not looked at
    assert call(mix=-1, fade=0, sid0=-5, cid0=-5, env=None, n_knots=0, out=mem.ptr(out) + 4) == 0
    assert call(mix=-7, patterns=None, K=1, spat=None) == 0

    # the band entry
    phi = mem.upload(shoebox.band_filters((500.0, 2000.0), 16000.0, 8).reshape(-1))
    per_pair = bc.per_pair_bytes(r, 2, 8, 30, 10, 5)
    ws = mem.upload(np.full(per_pair // 8, 7.5))
    out_b = mem.upload(np.full(64, sc.SENTINEL, dtype=np.float32))
    env_b = mem.upload(np.full(4, -3.0))
    good_b = dict(sources=mem.ptr(src), n=1, spat=mem.ptr(spat), capsules=mem.ptr(pos), n_cap=1, L=(3.0, 2.5, 2.0), beta=(0.5,) * 12, n_bands=2,
                  phi=mem.ptr(phi), half=8, air=(0.0, AIR), c=343.0, fs=16000.0, order=-1, ir_len=30, pitch=32, mix=10, fade=5, seed=1, sid0=0,
                  cid0=0, env=mem.ptr(env_b), n_knots=2, ws=mem.ptr(ws), ws_bytes=per_pair, out=mem.ptr(out_b))

    def call_b(**change):
        a = dict(good_b, **change)
        air = None if a["air"] is None else (ct.c_double * len(a["air"]))(*a["air"])
        return lib.call("al_ism_shoebox_bands_src", a["sources"], a["n"], a["spat"], a["capsules"], a["n_cap"], (ct.c_double * 3)(*a["L"]),
                        (ct.c_double * len(a["beta"]))(*a["beta"]), a["n_bands"], a["phi"], a["half"], air, a["c"], a["fs"], a["order"],
                        a["ir_len"], a["pitch"], a["mix"], a["fade"], a["seed"], a["sid0"], a["cid0"], a["env"], a["n_knots"], a["ws"],
                        a["ws_bytes"], a["out"], mem.stream())

    bad = [(dict(L=(0.0, 2.5, 2.0)), "al_ism_shoebox: "), (dict(beta=(0.5,) * 11 + (1.5,)), "al_ism_shoebox: "), (dict(pitch=28), "al_ism_shoebox: "),
           (dict(n_bands=9), "n_bands must be in 1 .. 8"), (dict(half=0), "half must be in"), (dict(half=1025), "half must be in 1 .. 1024 with a tail"),
           (dict(phi=None), "null filter table"), (dict(ws=None), "workspace must be"), (dict(ws_bytes=per_pair - 8), "workspace smaller than"),
           (dict(fade=0), "fade must be >= 1"), (dict(sid0=-1), "must be >= 0"), (dict(cid0=1 << 32), "must not exceed 2^32"),
           (dict(n_knots=3), "n_knots must be"), (dict(env=None), "null envelope table"), (dict(out=mem.ptr(out_b) + 4), "out must be 16-byte aligned"),
           (dict(air=None), "null air table"), (dict(air=(0.0, -1e-9)), "air must be"), (dict(air=(float("nan"), 0.0)), "air must be"),
           (dict(air=(float("inf"), 0.0), mix=-1), "air must be"), (dict(mix=-1, ws_bytes=per_pair - 8), "workspace smaller than")]
    for change, needle in bad:
        nd.raises_badarg(lambda: call_b(**change), "al_ism_shoebox_bands_src failed", needle)
    assert np.all(np.asarray(mem.download(out_b)) == sc.SENTINEL), "a refused call wrote"
    assert call_b() == 0 and call_b(spat=None) == 0
    assert call_b(mix=-1, fade=0, sid0=-5, env=None, n_knots=0, out=mem.ptr(out_b) + 4, half=1025 - 1000) == 0


def run_python_errors(r):
    room, s, m = (3.0, 2.5, 2.0), [[1.0, 1.0, 1.0], [0.7, 2.0, 1.5]], [[2.0, 1.5, 1.2], [0.5, 0.6, 0.7]]
    ok = dict(room=room, betas=(0.5,) * 6, sources=s, capsules=m, ir_len=64, sample_rate=16000)
    bands = shoebox.ShoeboxBands(centres=(500.0, 2000.0), half=8)
    ok_b = dict(ok, betas=np.full((6, 2), 0.5), bands=bands)
    nan = np.tile(shoebox.omni(), (2, 1))
    nan[1, 2] = np.nan
    dead = np.tile(shoebox.omni(), (2, 1))
    dead[0] = 0.0
    bad = [dict(source_patterns=np.ones((3, 4))), dict(source_patterns=np.ones((2, 3))), dict(source_patterns=np.ones((2, 1, 4))), dict(source_patterns=nan),
           dict(source_patterns=dead), dict(source_patterns=np.zeros(4)), dict(source_patterns="cardioid"), dict(air=-1e-3), dict(air=np.nan),
           dict(air=np.inf), dict(air=(1e-3, 2e-3)), dict(air="dry")]
    for change in bad:
        with pytest.raises(ValueError):
            shoebox.shoebox_irs_device(r, **dict(ok, **change))
        with pytest.raises(ValueError):
            shoebox.check_arguments(**dict(ok, **change))
    for change in (dict(air=(1e-3, 2e-3, 3e-3)), dict(air=(1e-3, -2e-3)), dict(air=np.ones((2, 1))), dict(source_patterns=np.ones((3, 4)))):
        with pytest.raises(ValueError):
            shoebox.shoebox_irs_device(r, **dict(ok_b, **change))
    with pytest.raises(ValueError, match="not yet"):      # bands with receiver patterns stay refused, with the new keywords too
        shoebox.shoebox_irs_device(r, **dict(ok_b, patterns=np.tile(shoebox.foa_patterns(), (2, 1, 1)), air=1e-3))
    # what is accepted: one pattern for every source, a row per source; one number for every band, a number per band
    one = shoebox.shoebox_irs_device(r, **dict(ok, source_patterns=shoebox.cardioid((1, 0, 0)), air=AIR))
    two = shoebox.shoebox_irs_device(r, **dict(ok, source_patterns=np.tile(shoebox.cardioid((1, 0, 0)), (2, 1)), air=AIR))
    assert one[1:] == ((128, 64), 64) and np.array_equal(bits(r.mem.download(one[0])[:256]), bits(r.mem.download(two[0])[:256]))
    one = shoebox.shoebox_irs_device(r, **dict(ok_b, air=AIR))
    two = shoebox.shoebox_irs_device(r, **dict(ok_b, air=(AIR, AIR)))
    assert np.array_equal(bits(r.mem.download(one[0])[:256]), bits(r.mem.download(two[0])[:256]))
    # neither keyword: the old entries, today's bits; and the new entries with nothing to add agree with them
    old = shoebox.shoebox_irs_device(r, **ok)
    new = shoebox.shoebox_irs_device(r, **dict(ok, source_patterns=shoebox.omni(), air=0.0))
    assert np.array_equal(bits(r.mem.download(old[0])[:256]), bits(r.mem.download(new[0])[:256]))
    st = core.ShoeboxIRState(room, betas=(0.5,) * 6, ir_len=64, sample_rate=16000, renderer=r)
    for call in (lambda: st.add_emitters(s, patterns=np.ones((3, 4))), lambda: st.add_emitters(s, patterns=np.zeros(4)),
                 lambda: st.add_emitters(s, patterns=nan), lambda: core.ShoeboxIRState(room, betas=(0.5,) * 6, air=-1.0),
                 lambda: core.ShoeboxIRState(room, betas=(0.5,) * 6, air=(1e-3, 2e-3)),
                 lambda: core.ShoeboxIRState(room, betas=np.full((6, 2), 0.5), bands=bands, air=(1e-3, 2e-3, 3e-3), sample_rate=16000)):
        with pytest.raises(ValueError):
            call()
    assert len(st.emitters) == 0 and st.emitter_patterns is None


TALKER = np.array([0.8, 0.9, 1.0])


def _state(r, tail=None, ir_len=520, max_order=3, air=AIR):
    st = core.ShoeboxIRState(tc.ROOM, betas=tc.BETAS, ir_len=ir_len, sample_rate=sc.SR, max_order=max_order, renderer=r, tail=tail, air=air)
    st.add_microphone("dir", dc.DIR_MIC, patterns=dc._dir_patterns(), capsule_names=["left", "right"])
    st.add_microphone("omni", dc.DIR_MIC)
    st.add_emitters([TALKER], alias="static", patterns=shoebox.cardioid((1.0, 0.2, 0.0)))
    st.add_emitters(np.linspace([3.2, 0.6, 1.5], [3.4, 2.8, 1.1], 3), alias="moving")                       # no patterns: omni rows
    st.add_emitters([[1.0, 2.5, 0.7], [1.2, 2.5, 0.7]], alias="pair", patterns=SPATS_5[3:])
    return st


def run_state(r):
    st = _state(r)
    spats = np.concatenate([shoebox.cardioid((1.0, 0.2, 0.0))[None], np.tile(shoebox.omni(), (3, 1)), SPATS_5[3:]])
    assert np.array_equal(st.emitter_patterns, spats) and st.num_emitters == 6
    st.simulate()
    sources = st.emitter_positions
    y64, A, _ = oracle(tc.ROOM, tc.BETAS, AIR, sources, spats, dc.DIR_MIC, dc._dir_patterns()[:, None, :], 520, float(sc.SR), max_order=3)
    assert_within(np.asarray(st.irs["dir"]), y64, 2.0 ** -24 * np.abs(y64) + 2.0 ** -30 * A, "state, directional microphone")
    y64, A, _ = oracle(tc.ROOM, tc.BETAS, AIR, sources, spats, dc.DIR_MIC, None, 520, float(sc.SR), max_order=3)
    assert_within(np.asarray(st.irs["omni"]), y64, 2.0 ** -24 * np.abs(y64) + 2.0 ** -30 * A, "state, omni microphone")
    # JSON round trip: the emitters entry keeps its form, the two new keys sit in the shoebox block
    d = json.loads(json.dumps(st.to_dict()))
    assert d["shoebox"]["air"] == AIR and sorted(d["shoebox"]["emitter_patterns"]) == ["pair", "static"]
    assert d["emitters"] == {k: v.tolist() for k, v in st.emitters.items()}
    assert core.ShoeboxIRState.describes(d)
    again = core.ShoeboxIRState.from_dict(d, renderer=r)
    assert json.loads(json.dumps(again.to_dict())) == d and np.array_equal(again.emitter_patterns, spats)
    again.simulate()
    for alias in ("dir", "omni"):
        assert np.array_equal(bits(np.asarray(again.irs[alias])), bits(np.asarray(st.irs[alias]))), alias
    # a dictionary from before: neither key, omni emitters and no air, the old entries' bits
    before = json.loads(json.dumps(d))
    del before["shoebox"]["air"], before["shoebox"]["emitter_patterns"]
    plain = core.ShoeboxIRState.from_dict(before, renderer=r)
    assert plain.air is None and plain.emitter_patterns is None
    assert "air" not in plain.to_dict()["shoebox"] and "emitter_patterns" not in plain.to_dict()["shoebox"]
    assert json.loads(json.dumps(plain.to_dict())) == before
    plain.simulate()
    want = sc.run_abi(r, tc.ROOM, tc.BETAS, sources, dc.DIR_MIC, 520, sc.SR, max_order=3)
    assert np.array_equal(bits(np.asarray(plain.irs["omni"])), bits(want[:, :, :520]))
    # bands: air per band in the dictionary
    banded = core.ShoeboxIRState(tc.ROOM, betas=bc.TAIL_BETA[:, :3], bands=dict(centres=[250.0, 1000.0, 3000.0], half=16), ir_len=300,
                                 sample_rate=sc.SR, max_order=2, renderer=r, air=rising_air(3))
    banded.add_microphone("omni", dc.DIR_MIC)
    banded.add_emitters([TALKER], patterns=LAW["dipole x"])
    d = json.loads(json.dumps(banded.to_dict()))
    assert d["shoebox"]["air"] == rising_air(3).tolist()
    banded.simulate()
    h64, bound = restate_bands(tc.ROOM, bc.TAIL_BETA[:, :3], rising_air(3), (250.0, 1000.0, 3000.0), 16, [TALKER], [LAW["dipole x"]], dc.DIR_MIC,
                               300, float(sc.SR), max_order=2)
    assert_within(np.asarray(banded.irs["omni"]), h64, bound, "state, bands")
    again = core.ShoeboxIRState.from_dict(d, renderer=r)
    again.simulate()
    assert np.array_equal(bits(np.asarray(again.irs["omni"])), bits(np.asarray(banded.irs["omni"])))
    # with a tail: every (row, source) pair under the envelope of its own patterns and the air
    tailed = _state(r, tail=tc.STATE_TAIL, ir_len=900, max_order=None)
    tailed.simulate()
    M, F = shoebox.tail_samples(tailed.tail, tc.ROOM, sc.SR)
    for alias, rp, cid0 in (("dir", dc._dir_patterns()[:, None, :], 0), ("omni", None, 2)):
        y64, A, _ = oracle(tc.ROOM, tc.BETAS, AIR, sources, spats, dc.DIR_MIC, rp, tc.Y_LEN, float(sc.SR))
        rows = [None, None] if rp is None else list(rp[:, 0])
        ln_env = np.stack([np.stack([shoebox.tail_envelope(tc.ROOM, tc.BETAS, 900, float(sc.SR), M, pattern=row, source_pattern=sp, air=AIR)
                                     for sp in spats]) for row in rows])
        assert_tail_rows(np.asarray(tailed.irs[alias]), y64, A, ln_env, 900, M, F, tc.STATE_TAIL["seed"], 0, cid0, f"state tail {alias}")


# ----------------------------------------------------------------------------- 6. Scene.generate(): sign checks on the model
def _window_energy(x, lo, hi):
    return float((np.asarray(x, dtype=np.float64)[..., lo:hi] ** 2).sum())


def run_talker_scene(r):
    """A cardioid source facing the microphone against the same source facing away, a click rendered by Scene.generate(): more
    energy in the first 5 ms after the direct arrival when facing, late-window energy within a factor of 2."""
    mic = np.array([[2.9, 2.0, 1.3]])
    towards = (mic[0] - TALKER) / np.linalg.norm(mic[0] - TALKER)
    click = np.zeros(4000, dtype=np.float32)       # an event lasts as long as its clip: the silence keeps the reverberation
    click[0] = 1.0
    audio = {}
    for name, direction in (("facing", towards), ("away", -towards)):
        st = core.ShoeboxIRState(tc.ROOM, betas=(0.9,) * 6, ir_len=3200, sample_rate=sc.SR, renderer=r)
        st.add_microphone("mic", mic)
        st.add_emitters([TALKER], alias="talker", patterns=shoebox.cardioid(direction))
        scene = core.Scene(0.5, st, sample_rate=sc.SR)
        scene.add_event(core.Event("talker", click, sc.SR, snr=12.0, scene_start=0.05, n_emitters=1))
        audio[name] = np.array(scene.generate(metadata_dcase=False)["mic"])[0].astype(np.float64)
    start = int(0.05 * sc.SR) + int(np.linalg.norm(mic[0] - TALKER) / sc.C_SOUND * sc.SR)
    early = {k: _window_energy(v, start - 41, start + int(0.005 * sc.SR)) for k, v in audio.items()}
    late = {k: _window_energy(v, start + int(0.08 * sc.SR), start + int(0.19 * sc.SR)) for k, v in audio.items()}
    print(f"talker scene: early energy facing / away {early['facing'] / early['away']:.3f}, late energy facing / away "
          f"{late['facing'] / late['away']:.3f}")
    assert early["facing"] > early["away"] > 0.0
    assert 0.5 <= late["facing"] / late["away"] <= 2.0


def run_talker_irs(r):
    """The same check on the IRs themselves (no level law in between): early energy higher facing, late energy within a factor 2."""
    mic = np.array([[2.9, 2.0, 1.3]])
    towards = (mic[0] - TALKER) / np.linalg.norm(mic[0] - TALKER)
    rows = {}
    for name, direction in (("facing", towards), ("away", -towards)):
        buf, _, _ = shoebox.shoebox_irs_device(r, tc.ROOM, (0.9,) * 6, [TALKER], mic, 4000, sc.SR, source_patterns=shoebox.cardioid(direction))
        rows[name] = np.asarray(r.mem.download(buf))[:4000].astype(np.float64)
    t0 = int(np.linalg.norm(mic[0] - TALKER) / sc.C_SOUND * sc.SR)
    early = {k: _window_energy(v, max(t0 - 41, 0), t0 + int(0.005 * sc.SR)) for k, v in rows.items()}
    late = {k: _window_energy(v, t0 + int(0.08 * sc.SR), 4000) for k, v in rows.items()}
    print(f"talker IRs: early energy facing / away {early['facing'] / early['away']:.2f}, late energy facing / away {late['facing'] / late['away']:.3f}")
    assert early["facing"] > early["away"] > 0.0
    assert 0.5 <= late["facing"] / late["away"] <= 2.0


def run_air_scene(r):
    """A hard room with bands and air_absorption, a click rendered by Scene.generate(): above 2 kHz the late energy is lower than without
    air, below 500 Hz the energy is within 10 %."""
    centres = (125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0)
    betas = np.full((6, 6), np.sqrt(1.0 - 0.02))          # concrete: 2 % at every band
    audio = {}
    for name, air in (("dry", None), ("air", shoebox.air_absorption(centres))):
        st = core.ShoeboxIRState((6.0, 5.0, 3.0), betas=betas, bands=dict(centres=list(centres), half=64), ir_len=6000, sample_rate=sc.SR,
                                 max_order=12, renderer=r, air=air)
        st.add_microphone("mic", np.array([[4.1, 3.2, 1.4]]))
        st.add_emitters([[1.2, 1.1, 1.6]], alias="burst")
        scene = core.Scene(0.8, st, sample_rate=sc.SR)
        # a click: the event's one scalar (the level law scales to the peak) then hangs on the direct arrival, which the air leaves
        # alone to 1 % over 3.6 m, and not on where a noise burst happens to pile up.  An event lasts as long as its clip
        burst = np.zeros(11200, dtype=np.float32)
        burst[0] = 1.0
        scene.add_event(core.Event("burst", burst, sc.SR, snr=12.0, scene_start=0.05, n_emitters=1))
        audio[name] = np.array(scene.generate(metadata_dcase=False)["mic"])[0].astype(np.float64)

    def band(x, lo_hz, hi_hz, start=0):
        spec = np.abs(np.fft.rfft(x[start:])) ** 2
        f = np.fft.rfftfreq(len(x) - start, 1.0 / sc.SR)
        return float(spec[(f >= lo_hz) & (f < hi_hz)].sum())

    late = int(0.25 * sc.SR)
    ratio_low = band(audio["air"], 0.0, 500.0) / band(audio["dry"], 0.0, 500.0)
    ratio_high = band(audio["air"], 2000.0, 8000.0, late) / band(audio["dry"], 2000.0, 8000.0, late)
    print(f"air scene: energy with air / without, below 500 Hz {ratio_low:.4f}, late above 2 kHz {ratio_high:.4f}")
    assert ratio_high < 1.0, "the late energy above 2 kHz is not lower with air"
    assert abs(ratio_low - 1.0) <= 0.1, "the energy below 500 Hz moved by more than 10 %"


# ----------------------------------------------------------------------------- 7. schedule independence (GPU only)
def run_shake_rows(r):
    """{name: rows} of the new entries without a tail and with one, each held to its restatement first;
    tests/test_gpu_shoebox_source.py compares the rows of differently scheduled builds bit for bit."""
    src, spats, cap = sc.SOURCES_5[:3], SPATS_5[2:5], sc.CAPSULES_3[:2]
    foa = np.stack([shoebox.foa_patterns(), dc.mixed4()])
    ir_len, M, F = 700, 300, 100
    n_knots = shoebox.n_knots_of(ir_len)
    out = {}
    for name, rp in (("omni", None), ("foa", foa)):
        K = 1 if rp is None else 4
        y64, A, _ = oracle(tc.ROOM, tc.BETAS, AIR, src, spats, cap, rp, ir_len, FS, max_order=3)
        out[name] = run_src(r, tc.ROOM, tc.BETAS, src, spats, cap, rp, AIR, ir_len, FS, max_order=3)
        assert_within(out[name], y64, 2.0 ** -24 * np.abs(y64) + 2.0 ** -30 * A, f"shake rows {name}")
        ln_env = constant_tables((2 * K, 3, n_knots))
        out[name + " tail"] = run_src(r, tc.ROOM, tc.BETAS, src, spats, cap, rp, AIR, ir_len, FS, max_order=3,
                                      tail=dict(M=M, F=F, ln_env=ln_env, sid0=7, cid0=3))
        assert_tail_rows(out[name + " tail"], y64, A, ln_env, ir_len, M, F, tc.SEED, 7, 3, f"shake rows {name} tail")
    beta, centres, half, air = bc.TAIL_BETA[:, :5], bc.centres_of(5, FS), 64, rising_air(5)
    out["bands"] = run_bands_src(r, tc.ROOM, beta, centres, half, src, spats, cap, air, ir_len, FS, max_order=3, pairs_per_pass=4)
    h64, bound = restate_bands(tc.ROOM, beta, air, centres, half, src, spats, cap, ir_len, FS, max_order=3)
    assert_within(out["bands"], h64, bound, "shake rows bands")
    ln_env = constant_tables((3, 5, n_knots))
    out["bands tail"] = run_bands_src(r, tc.ROOM, beta, centres, half, src, spats, cap, air, ir_len, FS, max_order=3, pairs_per_pass=4,
                                      tail=dict(M=M, F=F, ln_env=ln_env, sid0=7, cid0=3))
    h64, bound = restate_bands_tail(tc.ROOM, beta, air, centres, half, src, spats, cap, ir_len, FS, M, F, ln_env, bc.SEED, 7, 3, max_order=3)
    assert_within(out["bands tail"], h64, bound, "shake rows bands tail")
    return out
