"""Scenarios of the shoebox IR generator with frequency-dependent walls (al_ism_shoebox_bands, shoebox.ShoeboxBands,
shoebox.band_filters, shoebox.load_materials / material_betas, core.ShoeboxIRState(bands=..., materials=...)) and the float64 numpy
restatement of its definition (DESIGN.md "Shoebox IRs: frequency-dependent walls"; no reference code computes this).
tests/test_hostemu_shoebox_bands.py runs them on the host-emulated kernels, tests/test_gpu_shoebox_bands.py on the gfx950 build.

THE DEFINITION.  With B bands, beta (6, B), the table phi = shoebox.band_filters(centres, fs, half) of shape (B, 2 half + 1):
    y_b[s] = the image sum of tests/shoebox_cases.py (tap shape, +-40.5 reach, order rule, beta = 0 rule) under beta[:, b], at EVERY
             integer s in [-half, ir_len + half): the taps at negative s are kept
    y(t)   = sum_b sum_{j = -half .. half} phi_b[j] y_b[t - j]          (float64)
    h[t]   = float32(y(t)), t in [0, ir_len); pads +0.

THE BOUND (derived, not tuned), every sample, none excluded.  With A_b[s] the sum of |a_i| over the images of band b with a tap at s:
    |h - h64| <= 2^-24 |h64| + 2^-30 sum_b sum_j |phi_b[j]| A_b[t - j]
The first term is the one rounding to float32.  The second carries shoebox_cases' bound on a band sum (2^-30 A_b[s]: float64 tau and
libm differences, with margin) through the FIR, whose own float64 accumulation of B (2 half + 1) <= 8 * 601 products adds at most
4808 * 2^-53 = 5e-13 of sum |phi| |y_b| <= sum |phi| A_b: three orders below 2^-30 = 9e-10.

THE TAIL WITH BANDS (al_ism_shoebox_bands_tail).  ln_env (B, n_knots), M, F, w_e, w_l and the draws g(s) of tests/shoebox_tail_cases.py
(zero outside [0, ir_len)); y_b and y(t) as above with y_end = min(ir_len, M + F) in place of ir_len; and
    psi_k[j] = sum_b exp(ln_env[b][k]) phi_b[j],  k = t // 256,  p = (t % 256) / 256
    n(t) = (1 - p) sum_j psi_k[j] g(t - j) + p sum_j psi_{k+1}[j] g(t - j)        (p == 0 reads knot k alone)
    h = float32(w_e y(t) + w_l n(t)), no noise term where w_l == 0.
ITS BOUND, every sample.  With tol(s) = noise_draw_cases.RTOL |g64(s)| + ATOL for 0 <= s < ir_len (0 outside), |psi|_t the
interpolated (1 - p) |psi_k| + p |psi_{k+1}| and e_b(t) = (1 - p) exp(ln_env[b][k]) + p exp(ln_env[b][k + 1]):
    |h - h64| <= w_e 2^-30 sum_b sum_j |phi_b[j]| A_b[t - j]                         the image part, as above, under its fade
               + w_l sum_j |psi|_t[j] tol(t - j)                                     the draws' tolerance, carried through the FIR
               + w_l (2 half + 1 + B + 16) 2^-53 sum_b e_b(t) sum_j |phi_b[j]| |g(t - j)|   float64 accumulation, either order of the sums
               + 2^-24 |h64| + 2^-150                                                 the one rounding
The third term is the standard n u bound of a sum of n = 2 half + 1 products plus B band terms, with 16 u for exp, the
interpolation and the fade weights; it is taken against sum_b e_b sum_j |phi_b| |g| >= sum_j |psi| |g| so that it covers both
n(t) as written and the same number with the sums over b and j exchanged (k_ism_band_combine<true>).

THE MATERIAL FIXTURE tests/golden/shoebox_materials.json was derived from the reference's resources/mp3d_material_config.json by
keeping, of each of its 30 materials, the keys "name" and "absorption" as they stand and nothing else (no scattering, transmission,
labels, damping, density or speed), in the file's order.
"""
import ctypes as ct
import functools
import json
import os

import numpy as np
import pytest

from audiblelight_amd import _hip, core, engine, shoebox
from tests import noise_draw_cases as nd
from tests import shoebox_cases as sc
from tests import shoebox_tail_cases as tc

bits = sc.bits
FS = 16000.0
CENTRES_16K = (125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0)
CENTRES_8 = (63.0, 125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0, 8000.0)        # B = 8, at 48 kHz
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shoebox_materials.json")
# six walls x eight bands, all different, one wall at 0 in one band only and one at 1 in another: default_rng(11).uniform(0.3, 0.98)
BETA_8 = np.random.default_rng(11).uniform(0.3, 0.98, (6, 8))
BETA_8[0, 1], BETA_8[3, 2] = 0.0, 1.0


SEED = 0xB4D5F00D12345678
TAIL_BETA = np.random.default_rng(12).uniform(0.55, 0.97, (6, 8))      # every coefficient > 0; bands that decay at different rates


def centres_of(n_bands, fs):
    if n_bands == 8:
        assert fs == 48000.0
        return CENTRES_8
    return {1: (1000.0,), 2: (500.0, 2000.0), 3: (250.0, 1000.0, 3000.0), 5: (125.0, 250.0, 500.0, 1000.0, 2000.0), 6: CENTRES_16K}[n_bands]


# ----------------------------------------------------------------------------- the restatement
def _band_rows(room, beta, s, r, y_end, half, fs, c, max_order):
    """(y_b, A_b) of shape (B, y_end + 2 half): index i holds sample s = i - half.  shoebox_cases.oracle_pair's arithmetic,
    vectorised over the images, without its cut at sample 0, the gains of the B columns of beta (6, B) side by side."""
    lo, hi = -half, y_end + half
    reach = c * (hi + sc.HALF) / fs
    beta = np.asarray(beta, dtype=np.float64)
    ax = [sc._axis(s[i], r[i], room[i], 1.0, 1.0, reach) for i in range(3)]
    Rx, Ry, Rz = np.meshgrid(ax[0][0], ax[1][0], ax[2][0], indexing="ij")
    order = ax[0][1][:, None, None] + ax[1][1][None, :, None] + ax[2][1][None, None, :]
    d = np.sqrt(Rx * Rx + Ry * Ry + Rz * Rz)
    tau = d * fs / c
    keep = tau - sc.HALF < hi
    if max_order is not None:
        keep &= order <= max_order
    n_bands = beta.shape[1]
    y, A = np.zeros((n_bands, hi - lo)), np.zeros((n_bands, hi - lo))
    d, tau = d[keep], tau[keep]
    t = np.ceil(tau - sc.HALF)[:, None] + np.arange(sc.TAPS + 1)[None, :]
    u = t - tau[:, None]
    ok = (np.abs(u) < sc.HALF) & (t >= lo) & (t < hi)
    shape = 0.5 * (1.0 + np.cos(2.0 * np.pi * u / sc.TAPS)) * np.sinc(u)
    for b in range(n_bands):
        gains = [sc._axis(s[i], r[i], room[i], beta[2 * i, b], beta[2 * i + 1, b], reach)[2] for i in range(3)]
        gain = (gains[0][:, None, None] * gains[1][None, :, None] * gains[2][None, None, :])[keep]
        a = gain / (4.0 * np.pi * d)
        live = ok & (gain > 0.0)[:, None]                  # a wall of beta = 0 in its path: no image in this band
        idx = (t[live] - lo).astype(np.int64)
        y[b] = np.bincount(idx, weights=(a[:, None] * shape)[live], minlength=hi - lo)
        A[b] = np.bincount(idx, weights=np.broadcast_to(np.abs(a)[:, None], t.shape)[live], minlength=hi - lo)
    return y, A


@functools.lru_cache(maxsize=None)
def _restate_cached(room, beta, n_bands, centres, half, sources, capsules, ir_len, fs, c, max_order):
    beta = np.array(beta).reshape(6, n_bands)
    phi = shoebox.band_filters(centres, fs, half)
    C, N = len(capsules), len(sources)
    h, bound = np.zeros((C, N, ir_len)), np.zeros((C, N, ir_len))
    for ci in range(C):
        for ni in range(N):
            y, A = _band_rows(room, beta, sources[ni], capsules[ci], ir_len, half, fs, c, max_order)
            for b in range(n_bands):
                # full convolution: entry k holds sum_m phi[m] y[k - m], m = j + half, k - m = t - j + half: k = t + 2 half
                h[ci, ni] += np.convolve(y[b], phi[b])[2 * half: 2 * half + ir_len]
                bound[ci, ni] += np.convolve(A[b], np.abs(phi[b]))[2 * half: 2 * half + ir_len]
    bound = 2.0 ** -24 * np.abs(h) + 2.0 ** -30 * bound
    h.flags.writeable = bound.flags.writeable = False
    return h, bound


def restate(room, beta, centres, half, sources, capsules, ir_len, fs, c=sc.C_SOUND, max_order=None):
    """(h64, bound) of shape (C, N, ir_len): computed once per scenario and shared (read-only)."""
    beta = np.asarray(beta, dtype=np.float64)
    pts = lambda v: tuple(tuple(float(x) for x in row) for row in np.atleast_2d(v))           # noqa: E731
    return _restate_cached(tuple(float(x) for x in room), tuple(beta.reshape(-1)), beta.shape[1], tuple(float(x) for x in centres), int(half),
                           pts(sources), pts(capsules), int(ir_len), float(fs), float(c), max_order)


WORST = {"fraction": 0.0}


def assert_within(rows, h64, bound, what):
    rows = np.asarray(rows, dtype=np.float64)
    assert np.all(np.isfinite(rows)), what
    err = np.abs(rows - h64)
    frac = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)))
    WORST["fraction"] = max(WORST["fraction"], frac)
    print(f"shoebox bands bound [{what}]: max err {err.max():.3e}, max err / bound {frac:.3f} (so far {WORST['fraction']:.3f})")
    assert np.all(err <= bound), (what, "err / bound", frac, "at", np.unravel_index(np.argmax(err - bound), err.shape))


def band_envelopes(room, beta, ir_len, fs, M, c=sc.C_SOUND, rt60=None):
    return np.stack([shoebox.tail_envelope(room, beta[:, b], ir_len, fs, min(M, ir_len), c, rt60) for b in range(beta.shape[1])])


def restate_tail(room, beta, centres, half, sources, capsules, ir_len, fs, M, F, ln_env, seed, sid0, cid0, c=sc.C_SOUND, max_order=None,
                 phi=None):
    """(h64, bound) of shape (C, N, ir_len) of al_ism_shoebox_bands_tail."""
    beta, ln_env = np.asarray(beta, dtype=np.float64), np.asarray(ln_env, dtype=np.float64)
    sources, capsules = np.atleast_2d(sources), np.atleast_2d(capsules)
    n_bands, n_taps = beta.shape[1], 2 * half + 1
    phi = shoebox.band_filters(centres, fs, half) if phi is None else phi
    y_end = min(ir_len, M + F)
    w_e, w_l = tc.weights(ir_len, M, F)
    t = np.arange(ir_len)
    k, p = t // 256, (t % 256) / 256.0
    with np.errstate(over="ignore"):
        e = np.exp(ln_env)                                         # (B, n_knots); exp(-inf) = 0
    psi = np.einsum("bk,bj->kj", e, phi)                           # (n_knots, n_taps)

    def lerp(table):                                               # table (n_knots, ir_len) -> (1 - p) table[k] + p table[k + 1] at t
        return np.where(p == 0.0, table[k, t], (1.0 - p) * table[k, t] + p * table[np.minimum(k + 1, len(table) - 1), t])

    fir = lambda x, taps: np.convolve(x, taps)[half: half + ir_len]       # noqa: E731  sum_j taps[j + half] x[t - j], x zero outside
    h, bound = np.zeros((len(capsules), len(sources), ir_len)), np.zeros((len(capsules), len(sources), ir_len))
    for ci in range(len(capsules)):
        for ni in range(len(sources)):
            y, A = _band_rows(room, beta, sources[ni], capsules[ci], y_end, half, fs, c, max_order)
            img, img_bound = np.zeros(ir_len), np.zeros(ir_len)
            for b in range(n_bands):
                img[:y_end] += np.convolve(y[b], phi[b])[2 * half: 2 * half + y_end]
                img_bound[:y_end] += np.convolve(A[b], np.abs(phi[b]))[2 * half: 2 * half + y_end]
            g = tc.restated_g(seed, sid0 + ni, cid0 + ci, ir_len)
            tol = nd.RTOL * np.abs(g) + nd.ATOL
            noise = lerp(np.stack([fir(g, psi[kk]) for kk in range(len(psi))]))
            draw = lerp(np.stack([fir(tol, np.abs(psi[kk])) for kk in range(len(psi))]))
            spread = np.stack([fir(np.abs(g), np.abs(phi[b])) for b in range(n_bands)])          # (B, ir_len)
            accum = (n_taps + n_bands + 16) * 2.0 ** -53 * lerp(np.einsum("bk,bt->kt", e, spread))
            h[ci, ni] = w_e * img + np.where(w_l > 0.0, w_l * noise, 0.0)
            bound[ci, ni] = (w_e * 2.0 ** -30 * img_bound + np.where(w_l > 0.0, w_l * (draw + accum), 0.0) + 2.0 ** -24 * np.abs(h[ci, ni])
                             + 2.0 ** -150)
    return h, bound


# ----------------------------------------------------------------------------- running the entry point
def per_pair_bytes(r, n_bands, half, ir_len, mix=-1, fade=0):
    return r.lib.call("al_ism_shoebox_bands_workspace_bytes", int(n_bands), int(half), int(ir_len), int(mix), int(fade))


def run_bands_tail_abi(r, room, beta, centres, half, sources, capsules, ir_len, fs, M, F, ln_env=None, seed=SEED, sid0=0, cid0=0,
                       c=sc.C_SOUND, max_order=None, pitch=None, pairs_per_pass=None):
    """al_ism_shoebox_bands_tail as run_bands_abi runs the entry without a tail; ((C, N, pitch) rows, ln_env)."""
    mem, lib = r.mem, r.lib
    sources = np.ascontiguousarray(np.atleast_2d(sources), dtype=np.float64)
    capsules = np.ascontiguousarray(np.atleast_2d(capsules), dtype=np.float64)
    beta = np.ascontiguousarray(beta, dtype=np.float64)
    n, n_cap, n_bands = len(sources), len(capsules), beta.shape[1]
    pitch = shoebox.pitch_of(ir_len) if pitch is None else pitch
    total = n_cap * n * pitch
    phi = shoebox.band_filters(centres, fs, half)
    ln_env = band_envelopes(room, beta, ir_len, fs, M, c) if ln_env is None else np.ascontiguousarray(ln_env, dtype=np.float64)
    per_pair = per_pair_bytes(r, n_bands, half, ir_len, M, F)
    assert per_pair == n_bands * ((min(ir_len, M + F) + 2 * half + 255) // 256 * 256) * 8
    ws_bytes = per_pair * (n * n_cap if pairs_per_pass is None else pairs_per_pass)
    ws = mem.upload(np.full(ws_bytes // 8 + sc.GUARD, 7.5, dtype=np.float64))
    out = mem.upload(np.full(total + 2 * sc.GUARD, sc.SENTINEL, dtype=np.float32))
    src_dev, cap_dev, phi_dev = mem.upload(sources.reshape(-1)), mem.upload(capsules.reshape(-1)), mem.upload(phi.reshape(-1))
    env_dev = mem.upload(ln_env.reshape(-1))
    L = (ct.c_double * 3)(*room)
    lib.call("al_ism_shoebox_bands_tail", mem.ptr(src_dev), n, mem.ptr(cap_dev), n_cap, L, beta.ctypes.data_as(ct.POINTER(ct.c_double)),
             n_bands, mem.ptr(phi_dev), int(half), float(c), float(fs), -1 if max_order is None else int(max_order), int(ir_len), int(pitch),
             int(M), int(F), int(seed), int(sid0), int(cid0), mem.ptr(env_dev), ln_env.shape[1], mem.ptr(ws), ws_bytes,
             mem.ptr(out) + 4 * sc.GUARD, mem.stream())
    host = np.asarray(mem.download(out))
    assert np.all(host[:sc.GUARD] == sc.SENTINEL) and np.all(host[sc.GUARD + total:] == sc.SENTINEL), "guard overwritten"
    assert not np.any(host[sc.GUARD: sc.GUARD + total] == sc.SENTINEL), "a sample was not written"
    assert np.all(np.asarray(mem.download(ws))[ws_bytes // 8:] == 7.5), "the workspace's guard was overwritten"
    return host[sc.GUARD: sc.GUARD + total].reshape(n_cap, n, pitch).copy(), ln_env


def run_bands_abi(r, room, beta, centres, half, sources, capsules, ir_len, fs, c=sc.C_SOUND, max_order=None, pitch=None,
                  pairs_per_pass=None, phi=None):
    """al_ism_shoebox_bands into a buffer with sc.GUARD sentinels on either side and a workspace with a guard behind it; the
    (C, N, pitch) rows, the guards checked.  pairs_per_pass: the workspace holds exactly that many pairs (None: all of them)."""
    mem, lib = r.mem, r.lib
    sources = np.ascontiguousarray(np.atleast_2d(sources), dtype=np.float64)
    capsules = np.ascontiguousarray(np.atleast_2d(capsules), dtype=np.float64)
    beta = np.ascontiguousarray(beta, dtype=np.float64)
    n, n_cap, n_bands = len(sources), len(capsules), beta.shape[1]
    pitch = shoebox.pitch_of(ir_len) if pitch is None else pitch
    total = n_cap * n * pitch
    phi = shoebox.band_filters(centres, fs, half) if phi is None else np.ascontiguousarray(phi, dtype=np.float64)
    assert phi.shape == (n_bands, 2 * half + 1)
    per_pair = per_pair_bytes(r, n_bands, half, ir_len)
    assert per_pair == n_bands * ((ir_len + 2 * half + 255) // 256 * 256) * 8
    ws_bytes = per_pair * (n * n_cap if pairs_per_pass is None else pairs_per_pass)
    ws = mem.upload(np.full(ws_bytes // 8 + sc.GUARD, 7.5, dtype=np.float64))
    out = mem.upload(np.full(total + 2 * sc.GUARD, sc.SENTINEL, dtype=np.float32))
    src_dev, cap_dev, phi_dev = mem.upload(sources.reshape(-1)), mem.upload(capsules.reshape(-1)), mem.upload(phi.reshape(-1))
    L = (ct.c_double * 3)(*room)
    lib.call("al_ism_shoebox_bands", mem.ptr(src_dev), n, mem.ptr(cap_dev), n_cap, L, beta.ctypes.data_as(ct.POINTER(ct.c_double)), n_bands,
             mem.ptr(phi_dev), int(half), float(c), float(fs), -1 if max_order is None else int(max_order), int(ir_len), int(pitch),
             mem.ptr(ws), ws_bytes, mem.ptr(out) + 4 * sc.GUARD, mem.stream())
    host = np.asarray(mem.download(out))
    assert np.all(host[:sc.GUARD] == sc.SENTINEL) and np.all(host[sc.GUARD + total:] == sc.SENTINEL), "guard overwritten"
    assert not np.any(host[sc.GUARD: sc.GUARD + total] == sc.SENTINEL), "a sample was not written"
    assert np.all(np.asarray(mem.download(ws))[ws_bytes // 8:] == 7.5), "the workspace's guard was overwritten"
    return host[sc.GUARD: sc.GUARD + total].reshape(n_cap, n, pitch).copy()


def check_parity(r, room, beta, centres, half, sources, capsules, ir_len, fs, max_order=None, what=None, **kw):
    rows = run_bands_abi(r, room, beta, centres, half, sources, capsules, ir_len, fs, max_order=max_order, **kw)
    assert np.all(bits(rows[:, :, ir_len:]) == 0), "pad samples must be +0"
    h64, bound = restate(room, beta, centres, half, sources, capsules, ir_len, fs, max_order=max_order)
    assert_within(rows[:, :, :ir_len], h64, bound, what)
    return rows[:, :, :ir_len], h64


# ----------------------------------------------------------------------------- 0. the band filters
def run_band_filters():
    for fs, half, centres in ((48000.0, 256, CENTRES_16K), (48000.0, 512, CENTRES_16K), (16000.0, 256, CENTRES_16K), (8000.0, 16, CENTRES_16K[:5]),
                              (8000.0, 64, CENTRES_16K[:5]), (16000.0, 1, CENTRES_16K), (16000.0, 300, (250.0, 1000.0, 3000.0)),
                              (48000.0, 64, CENTRES_8)):
        phi = shoebox.band_filters(centres, fs, half)
        assert phi.shape == (len(centres), 2 * half + 1) and phi.dtype == np.float64 and phi.flags.c_contiguous
        delta = np.zeros(2 * half + 1)
        delta[half] = 1.0
        assert np.abs(phi.sum(axis=0) - delta).max() <= 1e-15, (fs, half)                  # sum_b phi_b = delta
        assert np.array_equal(phi, phi[:, ::-1]), (fs, half)                                # phi_b[-j] = phi_b[j], bit for bit
    one = shoebox.band_filters((1000.0,), 16000.0, 64)
    delta = np.zeros(129)
    delta[64] = 1.0
    assert np.abs(one[0] - delta).max() <= 1e-15                                            # B = 1: the impulse
    # the 125 Hz band of the default table passes its own centre and stops the top one
    phi = shoebox.band_filters(shoebox.OCTAVE_CENTRES, 48000.0, 512)
    j = np.arange(-512, 513)
    gain = lambda b, f: float((phi[b] * np.cos(2.0 * np.pi * f * j / 48000.0)).sum())       # noqa: E731
    assert 0.85 < gain(0, 125.0) < 1.0 and abs(gain(0, 4000.0)) < 1e-3 and 0.99 < gain(5, 8000.0) < 1.01
    assert shoebox.OCTAVE_CENTRES == (125, 250, 500, 1000, 2000, 4000)
    assert np.array_equal(shoebox.band_filters(sample_rate=48000.0), phi)                   # the defaults: octaves, half 512
    bad = [dict(centres=()), dict(centres=tuple(range(1, 10))), dict(centres=(500.0, 250.0)), dict(centres=(250.0, 250.0)),
           dict(centres=(0.0, 100.0)), dict(centres=(-5.0,)), dict(centres=(100.0, 8000.0)), dict(centres=(100.0, np.nan)),
           dict(centres=((100.0, 200.0),)), dict(half=0), dict(half=-3), dict(half=2.5), dict(half=True), dict(half=shoebox.MAX_BAND_HALF + 1),
           dict(sample_rate=0.0), dict(sample_rate=np.inf)]
    for change in bad:
        with pytest.raises(ValueError):
            shoebox.band_filters(**dict(dict(centres=(250.0, 1000.0), sample_rate=16000.0, half=16), **change))


# ----------------------------------------------------------------------------- 1. parity with the restatement
def _cfg(room="oblong", order=None, n_bands=3, half=16, pairs="1x1", fs=FS, ir_len=None):
    return (room, order, n_bands, half, pairs, fs, ir_len)


PARITY = (
    [_cfg(room, order, n_bands=3, half=64) for room in sc.ROOMS for order in (0, 1, 3, None)]
    + [_cfg(n_bands=nb, half=16, order=order) for nb in (1, 2, 5, 6) for order in (1, None)]     # 5: a group of four and a group of one
    + [_cfg(n_bands=2, half=half, order=3) for half in (1, 16, 300)]
    + [_cfg("cubic", None, n_bands=5, half=300, pairs="3x5", ir_len=400)]
    + [_cfg("cubic", 1, n_bands=8, half=64, fs=48000.0, ir_len=600), _cfg("oblong", None, n_bands=8, half=16, pairs="3x5", fs=48000.0, ir_len=520)]
)


def run_parity(r, room, order, n_bands, half, pairs, fs, ir_len):
    src, cap = (sc.SOURCES_5, sc.CAPSULES_3) if pairs == "3x5" else (sc.SOURCES_5[1:2], sc.CAPSULES_3[:1])
    ir_len = sc.parity_ir_len(order, 16000) if ir_len is None else ir_len
    rows, h64 = check_parity(r, sc.ROOMS[room], BETA_8[:, :n_bands], centres_of(n_bands, fs), half, src, cap, ir_len, fs, max_order=order,
                             what=f"{room} order={order} B={n_bands} half={half} {pairs} fs={fs:.0f}")
    assert np.abs(rows).max() > 0


EDGES = [(ir_len, 16) for ir_len in sc.EDGE_LEN] + [(5, 300), (257, 300), (1, 1)]


def run_edge_length(r, ir_len, half):
    """shoebox_cases.run_edge_length's room and points: row lengths around the tap count and the tile, the band sums reaching `half`
    past either end of the row (ir_len = 5 with half = 300: 605 band samples behind five outputs)."""
    room = (2.4, 2.0, 1.7)
    src = np.array([[0.5, 0.6, 0.7], [2.0, 1.5, 1.1]])
    cap = np.array([[1.9, 1.2, 0.9], [0.52, 0.63, 0.74]])     # the second capsule is 5 cm from the first source
    rows, _ = check_parity(r, room, BETA_8[:, 3:6], centres_of(3, FS), half, src, cap, ir_len, FS, what=f"edge ir_len={ir_len} half={half}")
    assert np.abs(rows).max() > 0


def run_close_capsule(r):
    """A capsule 1 cm from the source: tau = 0.47 samples, forty taps of the direct path lie at s < 0.  The band sums keep them (the
    gather's tiles below sample 0 are not empty here); the direct path has the same gain in every band, so what the FIR brings back
    from them into the row is sum_b phi_b = delta times it, and the peak stays at sample 0."""
    room, ir_len, half = (3.0, 2.5, 2.2), 300, 64
    s = np.array([1.0, 1.2, 1.1])
    m = s + np.array([0.01, 0.0, 0.0])
    rows, h64 = check_parity(r, room, BETA_8[:, 3:6], centres_of(3, FS), half, s, m, ir_len, FS, max_order=2, what="capsule at 1 cm")
    assert int(np.argmax(np.abs(rows[0, 0]))) == 0 and rows[0, 0, 0] > 1.0 / (4 * np.pi * 0.01) * 0.5


def run_crowded_tile(r):
    """shoebox_cases.run_crowded_tile's room, row and pair with two bands: more than 2000 images (the broadband oracle's count;
    band 0 has no wall at 0 and keeps every one of them), so the gather's last tiles go through several windows of its 96-entry
    LDS list."""
    room, ir_len = (2.0, 1.6, 1.2), 600
    s, m = np.array([0.7, 0.5, 0.4]), np.array([1.4, 1.1, 0.8])
    rows, _ = check_parity(r, room, BETA_8[:, :2], centres_of(2, FS), 16, s, m, ir_len, FS, what="crowded tile")
    assert np.abs(rows).max() > 0 and np.all(BETA_8[:, 0] > 0)
    _, _, used = sc.oracle(room, (0.9, 0.95, 0.85, 0.9, 0.97, 0.8), s, m, ir_len, FS)
    assert used[0, 0] > 2000, used


# ----------------------------------------------------------------------------- 2. ties to the broadband oracle and entry
def run_equal_columns(r):
    """Equal band columns: sum_b phi_b = delta, so the row is the broadband row of shoebox_cases' oracle (an oracle this module's
    restatement has no part in), within the bands' bound."""
    room, ir_len, half, order = sc.ROOMS["oblong"], 520, 64, 3
    src, cap = sc.SOURCES_5[:2], sc.CAPSULES_3[:2]
    beta = np.repeat(np.asarray(sc.UNEQUAL_BETAS)[:, None], 3, axis=1)
    rows = run_bands_abi(r, room, beta, centres_of(3, FS), half, src, cap, ir_len, FS, max_order=order)
    y64, _, _ = sc.oracle(room, sc.UNEQUAL_BETAS, src, cap, ir_len, FS, max_order=order)
    _, bound = restate(room, beta, centres_of(3, FS), half, src, cap, ir_len, FS, max_order=order)
    # none of these pairs has a tap below sample 0, so the broadband oracle's cut at 0 removes nothing
    assert_within(rows[:, :, :ir_len], y64, bound, "equal columns against the broadband oracle")


def run_one_band_is_the_broadband_entry(r):
    """B = 1: phi_0 = delta to 1e-17, so the row agrees with al_ism_shoebox within the two bounds."""
    room, ir_len, order = sc.ROOMS["cubic"], 520, None
    src, cap = sc.SOURCES_5[:2], sc.CAPSULES_3[1:]
    beta = np.asarray(sc.UNEQUAL_BETAS)[:, None]
    for half in (1, 64):
        rows = run_bands_abi(r, room, beta, (1000.0,), half, src, cap, ir_len, FS, max_order=order)
        want = sc.run_abi(r, room, sc.UNEQUAL_BETAS, src, cap, ir_len, FS, max_order=order)
        y64, A, _ = sc.oracle(room, sc.UNEQUAL_BETAS, src, cap, ir_len, FS, max_order=order)
        _, bound = restate(room, beta, (1000.0,), half, src, cap, ir_len, FS, max_order=order)
        err = np.abs(rows[:, :, :ir_len].astype(np.float64) - want[:, :, :ir_len].astype(np.float64))
        assert np.all(err <= bound + 2.0 ** -24 * np.abs(y64) + 2.0 ** -30 * A), float(err.max())


def run_one_wall(r):
    """One reflecting wall (x0) at order 1, the other five at 0: two images.  The row is the broadband direct path plus
    sum_b beta_b phi_b convolved with the broadband reflection off a rigid wall, both from shoebox_cases' oracle; both paths are
    longer than half + 41 samples, so neither the oracle's cut at 0 nor the row's end at 700 touches them."""
    room, ir_len, half = sc.ROOMS["oblong"], 700, 64
    s, m = np.array([3.6, 0.5, 0.6]), np.array([0.6, 2.8, 2.0])
    centres = centres_of(5, FS)
    beta_x0 = np.array([0.9, 0.7, 0.5, 0.3, 0.15])
    beta = np.zeros((6, 5))
    beta[0] = beta_x0
    rows = run_bands_abi(r, room, beta, centres, half, s, m, ir_len, FS, max_order=1)
    direct, A_d, used = sc.oracle_pair(room, np.zeros(6), s, m, ir_len, FS, max_order=1)
    both, A_both, used2 = sc.oracle_pair(room, (1.0, 0, 0, 0, 0, 0), s, m, ir_len, FS, max_order=1)
    assert (used, used2) == (1, 2)
    reflection, A_r = both - direct, A_both - A_d
    first = np.flatnonzero(A_both)[0]
    assert first > half and np.flatnonzero(A_r)[-1] + half < ir_len - 1
    phi = shoebox.band_filters(centres, FS, half)
    # sum_b phi_b = delta: the direct path goes through unchanged
    want = direct + np.convolve(reflection, (beta_x0[:, None] * phi).sum(axis=0))[half: half + ir_len]
    # the bound with A_b = A_direct + A_reflection, the reflection's weighted by beta_b <= 1
    spread = sum(np.convolve(A_d + beta_x0[b] * A_r, np.abs(phi[b]))[half: half + ir_len] for b in range(5))
    assert_within(rows[0, 0, :ir_len], want, 2.0 ** -24 * np.abs(want) + 2.0 ** -30 * spread, "one wall")
    assert np.abs(want).max() > 0 and np.abs(np.convolve(reflection, phi[0])).max() > 0


# ----------------------------------------------------------------------------- 3. identity
def run_identity(r):
    room, ir_len, half, order = sc.ROOMS["oblong"], 520, 64, 4
    beta, centres = BETA_8[:, :5], centres_of(5, FS)
    run = lambda s=sc.SOURCES_5, m=sc.CAPSULES_3, **k: run_bands_abi(r, room, beta, centres, half, s, m, ir_len, FS, max_order=order, **k)   # noqa: E731
    one = run()
    assert np.array_equal(bits(one), bits(run())), "two runs differ"
    # THE WORKSPACE: exactly one pair per pass (15 passes), four per pass (the last pass is part full), all of them at once
    for per_pass in (1, 4):
        assert np.array_equal(bits(run(pairs_per_pass=per_pass)), bits(one)), ("the bits depend on the workspace size", per_pass)
    for ci, ni in ((0, 0), (1, 3), (2, 4)):
        alone = run(sc.SOURCES_5[ni], sc.CAPSULES_3[ci])
        assert np.array_equal(bits(alone[0, 0]), bits(one[ci, ni])), (ci, ni)
    wide = run(sc.SOURCES_5[:2], sc.CAPSULES_3[:2], pitch=768 + 8, pairs_per_pass=3)
    assert np.array_equal(bits(wide[:, :, :ir_len]), bits(one[:2, :2, :ir_len])) and np.all(bits(wide[:, :, ir_len:]) == 0)


# ----------------------------------------------------------------------------- 3b. the tail with bands
def _tcfg(M, F, ir_len=1100, n_bands=3, half=64, pairs="1x1", order=None, pitch=None, sid0=0, cid0=0, per_pass=None):
    return (M, F, ir_len, n_bands, half, pairs, order, pitch, sid0, cid0, per_pass)


TAIL_PARITY = (
    [_tcfg(M, F) for M in (0, 300, 1100, 5000) for F in (1, 100)]          # the start of the row, mid-tile, at and past its end
    + [_tcfg(300, 100, n_bands=5, half=16), _tcfg(300, 213, n_bands=2, half=300, order=3)]     # M + F = 513; LDS sized for 256, 512
    + [_tcfg(100, 60, ir_len=700, n_bands=2, half=600, order=1)]            # ... and for 1024
    + [_tcfg(0, 1, ir_len=256 + 1024 + 10, n_bands=2, half=16, order=1, sid0=0xFFFFFFF0, cid0=9)]     # a row of two k_ism_band_tail workgroups
    + [_tcfg(300, 100, ir_len=450), _tcfg(300, 100, ir_len=513), _tcfg(300, 100, ir_len=517, pitch=1024 + 512 + 8)]
    + [_tcfg(255, 1, ir_len=900, n_bands=5, half=64, pairs="3x5", order=1, pitch=1200, sid0=1, cid0=0xFFFFFFFD, per_pass=4)]
)


def run_tail_parity(r, M, F, ir_len, n_bands, half, pairs, order, pitch, sid0, cid0, per_pass):
    src, cap = tc.points(pairs)
    room, beta, centres = tc.ROOM, TAIL_BETA[:, :n_bands], centres_of(n_bands, FS)
    rows, ln_env = run_bands_tail_abi(r, room, beta, centres, half, src, cap, ir_len, FS, M, F, sid0=sid0, cid0=cid0, max_order=order,
                                      pitch=pitch, pairs_per_pass=per_pass)
    assert np.all(bits(rows[:, :, ir_len:]) == 0), "pad samples must be +0"
    h64, bound = restate_tail(room, beta, centres, half, src, cap, ir_len, FS, M, F, ln_env, SEED, sid0, cid0, max_order=order)
    assert_within(rows[:, :, :ir_len], h64, bound, f"tail M={M} F={F} ir_len={ir_len} B={n_bands} half={half} {pairs} order={order}")
    if ir_len > M + F:
        assert np.all(rows[:, :, M + F: ir_len] != 0.0), "a tail sample is zero"


def run_tail_tables(r):
    """Knot tables that do not lie on a line, differ from band to band and hold -inf: an interpolation in the wrong interval, with
    the p of another sample or with another band's knots fails by far; a dead knot gives exact zeros and no NaN."""
    src, cap = tc.points("1x1")
    room, beta, centres, half, ir_len, M, F = tc.ROOM, TAIL_BETA[:, :3], centres_of(3, FS), 16, 1100, 100, 60
    n_knots = shoebox.n_knots_of(ir_len)
    jagged = np.random.default_rng(4).uniform(-9.0, -2.0, (3, n_knots))
    for what, table in (("jagged", jagged), ("-inf", np.full((3, n_knots), -np.inf)),
                        ("one band dead from knot 2", np.where((np.arange(3)[:, None] == 1) & (np.arange(n_knots)[None, :] >= 2), -np.inf, jagged))):
        rows, _ = run_bands_tail_abi(r, room, beta, centres, half, src, cap, ir_len, FS, M, F, ln_env=table, max_order=1)
        h64, bound = restate_tail(room, beta, centres, half, src, cap, ir_len, FS, M, F, table, SEED, 0, 0, max_order=1)
        assert_within(rows[:, :, :ir_len], h64, bound, f"tail tables: {what}")
        if what == "-inf":
            assert np.all(rows[:, :, M + F:] == 0.0)


def run_tail_equal_bands(r):
    """Equal columns: psi_k = e_k delta, so the row is the broadband tail's (al_ism_shoebox_tail, restated by shoebox_tail_cases)
    except for the envelope's interpolation, linear in amplitude here and in the logarithm there: the two envelopes differ by a
    factor in [1, exp(Delta_k^2 / 8)], Delta_k = |ln_env[k + 1] - ln_env[k]| (Hoeffding's lemma)."""
    src, cap = tc.points("1x1")
    ir_len, M, F, half, order = 1100, 300, 100, 64, 3
    beta = np.repeat(np.asarray(tc.BETAS)[:, None], 3, axis=1)
    rows, ln_env = run_bands_tail_abi(r, tc.ROOM, beta, centres_of(3, FS), half, src, cap, ir_len, FS, M, F, max_order=order)
    assert np.array_equal(ln_env[0], ln_env[1]) and np.array_equal(ln_env[0], ln_env[2])
    wide, _ = tc.run_tail_abi(r, src, cap, ir_len, M, F, seed=SEED, max_order=order, ln_env=ln_env[0])
    y64, A = tc.image_oracle("1x1", order)
    h_wide, bound_wide = tc.restate(y64[0, 0], A[0, 0], ln_env[0], ir_len, M, F, SEED, 0, 0)
    _, bound = restate_tail(tc.ROOM, beta, centres_of(3, FS), half, src, cap, ir_len, FS, M, F, ln_env, SEED, 0, 0, max_order=order)
    delta = np.abs(np.diff(ln_env[0]))[np.arange(ir_len) // 256]
    _, w_l = tc.weights(ir_len, M, F)
    lift = (np.exp(delta * delta / 8.0) - 1.0) * w_l * tc.envelope(ln_env[0], ir_len) * np.abs(tc.restated_g(SEED, 0, 0, ir_len))
    err = np.abs(rows[0, 0, :ir_len].astype(np.float64) - wide[0, 0, :ir_len].astype(np.float64))
    allowed = bound[0, 0] + bound_wide + lift
    print(f"equal bands against the broadband tail: max err / allowed {float((err / allowed).max()):.3f}, the lift's share at most {float((lift / allowed).max()):.3f}")
    assert np.all(err <= allowed)
    assert delta.max() > 0.05                          # the envelope does decay between two knots


def run_tail_no_tail_bits(r):
    """M >= ir_len: the bits of the entry without a tail."""
    src, cap = tc.points("3x5")
    room, beta, centres, half, ir_len = tc.ROOM, TAIL_BETA[:, :5], centres_of(5, FS), 64, 520
    for pitch in (None, 768 + 8):
        want = run_bands_abi(r, room, beta, centres, half, src, cap, ir_len, FS, max_order=3, pitch=pitch)
        for M, F in ((ir_len, 1), (ir_len + 1000, 7), (1 << 40, 1), (ir_len, 1 << 62)):
            got, _ = run_bands_tail_abi(r, room, beta, centres, half, src, cap, ir_len, FS, M, F, max_order=3, pitch=pitch,
                                        ln_env=np.full((5, shoebox.n_knots_of(ir_len)), -3.0))
            assert np.array_equal(bits(got), bits(want)), ("the tail entry with mix >= ir_len differs from al_ism_shoebox_bands", M, F, pitch)


def run_tail_identity(r):
    src, cap = tc.points("3x5")
    room, beta, centres, half, ir_len, M, F, sid0, cid0 = tc.ROOM, TAIL_BETA[:, :5], centres_of(5, FS), 64, 700, 100, 50, 7, 3
    run = lambda s=src, m=cap, **k: run_bands_tail_abi(r, room, beta, centres, half, s, m, ir_len, FS, M, F,   # noqa: E731
                                                       **dict(dict(sid0=sid0, cid0=cid0, max_order=2), **k))[0]
    one = run()
    assert np.array_equal(bits(one), bits(run())), "two runs differ"
    for per_pass in (1, 4):
        assert np.array_equal(bits(run(pairs_per_pass=per_pass)), bits(one)), ("the bits depend on the workspace size", per_pass)
    wide = run(pitch=1024 + 256 + 4, pairs_per_pass=2)
    assert np.array_equal(bits(wide[:, :, :ir_len]), bits(one[:, :, :ir_len])) and np.all(bits(wide[:, :, ir_len:]) == 0)
    for ci, ni in ((0, 0), (2, 4)):
        alone = run(src[ni], cap[ci], sid0=sid0 + ni, cid0=cid0 + ci)
        assert np.array_equal(bits(alone[0, 0]), bits(one[ci, ni])), (ci, ni)
        other = run(src[ni], cap[ci], sid0=sid0 + ni, cid0=cid0 + ci, seed=SEED + 1)
        # the noise reaches `half` samples back from M + 1 through the FIR, under a fade weight that is 0 at M itself
        assert np.array_equal(bits(other[0, 0, :M + 1]), bits(alone[0, 0, :M + 1]))
        assert np.all(other[0, 0, M + 1: ir_len] != alone[0, 0, M + 1: ir_len])


def run_tail_abi_refusals(r):
    mem, lib = r.mem, r.lib
    src, cap = mem.upload(np.array([1.0, 1.0, 1.0])), mem.upload(np.array([2.0, 1.5, 1.2]))
    out = mem.upload(np.full(64, sc.SENTINEL, dtype=np.float32))
    phi = mem.upload(shoebox.band_filters((500.0, 2000.0), 16000.0, 8).reshape(-1))
    env = mem.upload(np.full(4, -3.0))
    per_pair = per_pair_bytes(r, 2, 8, 30, 10, 5)
    assert per_pair == 2 * 256 * 8
    ws = mem.upload(np.full(per_pair // 8, 7.5))
    good = dict(sources=mem.ptr(src), n=1, capsules=mem.ptr(cap), n_cap=1, L=(3.0, 2.5, 2.0), beta=(0.5,) * 12, n_bands=2, phi=mem.ptr(phi),
                half=8, c=343.0, fs=16000.0, order=-1, ir_len=30, pitch=32, mix=10, fade=5, seed=1, sid0=0, cid0=0, env=mem.ptr(env),
                n_knots=2, ws=mem.ptr(ws), ws_bytes=per_pair, out=mem.ptr(out))

    def call(**change):
        a = dict(good, **change)
        return lib.call("al_ism_shoebox_bands_tail", a["sources"], a["n"], a["capsules"], a["n_cap"], (ct.c_double * 3)(*a["L"]),
                        (ct.c_double * len(a["beta"]))(*a["beta"]), a["n_bands"], a["phi"], a["half"], a["c"], a["fs"], a["order"], a["ir_len"],
                        a["pitch"], a["mix"], a["fade"], a["seed"], a["sid0"], a["cid0"], a["env"], a["n_knots"], a["ws"], a["ws_bytes"],
                        a["out"], mem.stream())

    bad = [(dict(L=(0.0, 2.5, 2.0)), "al_ism_shoebox: "), (dict(beta=(0.5,) * 11 + (1.5,)), "al_ism_shoebox: "), (dict(pitch=28), "al_ism_shoebox: "),
           (dict(n_bands=9), "n_bands must be in 1 .. 8"), (dict(half=0), "half must be in"), (dict(half=1025), "half must be in 1 .. 1024 with a tail"),
           (dict(phi=None), "null filter table"), (dict(ws=None), "workspace must be"), (dict(ws_bytes=per_pair - 8), "workspace smaller than"),
           (dict(mix=-1), "mix must be >= 0"), (dict(fade=0), "fade must be >= 1"), (dict(sid0=-1), "must be >= 0"),
           (dict(cid0=1 << 32), "must not exceed 2^32"), (dict(n_knots=3), "n_knots must be"), (dict(env=None), "null envelope table"),
           (dict(out=mem.ptr(out) + 4), "out must be 16-byte aligned")]
    for change, needle in bad:
        nd.raises_badarg(lambda: call(**change), "al_ism_shoebox_bands_tail failed", needle)
    assert np.all(np.asarray(mem.download(out)) == sc.SENTINEL), "a refused call wrote"
    assert call() == 0
    # the workspace of a row with a tail is sized by M + F, not by ir_len
    assert per_pair_bytes(r, 2, 8, 1000, 10, 5) == per_pair < per_pair_bytes(r, 2, 8, 1000)


# ----------------------------------------------------------------------------- 3c. schedule independence
def run_shake_rows(r):
    """{name: (rows, bound)} of one call without a tail and one with, both held to their restatement first: three chunks of taps per
    band (half = 300), five bands, two passes over the workspace, so every LDS hand-over of k_ism_band_combine happens many times per
    workgroup; with the tail k_ism_band_combine<true> under the fade and k_ism_band_tail past it.  tests/test_gpu_shoebox_bands.py
    compares the rows of differently scheduled builds bit for bit."""
    room, half, src, cap = sc.ROOMS["oblong"], 300, sc.SOURCES_5[:3], sc.CAPSULES_3[:2]
    centres = centres_of(5, FS)
    plain = run_bands_abi(r, room, BETA_8[:, :5], centres, half, src, cap, 700, FS, max_order=3, pairs_per_pass=4)[:, :, :700]
    h64, bound = restate(room, BETA_8[:, :5], centres, half, src, cap, 700, FS, max_order=3)
    assert_within(plain, h64, bound, "schedule independence: no tail")
    tailed, ln_env = run_bands_tail_abi(r, room, TAIL_BETA[:, :5], centres, half, src, cap, 1100, FS, 300, 100, max_order=3, pairs_per_pass=4)
    h64_t, bound_t = restate_tail(room, TAIL_BETA[:, :5], centres, half, src, cap, 1100, FS, 300, 100, ln_env, SEED, 0, 0, max_order=3)
    assert_within(tailed[:, :, :1100], h64_t, bound_t, "schedule independence: tail")
    return {"bands": (plain, bound), "bands_tail": (tailed[:, :, :1100], bound_t)}


# ----------------------------------------------------------------------------- 4. materials
def run_materials():
    table = shoebox.load_materials(FIXTURE)
    raw = json.load(open(FIXTURE))
    assert len(table) == 30 and all(set(m) == {"name", "absorption"} for m in raw["materials"])
    assert os.path.getsize(FIXTURE) < 16384
    for name in ("Default", "Carpet", "Carpet, Heavy", "Acoustic Tile", "Wood Floor", "wood, Thin", "Sound Proof"):
        assert name in table
    alpha = lambda b: 1.0 - np.asarray(b) ** 2     # noqa: E731
    carpet = shoebox.material_betas(table, "Carpet")
    assert carpet.shape == (6, 6) and np.all(carpet == carpet[0])
    assert np.allclose(alpha(carpet[0]), (0.01, 0.05, 0.1, 0.2, 0.45, 0.65), rtol=2.0 ** -23, atol=0)          # the file holds float32 values
    assert np.allclose(alpha(shoebox.material_betas(table, "Default")), 0.1, rtol=2.0 ** -23, atol=0)          # two points, 20 Hz and 20 kHz
    # linear in log2 f between two points, held at the end values outside
    got = alpha(shoebox.material_betas(table, "Carpet", (62.5, 125.0 * 2 ** 0.5, 3000.0, 4000.0, 16000.0))[0])
    f32 = lambda v: float(np.float32(v))           # noqa: E731
    want = (f32(0.01), 0.5 * (f32(0.01) + f32(0.05)), f32(0.45) + np.log2(1.5) * (f32(0.65) - f32(0.45)), f32(0.65), f32(0.65))
    assert np.allclose(got, want, rtol=1e-12, atol=0)
    walls = ("Carpet", "Acoustic Tile", "Brick", "Glass", "Wood Floor", "Concrete")
    six = shoebox.material_betas(table, walls, (250.0, 1000.0))
    assert six.shape == (2 * 3, 2)
    for i, name in enumerate(walls):
        assert np.array_equal(six[i], shoebox.material_betas(table, name, (250.0, 1000.0))[0])
    assert np.all(shoebox.material_betas(table, "Sound Proof") == 0.0)
    with pytest.raises(KeyError):
        shoebox.material_betas(table, "Unobtainium")
    with pytest.raises(KeyError):
        shoebox.material_betas(table, ("Carpet",) * 5 + ("carpet",))
    with pytest.raises(ValueError):
        shoebox.material_betas(table, ("Carpet",) * 5)
    return table


# ----------------------------------------------------------------------------- 5. refusals
def run_abi_refusals(r):
    mem, lib = r.mem, r.lib
    src, cap = mem.upload(np.array([1.0, 1.0, 1.0])), mem.upload(np.array([2.0, 1.5, 1.2]))
    out = mem.upload(np.full(64, sc.SENTINEL, dtype=np.float32))
    phi = mem.upload(shoebox.band_filters((500.0, 2000.0), 16000.0, 8).reshape(-1))
    per_pair = per_pair_bytes(r, 2, 8, 30)
    assert per_pair == 2 * 256 * 8
    ws = mem.upload(np.full(per_pair // 8 + 2, 7.5))
    good = dict(sources=mem.ptr(src), n=1, capsules=mem.ptr(cap), n_cap=1, L=(3.0, 2.5, 2.0), beta=(0.5,) * 12, n_bands=2, phi=mem.ptr(phi),
                half=8, c=343.0, fs=16000.0, order=-1, ir_len=30, pitch=32, ws=mem.ptr(ws), ws_bytes=per_pair, out=mem.ptr(out))

    def call(**change):
        a = dict(good, **change)
        L = None if a["L"] is None else (ct.c_double * 3)(*a["L"])
        beta = None if a["beta"] is None else (ct.c_double * len(a["beta"]))(*a["beta"])
        return lib.call("al_ism_shoebox_bands", a["sources"], a["n"], a["capsules"], a["n_cap"], L, beta, a["n_bands"], a["phi"], a["half"],
                        a["c"], a["fs"], a["order"], a["ir_len"], a["pitch"], a["ws"], a["ws_bytes"], a["out"], mem.stream())

    # everything the plain entry refuses, with its messages; a bad coefficient in either band's column
    old = [dict(L=(0.0, 2.5, 2.0)), dict(L=(3.0, 2.5, float("inf"))), dict(c=0.0), dict(c=float("nan")), dict(fs=-1.0),
           dict(beta=(0.5,) * 5 + (1.01,) + (0.5,) * 6), dict(beta=(0.5,) * 11 + (-0.01,)), dict(beta=(float("nan"),) + (0.5,) * 11),
           dict(n=0), dict(n_cap=0), dict(ir_len=0), dict(pitch=28), dict(pitch=34, ir_len=33), dict(order=-2), dict(sources=None),
           dict(capsules=None), dict(out=None), dict(L=None), dict(beta=None)]
    for change in old:
        nd.raises_badarg(lambda: call(**change), "al_ism_shoebox_bands failed", "al_ism_shoebox: ")
    new = [(dict(n_bands=0), "n_bands must be in 1 .. 8"), (dict(n_bands=9), "n_bands must be in 1 .. 8"), (dict(n_bands=-1), "n_bands must be"),
           (dict(half=0), "half must be in 1 .. 4096"), (dict(half=-8), "half must be in"), (dict(half=4097), "half must be in 1 .. 4096"),
           (dict(phi=None), "null filter table"), (dict(ws=None), "workspace must be 16-byte aligned"),
           (dict(ws=mem.ptr(ws) + 8), "workspace must be 16-byte aligned"), (dict(ws_bytes=per_pair - 1), "workspace smaller than"),
           (dict(ws_bytes=0), "workspace smaller than"), (dict(ws_bytes=-per_pair), "workspace smaller than"),
           (dict(L=(5.0e-5, 2.5, 2.0), half=4096, ws_bytes=1 << 40), "mirror cells")]
    for change, needle in new:
        nd.raises_badarg(lambda: call(**change), "al_ism_shoebox_bands: ", needle)
    assert np.all(np.asarray(mem.download(out)) == sc.SENTINEL), "a refused call wrote"
    assert np.all(np.asarray(mem.download(ws)) == 7.5), "a refused call wrote the workspace"
    for args in ((0, 8, 30, -1, 0), (9, 8, 30, -1, 0), (2, 0, 30, -1, 0), (2, 4097, 30, -1, 0), (2, 8, 0, -1, 0), (2, 8, 30, 5, 0)):
        assert lib.call("al_ism_shoebox_bands_workspace_bytes", *args) == _hip.AL_E_BADARG, args
    assert lib.call("al_ism_shoebox_bands_workspace_bytes", 8, 4096, 1, -1, 0) == 8 * (8192 + 256) * 8
    assert lib.call("al_ism_shoebox_bands_workspace_bytes", 2, 8, 1000, 100, 50) == 2 * 256 * 8      # a tail's image part: min(ir_len, M + F)
    assert call() == 0
    assert call(ws_bytes=per_pair + 15) == 0                                                       # part of a pair more: one pair per pass
    assert call(order=0, beta=(0.0, 1.0) * 6) == 0


def run_python_errors(r):
    room, s, m = (3.0, 2.5, 2.0), [[1.0, 1.0, 1.0]], [[2.0, 1.5, 1.2]]
    Bands = shoebox.ShoeboxBands
    two = Bands((500.0, 2000.0), 8)
    ok = dict(room=room, betas=np.full((6, 2), 0.5), sources=s, capsules=m, ir_len=64, sample_rate=16000, bands=two)
    bad = [dict(betas=(0.5,) * 6), dict(betas=np.full((6, 3), 0.5)), dict(betas=np.full((2, 6), 0.5)), dict(betas=np.full((6, 2), 1.5)),
           dict(betas=np.full((6, 2), np.nan)), dict(bands=dict(centres=(500.0, 2000.0), half=8)), dict(bands=(500.0, 2000.0)),
           dict(bands=Bands((500.0, 8000.0), 8)), dict(bands=Bands((2000.0, 500.0), 8)), dict(bands=Bands((500.0, 2000.0), 0)),
           dict(bands=Bands((500.0, 2000.0), 2.5)), dict(bands=Bands((500.0, 2000.0), shoebox.MAX_BAND_HALF + 1)),
           dict(bands=Bands(tuple(100.0 * k for k in range(1, 10)), 8), betas=np.full((6, 9), 0.5)),
           dict(patterns=shoebox.omni()[None, None, :]),                      # not yet: K x B gains per image
           dict(tail=shoebox.ShoeboxTail(seed=1), betas=np.array([[0.5, 0.0]] + [[0.5, 0.5]] * 5)),      # a tail: every beta[:, b] > 0
           dict(tail=shoebox.ShoeboxTail(seed=1), bands=Bands((500.0, 2000.0), shoebox.MAX_BAND_TAIL_HALF + 1)),
           dict(tail=shoebox.ShoeboxTail(seed=1), capsule_id0=1 << 32), dict(tail=shoebox.ShoeboxTail(seed=1), source_id0=-1),
           dict(workspace_cap=-1), dict(workspace_cap=1.5)]
    for change in bad:
        with pytest.raises(ValueError):
            shoebox.shoebox_irs_device(r, **dict(ok, **change))
    with pytest.raises(ValueError, match="not yet"):
        shoebox.shoebox_irs_device(r, **dict(ok, patterns=shoebox.omni()[None, None, :]))
    buf, strides, n = shoebox.shoebox_irs_device(r, **ok)
    assert strides == (64, 64) and n == 64
    buf, strides, n = shoebox.shoebox_irs_device(r, **dict(ok, ir_len=600, tail=shoebox.ShoeboxTail(seed=5)))
    assert strides == (600, 600) and n == 600
    # the workspace cap does not change a bit: one pair per pass (a cap of 0 still gives one pair) against all at once
    many = dict(ok, sources=sc.SOURCES_5[:3] * 0.5, capsules=[[2.0, 1.5, 1.2], [2.5, 0.5, 0.7]], ir_len=300)
    a = np.asarray(r.mem.download(shoebox.shoebox_irs_device(r, **many)[0]))
    b = np.asarray(r.mem.download(shoebox.shoebox_irs_device(r, **dict(many, workspace_cap=0))[0]))
    assert np.array_equal(bits(a[:6 * 300]), bits(b[:6 * 300])) and np.abs(a[:6 * 300]).max() > 0
    assert Bands.from_dict(json.loads(json.dumps(two.to_dict()))) == two and Bands().centres == shoebox.OCTAVE_CENTRES and Bands().half == 512
    table = shoebox.load_materials(FIXTURE)
    for kw in (dict(betas=(0.5,) * 6, bands=two), dict(betas=np.full((6, 2), 0.5)), dict(rt60=0.4, bands=two), dict(materials="Carpet"),
               dict(materials="Carpet", material_table=table, betas=(0.5,) * 6), dict(materials=("Carpet",) * 5, material_table=table),
               dict(betas=np.array([[0.5, 0.0]] + [[0.5, 0.5]] * 5), bands=two, tail=shoebox.ShoeboxTail())):
        with pytest.raises(ValueError):
            core.ShoeboxIRState(room, sample_rate=16000, **kw)
    with pytest.raises(KeyError):
        core.ShoeboxIRState(room, sample_rate=16000, materials="Unobtainium", material_table=table)
    st = core.ShoeboxIRState(room, betas=np.full((6, 2), 0.5), bands=two, ir_len=64, sample_rate=16000, renderer=r)
    with pytest.raises(ValueError, match="not yet"):
        st.add_foa_listener("foa", [1.0, 1.0, 1.0])


# ----------------------------------------------------------------------------- 6. the state and the scene
WALLS = ("Carpet, Heavy", "Acoustic Tile", "Brick", "Glass", "Wood Floor", "Concrete")
STATE_BANDS = dict(centres=[125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0], half=64)


def run_state(r):
    table = shoebox.load_materials(FIXTURE)
    room, ir_len = sc.ROOMS["oblong"], 333
    st = core.ShoeboxIRState(room, materials=WALLS, material_table=table, bands=STATE_BANDS, ir_len=ir_len, sample_rate=sc.SR, max_order=3,
                             renderer=r)
    assert st.bands == shoebox.ShoeboxBands(tuple(STATE_BANDS["centres"]), 64) and st.betas.shape == (6, 6) and st.materials == list(WALLS)
    assert np.array_equal(st.betas, shoebox.material_betas(table, WALLS))
    st.add_microphone("mic000", sc.CAPSULES_3)
    st.add_emitters(sc.SOURCES_5[:1])
    st.add_emitters(sc.SOURCES_5[1:4])
    st.simulate()
    t = st.irs["mic000"]
    assert isinstance(t, shoebox.DeviceIRTensor) and t.shape == (3, 4, ir_len)
    first = np.array(np.asarray(t))
    h64, bound = restate(room, st.betas, STATE_BANDS["centres"], 64, sc.SOURCES_5[:4], sc.CAPSULES_3, ir_len, float(sc.SR), max_order=3)
    assert_within(first, h64, bound, "state")
    # the JSON round trip: betas, bands and names are stored, no material file is needed to load, the bits come back
    d = json.loads(json.dumps(st.to_dict()))
    assert d["shoebox"]["bands"] == STATE_BANDS and d["shoebox"]["materials"] == list(WALLS)
    assert np.array_equal(np.asarray(d["shoebox"]["betas"]), st.betas)
    again = core.ShoeboxIRState.from_dict(d, renderer=r)
    assert again.bands == st.bands and again.materials == list(WALLS) and np.array_equal(again.betas, st.betas)
    again.simulate()
    assert np.array_equal(bits(np.asarray(again.irs["mic000"])), bits(first))
    assert json.loads(json.dumps(again.to_dict())) == d
    # with a tail: every band under its own envelope, the bits again from the JSON
    tail = dict(mix_time=0.012, fade_time=0.004, rt60=None, seed=0x1234567890ABCDEF)           # M = 192, F = 64 at 16 kHz
    walls = ("Carpet, Heavy", "Acoustic Tile", "Brick", "Glass", "Wood Floor", "Curtain")        # none absorbs everything
    tailed = core.ShoeboxIRState(room, materials=walls, material_table=table, bands=STATE_BANDS, ir_len=900, sample_rate=sc.SR, renderer=r,
                                 tail=tail)
    tailed.add_microphone("mic000", sc.CAPSULES_3[:2])
    tailed.add_microphone("mic001", sc.CAPSULES_3[2:])
    tailed.add_emitters(sc.SOURCES_5[:2])
    tailed.simulate()
    M, F = shoebox.tail_samples(tailed.tail, room, sc.SR)
    assert (M, F) == (192, 64)
    ln_env = band_envelopes(room, tailed.betas, 900, float(sc.SR), M)
    for alias, caps, cid0 in (("mic000", sc.CAPSULES_3[:2], 0), ("mic001", sc.CAPSULES_3[2:], 2)):     # capsules numbered through the microphones
        h64, bound = restate_tail(room, tailed.betas, STATE_BANDS["centres"], 64, sc.SOURCES_5[:2], caps, 900, float(sc.SR), M, F, ln_env,
                                  tail["seed"], 0, cid0)
        assert_within(np.asarray(tailed.irs[alias]), h64, bound, f"state with a tail, {alias}")
    d_t = json.loads(json.dumps(tailed.to_dict()))
    assert d_t["shoebox"]["tail"] == tail and d_t["shoebox"]["bands"] == STATE_BANDS
    again_t = core.ShoeboxIRState.from_dict(d_t, renderer=r)
    again_t.simulate()
    for alias in ("mic000", "mic001"):
        assert np.array_equal(bits(np.asarray(again_t.irs[alias])), bits(np.asarray(tailed.irs[alias]))), alias
    # the default bands with materials; betas (6, B) given directly carry no names
    assert core.ShoeboxIRState(room, materials="Carpet", material_table=table, sample_rate=sc.SR).bands == shoebox.ShoeboxBands()
    plain_b = core.ShoeboxIRState(room, betas=st.betas, bands=st.bands, ir_len=ir_len, sample_rate=sc.SR, max_order=3, renderer=r)
    assert plain_b.materials is None and "materials" not in plain_b.to_dict()["shoebox"]
    # A PRE-BANDS DICTIONARY (as the parent commit wrote it: six betas, no "bands", no "materials") loads unchanged
    old = {"backend": "SHOEBOX", "sample_rate": sc.SR, "emitters": {"emitters000": sc.SOURCES_5[:2].tolist()},
           "microphones": {"mic000": {"micarray_type": "MicArray", "coordinates_absolute": sc.CAPSULES_3.tolist(), "n_capsules": 3}},
           "shoebox": {"room": list(room), "betas": list(sc.UNEQUAL_BETAS), "rt60": None, "ir_len": 300, "c": 343.0, "max_order": 2}}
    loaded = core.ShoeboxIRState.from_dict(json.loads(json.dumps(old)), renderer=r)
    assert loaded.bands is None and loaded.materials is None and loaded.betas.shape == (6,)
    assert "bands" not in loaded.to_dict()["shoebox"] and "materials" not in loaded.to_dict()["shoebox"]
    assert loaded.to_dict()["shoebox"] == old["shoebox"]
    loaded.simulate()
    want = sc.run_abi(r, room, sc.UNEQUAL_BETAS, sc.SOURCES_5[:2], sc.CAPSULES_3, 300, sc.SR, max_order=2)
    assert np.array_equal(bits(np.asarray(loaded.irs["mic000"])), bits(want[:, :, :300]))


def _band_energy(x, fs, lo_hz, hi_hz):
    spec = np.abs(np.fft.rfft(x, axis=-1)) ** 2
    f = np.fft.rfftfreq(x.shape[-1], 1.0 / fs)
    return float(spec[..., (f >= lo_hz) & (f < hi_hz)].sum())


def run_end_to_end(r, monkeypatch, tmp_path):
    """A room of heavy carpet on every wall (2 % absorption at 125 Hz, 63 % at 4 kHz), rendered by Scene.generate() without the
    tensor touching the host, equal to the same scene on StaticIRState(np.asarray(tensor)) and to the scene from its JSON.  THE
    SIGN CHECK ON THE MODEL (not a tolerance): from an early window of the IR to a late one the energy above 2 kHz falls faster
    than the energy below 500 Hz."""
    table = shoebox.load_materials(FIXTURE)
    room, ir_len = (4.1, 3.3, 2.6), 1203
    st = core.ShoeboxIRState(room, materials="Carpet, Heavy", material_table=table, bands=dict(centres=list(CENTRES_16K), half=64),
                             ir_len=ir_len, sample_rate=sc.SR, renderer=r)
    st.add_microphone("mic000", np.array([[2.0, 1.6, 1.2], [2.05, 1.6, 1.2]]))
    st.add_emitters([[0.8, 0.9, 1.0]], alias="static")
    st.add_emitters(np.linspace([3.2, 0.6, 1.5], [3.4, 2.8, 1.1], 3), alias="moving")
    scene = sc._add_events(core.Scene(1.2, st, sample_rate=sc.SR))

    def refuse(*a, **k):
        raise AssertionError("an IR tensor went through the host")

    real_upload = engine.Renderer.upload_irs
    monkeypatch.setattr(engine.Renderer, "upload_irs", refuse)
    got = {k: np.array(v) for k, v in scene.generate().items()}
    tensor = st.irs["mic000"]
    assert tensor._host is None, "the render downloaded the IR tensor"
    path = tmp_path / "shoebox_bands_scene.json"
    scene.to_json(str(path))
    meta = json.loads(path.read_text())["state"]["shoebox"]
    assert meta["materials"] == ["Carpet, Heavy"] * 6 and meta["bands"]["half"] == 64 and np.asarray(meta["betas"]).shape == (6, 6)
    again = core.Scene.from_json(str(path), {a: e._raw for a, e in scene.events.items()})
    assert isinstance(again.state, core.ShoeboxIRState) and again.state.bands == st.bands
    again.state.renderer = r
    got_again = sc._render(again)
    monkeypatch.setattr(engine.Renderer, "upload_irs", real_upload)

    host = np.asarray(tensor)
    want = sc._render(sc._add_events(core.Scene(1.2, core.StaticIRState({"mic000": host}), sample_rate=sc.SR)))
    assert want["mic000"].shape == (2, round(1.2 * sc.SR)) and np.abs(want["mic000"]).max() > 0
    assert np.array_equal(bits(got["mic000"]), bits(want["mic000"]))
    assert np.array_equal(bits(got_again["mic000"]), bits(want["mic000"]))
    # two windows of the rendered IRs: 10 .. 30 ms and 50 .. 70 ms
    early, late = host[:, :, 160:480].astype(np.float64), host[:, :, 800:1120].astype(np.float64)
    high = _band_energy(late, sc.SR, 2000.0, 8000.0) / _band_energy(early, sc.SR, 2000.0, 8000.0)
    low = _band_energy(late, sc.SR, 0.0, 500.0) / _band_energy(early, sc.SR, 0.0, 500.0)
    print(f"materials room: late / early energy above 2 kHz {high:.4f}, below 500 Hz {low:.4f}")
    assert high < low
