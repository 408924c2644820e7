"""Scenarios of the rigid-sphere receivers of the device shoebox IR generator (al_ism_shoebox_sphere, shoebox.sphere_filters,
shoebox.sphere_diffuse_filter, shoebox.shoebox_sphere_irs_device, core.ShoeboxIRState.add_sphere_microphone / add_binaural_listener)
and the float64 numpy restatement of their definition (DESIGN.md "Shoebox IRs: rigid-sphere receivers"; no reference code computes
this).  tests/test_hostemu_shoebox_sphere.py runs them on the host-emulated kernels, tests/test_gpu_shoebox_sphere.py on the gfx950
build.

THE DEFINITION.  Everything of shoebox_cases, shoebox_tail_cases, shoebox_bands_cases and shoebox_source_cases stands.  A sphere has the
centre o and C capsules with unit directions n_c; images are taken relative to o (R = image - o, d = |R|, u = R / d, tau = d fs / c)
with the amplitude A = prod beta^k / (4 pi d) gs exp(-m d).  With mu = clamp(n_c . u, -1, 1) and
    P_0 = 1, P_1 = mu, P_{l+1} = ((2 l + 1) mu P_l - l P_{l-1}) / (l + 1)             (float64, this order)
    y_l[s] = sum_images A P_l(mu) tap(s - tau)      at every integer s in [-half, y_end + half), l < n_orders
    y(t)   = sum_l sum_{j = -half .. half} b_l[j] y_l[t - j],   h[t] = float32(y(t)), pads +0,
b the table handed to the entry ((n_orders, 2 half + 1); shoebox.sphere_filters gives the physical one, the entry takes any).

THE BOUND (derived as the sibling modules derive theirs, not tuned), every sample, none excluded.  With A[s] the sum of
|A| (|ws| + |vs|_2) over the images with a tap at s (|P_l| <= 1 on [-1, 1]):
    |h - h64| <= 2^-24 |h64| + (2^-30 + n_orders^2 2^-49) sum_l sum_j |b_l[j]| A[t - j]
The first term is the one rounding to float32.  2^-30 A is shoebox_source_cases' bound on an image sum (float64 tau against a tap
slope of about pi, libm differences), carried through the FIR, whose own float64 accumulation of at most 64 * 129 products adds
8256 * 2^-53 = 2^-40 of sum |b| A.  THE RECURRENCE TERM: mu = n . u is three products and two sums on a unit-length pair,
|delta mu| <= 4 * 2^-53 = 2^-51, and |P_l'| <= l (l + 1) / 2 on [-1, 1], so the rounding of mu moves P_l by at most l (l + 1) 2^-52; a
step of the recurrence commits three roundings (a fused multiply-add, where the compiler forms one, fewer) of relative 2^-53 on
terms of magnitude <= 2, and an error committed at step k reaches order l multiplied by at most (l - k + 1) (the error obeys the
same recurrence; its response to a unit error at step k is largest at mu = +-1, where it grows as (k + 1) (H_l - H_k) with H the
harmonic numbers; over 20 001 values of mu and every k < l <= 64 it stays below 0.993 (l - k + 1)), so the steps add at most
sum_k 6 (l - k + 1) 2^-53 <= 3 l^2 2^-53.  Together below 4 l^2 2^-52 <= n_orders^2 2^-50; the bound takes twice that.

THE TAIL.  ln_env (N, n_knots) (source n's omni law), M, F, w_e, w_l, the draws g(s) of shoebox_tail_cases (zero outside [0, ir_len)),
psi_d the diffuse-field filter; y as above with y_end = min(ir_len, M + F);
    n(t) = ((1 - p) e_k + p e_{k+1}) sum_j psi_d[j] g(t - j),  e_k = exp(ln_env[n][k]),  k = t // 256,  p = (t % 256) / 256,
    h = float32(w_e y(t) + w_l n(t)), no noise term where w_l == 0.
ITS BOUND: shoebox_bands_cases' with B = 1: the image part above under w_e; w_l e(t) sum_j |psi_d[j]| tol(t - j) for the draws'
tolerance; w_l (2 half + 1 + 1 + 16) 2^-53 e(t) sum_j |psi_d[j]| |g(t - j)| for the accumulation, in either order of the products;
2^-24 |h64| + 2^-150 for the one rounding.
"""
import ctypes as ct
import functools
import json

import numpy as np
import pytest
from scipy import special

from audiblelight_amd import _hip, core, engine, shoebox
from tests import noise_draw_cases as nd
from tests import shoebox_bands_cases as bc
from tests import shoebox_cases as sc
from tests import shoebox_directional_cases as dc
from tests import shoebox_source_cases as srcc
from tests import shoebox_tail_cases as tc

bits = sc.bits
FS = 16000.0
SEED = 0x5B4E7E5F00D12345
HEAD, ARRAY = 0.0875, 0.042
CENTRE = np.array([1.31, 1.42, 1.2])                     # shoebox_cases' first capsule: at least 0.9 m from SOURCES_5[:3]
SOURCES_3 = sc.SOURCES_5[:3]
# five capsule directions: the two on the x axis, one on -z, two oblique
DIRECTIONS_5 = np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, -1.0], list(dc.OBLIQUE), [-0.6, 0.64, 0.48]])
WORST = {"fraction": 0.0}


# ----------------------------------------------------------------------------- the restatement: the definition, in float64
def legendre(n_orders, mu):
    """P_l(mu), l < n_orders, by the definition's recurrence: (n_orders, ...)."""
    mu = np.asarray(mu, dtype=np.float64)
    P = np.zeros((n_orders,) + mu.shape)
    P[0] = 1.0
    if n_orders > 1:
        P[1] = mu
    for l in range(1, n_orders - 1):
        P[l + 1] = ((2 * l + 1) * mu * P[l] - l * P[l - 1]) / (l + 1)
    return P


def order_rows(room, betas, air, s, centre, direction, spat, n_orders, lo, hi, fs, c=sc.C_SOUND, max_order=None):
    """(y_l (n_orders, hi - lo), A (hi - lo)) of one source at one capsule, index i at sample lo + i."""
    R, d, tau, sign, k = srcc.images(room, s, centre, hi, fs, c, max_order)
    u = R / d[:, None]
    mu = np.clip(direction[0] * u[:, 0] + direction[1] * u[:, 1] + direction[2] * u[:, 2], -1.0, 1.0)
    P = legendre(n_orders, mu)
    gs = srcc.source_gain(spat, sign, u)
    ws = 1.0 if spat is None else srcc._norm(spat)
    with np.errstate(divide="ignore"):
        gain = np.prod(np.asarray(betas, dtype=np.float64)[None, :] ** k, axis=1)             # numpy: 0.0 ** 0 == 1.0
    a = gain / (4.0 * np.pi * d) * np.exp(-air * d)
    t = np.ceil(tau - sc.HALF)[:, None] + np.arange(sc.TAPS + 1)[None, :]
    x = t - tau[:, None]
    live = (np.abs(x) < sc.HALF) & (t >= lo) & (t < hi) & (gain > 0.0)[:, None]
    shape = 0.5 * (1.0 + np.cos(2.0 * np.pi * x / sc.TAPS)) * np.sinc(x)
    idx = (t[live] - lo).astype(np.int64)
    y = np.stack([np.bincount(idx, weights=((a * gs * P[l])[:, None] * shape)[live], minlength=hi - lo) for l in range(n_orders)])
    A = np.bincount(idx, weights=np.broadcast_to((np.abs(a) * ws)[:, None], t.shape)[live], minlength=hi - lo)
    return y, A


def image_part(room, betas, air, s, centre, direction, spat, table, y_end, fs, c=sc.C_SOUND, max_order=None):
    """(sum_l b_l * y_l, sum_l |b_l| * A) at t in [0, y_end) of one pair."""
    n_orders, half = table.shape[0], (table.shape[1] - 1) // 2
    y, A = order_rows(room, betas, air, s, centre, direction, spat, n_orders, -half, y_end + half, fs, c, max_order)
    img = sum(np.convolve(y[l], table[l])[2 * half: 2 * half + y_end] for l in range(n_orders))
    spread = np.convolve(A, np.abs(table).sum(axis=0))[2 * half: 2 * half + y_end]
    return img, (2.0 ** -30 + n_orders ** 2 * 2.0 ** -49) * spread


_RESTATED = {}


def restate(room, betas, air, sources, spats, centre, directions, table, ir_len, fs, c=sc.C_SOUND, max_order=None):
    """(h64, bound) of shape (C, N, ir_len) of the entry without a tail: computed once per scenario and shared (read-only)."""
    sources, directions = np.atleast_2d(sources), np.atleast_2d(directions)
    key = (tuple(room), tuple(betas), float(air), sources.tobytes(), None if spats is None else np.asarray(spats).tobytes(),
           np.asarray(centre).tobytes(), directions.tobytes(), table.tobytes(), table.shape, ir_len, fs, c, max_order)
    if key not in _RESTATED:
        h, bound = np.zeros((len(directions), len(sources), ir_len)), np.zeros((len(directions), len(sources), ir_len))
        for ci in range(len(directions)):
            for ni in range(len(sources)):
                h[ci, ni], bound[ci, ni] = image_part(room, betas, air, sources[ni], centre, directions[ci],
                                                      None if spats is None else spats[ni], table, ir_len, fs, c, max_order)
        bound += 2.0 ** -24 * np.abs(h)
        h.flags.writeable = bound.flags.writeable = False
        _RESTATED[key] = (h, bound)
    return _RESTATED[key]


def restate_tail(room, betas, air, sources, spats, centre, directions, table, psi, ir_len, fs, M, F, ln_env, seed, sid0, cid0, c=sc.C_SOUND,
                 max_order=None):
    """(h64, bound) of shape (C, N, ir_len) of the entry with a tail; ln_env (N, n_knots)."""
    sources, directions, ln_env = np.atleast_2d(sources), np.atleast_2d(directions), np.asarray(ln_env, dtype=np.float64)
    half, n_taps = (len(psi) - 1) // 2, len(psi)
    y_end = min(ir_len, M + F)
    w_e, w_l = tc.weights(ir_len, M, F)
    t = np.arange(ir_len)
    k, p = t // 256, (t % 256) / 256.0
    fir = lambda x, taps: np.convolve(x, taps)[half: half + ir_len]                                       # noqa: E731
    h, bound = np.zeros((len(directions), len(sources), ir_len)), np.zeros((len(directions), len(sources), ir_len))
    for ni in range(len(sources)):
        with np.errstate(over="ignore"):
            knots = np.exp(ln_env[ni])
        e = np.where(p == 0.0, knots[k], (1.0 - p) * knots[k] + p * knots[np.minimum(k + 1, len(knots) - 1)])
        for ci in range(len(directions)):
            img, img_bound = np.zeros(ir_len), np.zeros(ir_len)
            img[:y_end], img_bound[:y_end] = image_part(room, betas, air, sources[ni], centre, directions[ci],
                                                        None if spats is None else spats[ni], table, y_end, fs, c, max_order)
            g = tc.restated_g(seed, sid0 + ni, cid0 + ci, ir_len)
            noise = e * fir(g, psi)
            draw = e * fir(nd.RTOL * np.abs(g) + nd.ATOL, np.abs(psi))
            accum = (n_taps + 1 + 16) * 2.0 ** -53 * e * fir(np.abs(g), np.abs(psi))
            h[ci, ni] = w_e * img + np.where(w_l > 0.0, w_l * noise, 0.0)
            bound[ci, ni] = w_e * img_bound + np.where(w_l > 0.0, w_l * (draw + accum), 0.0) + 2.0 ** -24 * np.abs(h[ci, ni]) + 2.0 ** -150
    return h, bound


def assert_within(rows, h64, bound, what):
    rows = np.asarray(rows, dtype=np.float64)
    assert np.all(np.isfinite(rows)), what
    err = np.abs(rows - h64)
    frac = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)))
    WORST["fraction"] = max(WORST["fraction"], frac)
    print(f"shoebox sphere bound [{what}]: max err {err.max():.3e}, max err / bound {frac:.3f} (so far {WORST['fraction']:.3f})")
    assert np.all(err <= bound), (what, "err / bound", frac, "at", np.unravel_index(np.argmax(err - bound), err.shape))


# ----------------------------------------------------------------------------- tables
def random_table(n_orders, half, seed=0):
    """A seeded table the entry has to take as any other: every order of comparable weight, sum_j |b_l[j]| about 1."""
    return np.random.default_rng(1000 * n_orders + half + seed).uniform(-1.0, 1.0, (n_orders, 2 * half + 1)) / (half + 1.0)


def delta_table(weights, half):
    table = np.zeros((len(weights), 2 * half + 1))
    table[:, half] = weights
    return table


@functools.lru_cache(maxsize=None)
def physical(radius, fs, n_orders=None, half=None):
    table, psi = shoebox.sphere_filters(radius, fs, sc.C_SOUND, n_orders, half), shoebox.sphere_diffuse_filter(radius, fs, sc.C_SOUND, n_orders, half)
    table.flags.writeable = psi.flags.writeable = False
    return table, psi


# ----------------------------------------------------------------------------- running the entry point
def per_pair_bytes(r, n_orders, half, ir_len, mix=-1, fade=0):
    return r.lib.call("al_ism_shoebox_sphere_workspace_bytes", int(n_orders), int(half), int(ir_len), int(mix), int(fade))


def run_sphere(r, room, betas, sources, spats, centre, directions, air, table, ir_len, fs, c=sc.C_SOUND, max_order=None, pitch=None,
               pairs_per_pass=None, tail=None):
    """al_ism_shoebox_sphere into a buffer with sc.GUARD sentinels on either side and a workspace of exactly pairs_per_pass pairs
    (None: all) with a guard behind it: the (C, N, pitch) rows, the guards checked.  tail: None (mix = -1) or a dictionary M, F, psi,
    ln_env (N, n_knots) and optionally seed, sid0, cid0."""
    mem, lib = r.mem, r.lib
    sources = np.ascontiguousarray(np.atleast_2d(sources), dtype=np.float64)
    directions = np.ascontiguousarray(np.atleast_2d(directions), dtype=np.float64)
    table = np.ascontiguousarray(table, dtype=np.float64)
    n, n_cap, n_orders, half = len(sources), len(directions), table.shape[0], (table.shape[1] - 1) // 2
    pitch = shoebox.pitch_of(ir_len) if pitch is None else pitch
    total = n_cap * n * pitch
    t = dict(M=-1, F=0, seed=SEED, sid0=0, cid0=0, ln_env=None, psi=None)
    t.update(tail or {})
    if t["ln_env"] is not None:
        assert np.shape(t["ln_env"]) == (n, shoebox.n_knots_of(ir_len)) and np.shape(t["psi"]) == (2 * half + 1,)
    per_pair = per_pair_bytes(r, n_orders, half, ir_len, t["M"], t["F"])
    y_end = ir_len if t["M"] < 0 else min(ir_len, t["M"] + t["F"])
    assert per_pair == n_orders * ((y_end + 2 * half + 255) // 256 * 256) * 8
    ws_bytes = per_pair * (n * n_cap if pairs_per_pass is None else pairs_per_pass)
    ws = mem.upload(np.full(ws_bytes // 8 + sc.GUARD, 7.5, dtype=np.float64))
    out = srcc._guarded(mem, total)
    dev = [srcc._dev(mem, v) for v in (sources, spats, directions, table, t["psi"], t["ln_env"])]
    centre = np.ascontiguousarray(centre, dtype=np.float64)
    lib.call("al_ism_shoebox_sphere", mem.ptr(dev[0]), n, srcc._ptr(mem, dev[1]), centre.ctypes.data_as(ct.POINTER(ct.c_double)), mem.ptr(dev[2]),
             n_cap, (ct.c_double * 3)(*room), (ct.c_double * 6)(*betas), float(air), mem.ptr(dev[3]), n_orders, half, srcc._ptr(mem, dev[4]),
             float(c), float(fs), -1 if max_order is None else int(max_order), int(ir_len), int(pitch), int(t["M"]), int(t["F"]),
             int(t["seed"]), int(t["sid0"]), int(t["cid0"]), srcc._ptr(mem, dev[5]), 0 if t["ln_env"] is None else np.shape(t["ln_env"])[1],
             mem.ptr(ws), ws_bytes, mem.ptr(out) + 4 * sc.GUARD, mem.stream())
    assert np.all(np.asarray(mem.download(ws))[ws_bytes // 8:] == 7.5), "the workspace's guard was overwritten"
    return srcc._unguard(mem, out, total, (n_cap, n, pitch))


def check_parity(r, room, betas, sources, spats, centre, directions, air, table, ir_len, fs, max_order=None, what=None, **kw):
    rows = run_sphere(r, room, betas, sources, spats, centre, directions, air, table, ir_len, fs, max_order=max_order, **kw)
    assert np.all(bits(rows[:, :, ir_len:]) == 0), "pad samples must be +0"
    h64, bound = restate(room, betas, air, sources, spats, centre, directions, table, ir_len, fs, max_order=max_order)
    assert_within(rows[:, :, :ir_len], h64, bound, what)
    return rows[:, :, :ir_len], h64


# ----------------------------------------------------------------------------- 1. the filters (CPU only)
# (radius, fs, half): the worst |DTFT of the table - exact series| over 41 mu x 400 frequencies, as measured
FILTER_CASES = {(0.042, 48000.0, 64): 2.72e-3, (0.042, 44100.0, 64): 2.76e-3, (0.0875, 16000.0, 64): 2.70e-3, (0.0875, 48000.0, 96): 4.32e-3}
FILTER_MARGIN = 1.5      # of the measured deviation: the computation is deterministic, the margin is for the evaluation grid


def exact_series(radius, fs, f, mu, c=sc.C_SOUND):
    """The rigid-sphere series from scipy's spherical Bessel functions, 20 orders past Wiscombe's length at the Nyquist frequency,
    times the filters' taper: complex (len(mu), len(f))."""
    x = 2.0 * np.pi * f * radius / c
    f_p = 0.8 * 0.5 * fs
    T = np.where(f <= f_p, 1.0, np.where(f < 1.25 * f_p, np.cos(0.5 * np.pi * (f - f_p) / (0.25 * f_p)) ** 2, 0.0))
    n = shoebox.wiscombe_length(float(x.max())) + 20
    P = legendre(n, mu)
    out = np.zeros((len(mu), len(f)), dtype=np.complex128)
    for l in range(n):
        dh = special.spherical_jn(l, x, derivative=True) + 1j * special.spherical_yn(l, x, derivative=True)
        out += P[l][:, None] * (np.conj((2 * l + 1) * 1j * (-1j) ** l / (x * x * dh)) * T)[None, :]
    return out


def run_filters():
    mu = np.linspace(-1.0, 1.0, 41)
    for (radius, fs, half), measured in FILTER_CASES.items():
        table, psi = physical(radius, fs, None, half)
        n_orders = table.shape[0]
        assert table.shape == (n_orders, 2 * half + 1) and table.dtype == np.float64 and table.flags.c_contiguous
        assert n_orders == shoebox.wiscombe_length(2.0 * np.pi * 0.8 * 0.5 * fs * radius / sc.C_SOUND) <= 64
        f = np.linspace(20.0, 0.5 * fs, 400)
        j = np.arange(-half, half + 1)
        response = legendre(n_orders, mu).T @ (table @ np.exp(-2j * np.pi * np.outer(j, f) / fs))
        worst = float(np.abs(response - exact_series(radius, fs, f, mu)).max())
        margin = FILTER_MARGIN * measured
        print(f"sphere filters a={radius} fs={fs:.0f} half={half}: {n_orders} orders, worst deviation from the exact series {worst:.3e}")
        assert worst <= margin, (radius, fs, half, worst)
        assert np.abs(legendre(n_orders, mu).T @ table.sum(axis=1) - 1.0).max() <= margin              # the DC gain, at every angle
        front = legendre(n_orders, np.array(1.0)) @ table
        assert abs(int(j[np.argmax(np.abs(front))]) - int(np.rint(-radius * fs / sc.C_SOUND))) <= 1    # the facing point leads the centre
        assert psi.shape == (2 * half + 1,) and np.array_equal(psi, psi[::-1]) and abs(psi.sum() - 1.0) <= margin
    # the defaults
    assert shoebox.sphere_filters(ARRAY, 48000.0).shape == (28, 129) and shoebox.sphere_filters(HEAD, 48000.0).shape == (47, 2 * 98 + 1)
    assert shoebox.sphere_diffuse_filter(HEAD, 48000.0).shape == (2 * 98 + 1,)
    # fewer orders than Wiscombe's length: the pass edge comes down, the table stays a low-pass of the same sphere
    few = shoebox.sphere_filters(ARRAY, 48000.0, n_orders=12)
    assert few.shape == (12, 129) and np.abs(legendre(12, mu).T @ few.sum(axis=1) - 1.0).max() <= 0.01
    f = np.array([1000.0, 20000.0])
    resp = np.abs(legendre(12, mu[-1:]).T @ (few @ np.exp(-2j * np.pi * np.outer(np.arange(-64, 65), f) / 48000.0)))[0]
    assert resp[0] > 1.0 and resp[1] < 0.02
    assert np.array_equal(shoebox.sphere_filters(ARRAY, 48000.0, n_orders=40)[:28], shoebox.sphere_filters(ARRAY, 48000.0))     # more: f_p stays
    # a head at 96 kHz needs more than 64 orders: the series is cut at 64 and the pass edge lowered
    assert shoebox.sphere_filters(HEAD, 96000.0).shape[0] == 64
    # the Hankel recurrence against scipy, up to order 54
    x = np.geomspace(0.05, 60.0, 200)
    ref = np.array([special.spherical_jn(l, x) + 1j * special.spherical_yn(l, x) for l in range(55)])
    assert np.abs(shoebox.spherical_hankel1(54, x) / ref - 1.0).max() <= 1e-12
    bad = [dict(radius=0.0), dict(radius=-0.1), dict(radius=np.nan), dict(sample_rate=0.0), dict(c=np.inf), dict(n_orders=3), dict(n_orders=65),
           dict(n_orders=8.5), dict(n_orders=True), dict(half=0), dict(half=1025), dict(half=2.5)]
    for change in bad:
        for make in (shoebox.sphere_filters, shoebox.sphere_diffuse_filter):
            with pytest.raises(ValueError):
                make(**dict(dict(radius=ARRAY, sample_rate=16000.0), **change))


# ----------------------------------------------------------------------------- 2. parity with the restatement
def _cfg(room="oblong", order=None, n_orders=5, half=16, pairs="1x1", ir_len=None, table="random"):
    return (room, order, n_orders, half, pairs, ir_len, table)


PARITY = (
    [_cfg(room, order, pairs="3x5") for room in sc.ROOMS for order in (0, 1, 3, None)]
    + [_cfg(n_orders=n, order=order, ir_len=400) for n in (1, 2, 4, 9) for order in (1, None)]     # 5 and 9: groups of four and a group of one
    + [_cfg(n_orders=64, order=1, ir_len=300), _cfg(n_orders=64, order=None, ir_len=257, half=1)]
    + [_cfg(n_orders=2, half=half, order=3, ir_len=400) for half in (1, 16, 64)]
    + [_cfg("cubic", 3, pairs="3x5", ir_len=600, table="physical")]                               # the head at 8 kHz: 16 orders, half 64
)


def run_parity(r, room, order, n_orders, half, pairs, ir_len, table):
    src, dirs = (SOURCES_3, DIRECTIONS_5) if pairs == "3x5" else (SOURCES_3[1:2], DIRECTIONS_5[3:4])
    fs = FS
    if table == "physical":
        fs = 8000.0
        b, _ = physical(HEAD, fs)
        assert b.shape == (16, 129)
    else:
        b = random_table(n_orders, half)
    ir_len = (700 if order is None else 1000) if ir_len is None else ir_len
    rows, _ = check_parity(r, sc.ROOMS[room], sc.UNEQUAL_BETAS, src, None, CENTRE, dirs, 0.0, b, ir_len, fs, max_order=order,
                           what=f"{room} order={order} orders={b.shape[0]} half={(b.shape[1] - 1) // 2} {pairs} {table}")
    assert np.all(np.abs(rows).max(axis=2) > 0), "a row is silent"


EDGE_LEN = (1, 81, 256, 257, 1000)


def run_edge_length(r, ir_len):
    """shoebox_cases.run_edge_length's room: row lengths around the tap count and the tile, the order sums reaching `half` past
    either end of the row."""
    room, betas = (2.4, 2.0, 1.7), (0.8, 0.7, 0.9, 0.6, 0.5, 0.95)
    src = np.array([[0.5, 0.6, 0.7], [2.0, 1.5, 1.1]])
    rows, _ = check_parity(r, room, betas, src, None, (1.5, 1.2, 0.9), DIRECTIONS_5[2:5], 0.0, random_table(3, 16), ir_len, FS,
                           what=f"edge ir_len={ir_len}")
    assert np.abs(rows).max() > 0


def run_on_axis(r):
    """A source on the sphere's x axis at exactly 2 radius from the centre, capsules pointing exactly at it and exactly away: the
    direct path has mu = +1 and -1 (P_l = 1 and (-1)^l: any drift of the recurrence or a clamp on the wrong side shows at the
    high orders), and it arrives 11.7 samples into the row, so its taps and the order sums below sample 0 are in use.  The radius
    is 0.125 m, a binary fraction as the centre's coordinates are, so that the distance is 2 radius to the bit."""
    room, radius = sc.ROOMS["oblong"], 0.125
    centre = np.array([2.0, 1.5, 1.25])
    s = centre + np.array([2.0 * radius, 0.0, 0.0])
    shoebox.check_sphere(room, centre, radius, s[None])                      # 2 radius is allowed; any closer is not
    with pytest.raises(ValueError):
        shoebox.check_sphere(room, centre, radius, (centre + np.array([1.99 * radius, 0.0, 0.0]))[None])
    b, _ = physical(radius, FS)
    assert b.shape == (28, 129)
    for order in (0, None):
        rows, h64 = check_parity(r, room, sc.UNEQUAL_BETAS, s, None, centre, DIRECTIONS_5[:2], 0.0, b, 400, FS, max_order=order,
                                 what=f"on axis at 2 radius, order={order}")
    y, _ = order_rows(room, sc.UNEQUAL_BETAS, 0.0, s, centre, DIRECTIONS_5[1], None, b.shape[0], 0, 100, FS, max_order=0)
    y0 = y[0][np.abs(y[0]) > 0]
    assert np.array_equal(y[21][np.abs(y[0]) > 0], -y0) and np.array_equal(y[20][np.abs(y[0]) > 0], y0)      # mu = -1 exactly
    # the facing capsule is louder and earlier than the one at the back pole (the table's peaks: 1.62 at -6 samples against 0.74 at
    # +9, the bright spot of the waves that creep round both sides: a fs / c = 5.8 and (pi / 2) a fs / c = 9.2)
    peak = np.argmax(np.abs(h64[:, 0, :60]), axis=1)
    assert np.abs(h64[0, 0, :60]).max() > 1.5 * np.abs(h64[1, 0, :60]).max() and 10 <= peak[1] - peak[0] <= 20


def run_source_and_air(r):
    """Patterned sources and air through the sphere entry: the source side of shoebox_source_cases in the common amplitude."""
    b = random_table(5, 16)
    for order in (1, None):
        rows, _ = check_parity(r, sc.ROOMS["oblong"], sc.UNEQUAL_BETAS, SOURCES_3, srcc.SPATS_5[2:5], CENTRE, DIRECTIONS_5, srcc.AIR, b,
                               700, FS, max_order=order, what=f"source patterns and air, order={order}")
        assert np.all(np.abs(rows).max(axis=2) > 0)


# ----------------------------------------------------------------------------- 3. ties that do not use the restatement
def run_omni_tie(r):
    """One order with a delta table: P_0 = 1, so the rows are al_ism_shoebox's at the centre."""
    room, ir_len, order = sc.ROOMS["cubic"], 520, None
    for half in (1, 16):
        rows = run_sphere(r, room, sc.UNEQUAL_BETAS, SOURCES_3, None, CENTRE, DIRECTIONS_5[:2], 0.0, delta_table([1.0], half), ir_len, FS,
                          max_order=order)
        want = sc.run_abi(r, room, sc.UNEQUAL_BETAS, SOURCES_3, CENTRE, ir_len, FS, max_order=order)
        y64, A, _ = sc.oracle(room, sc.UNEQUAL_BETAS, SOURCES_3, CENTRE, ir_len, FS, max_order=order)
        err = np.abs(rows[:, :, :ir_len].astype(np.float64) - want[:, :, :ir_len].astype(np.float64))
        # both bounds; the sphere's restated with A of the omni oracle (an oracle this module's restatement has no part in)
        assert np.all(err <= 2.0 * (2.0 ** -24 * np.abs(y64) + 2.0 ** -30 * A) + 2.0 ** -49 * A), float(err.max())
        # and bit for bit: gain[0] = 1.0, the images in the same canonical order, a delta table that adds +-0 and multiplies by 1
        assert np.array_equal(bits(rows), bits(np.broadcast_to(want, rows.shape))), f"half={half}: not the bits of al_ism_shoebox"
        assert np.abs(want).max() > 0


def run_first_order_tie(r):
    """Two orders with the table (w delta, v delta): the rows of al_ism_shoebox_dir at the centre with the patterns (w, v n_c).  That
    kernel's sign of u and direction convention are pinned by its own suite."""
    room, ir_len, order = sc.ROOMS["oblong"], 520, 3
    w, v = 0.3, 0.7
    dirs = DIRECTIONS_5[1:5]
    rows = run_sphere(r, room, sc.UNEQUAL_BETAS, SOURCES_3, None, CENTRE, dirs, 0.0, delta_table([w, v], 16), ir_len, FS, max_order=order)
    patterns = np.concatenate([np.full((4, 1), w), v * dirs], axis=1)[None]                 # (1, 4, 4): one position, four channels
    want = dc.run_abi(r, room, sc.UNEQUAL_BETAS, SOURCES_3, CENTRE, patterns, ir_len, FS, max_order=order)
    y64, A, _ = sc.oracle(room, sc.UNEQUAL_BETAS, SOURCES_3, CENTRE, ir_len, FS, max_order=order)
    err = np.abs(rows[:, :, :ir_len].astype(np.float64) - want[:, :, :ir_len].astype(np.float64))
    allowed = 2.0 ** -24 * (np.abs(rows[:, :, :ir_len]) + np.abs(want[:, :, :ir_len])) + (2.0 * 2.0 ** -30 + 4 * 2.0 ** -49) * (w + v) * A
    print(f"first-order tie: max err / allowed {float(np.max(err / np.where(allowed > 0, allowed, 1.0))):.3f}")
    assert np.all(err <= allowed)
    flipped = run_sphere(r, room, sc.UNEQUAL_BETAS, SOURCES_3, None, CENTRE, -dirs, 0.0, delta_table([w, v], 16), ir_len, FS, max_order=order)
    assert np.abs(flipped[:, :, :ir_len] - want[:, :, :ir_len]).max() > 1e4 * allowed.max()      # a wrong sign would not pass


def run_null_arguments(r):
    """Omni source rows and air = 0: the bits of NULL and 0 (the kernels without the source side)."""
    room, ir_len, b = sc.ROOMS["oblong"], 520, random_table(5, 16)
    plain = run_sphere(r, room, sc.UNEQUAL_BETAS, SOURCES_3, None, CENTRE, DIRECTIONS_5, 0.0, b, ir_len, FS, max_order=3)
    omni = run_sphere(r, room, sc.UNEQUAL_BETAS, SOURCES_3, srcc.OMNI_5[:3], CENTRE, DIRECTIONS_5, 0.0, b, ir_len, FS, max_order=3)
    assert np.array_equal(bits(omni), bits(plain)) and np.abs(plain).max() > 0


def tail_tables(n, ir_len):
    """A distinct decaying knot table per source: a wrong stride reads a level that is off by at least 0.25 Np."""
    return -3.0 - 0.25 * np.arange(n)[:, None] - 0.4 * np.arange(shoebox.n_knots_of(ir_len))[None, :]


def run_no_tail(r):
    """M >= ir_len: the bits of mix < 0."""
    room, ir_len = tc.ROOM, 520
    b, psi = physical(HEAD, FS)
    for pitch in (None, 768 + 8):
        want = run_sphere(r, room, tc.BETAS, SOURCES_3, None, CENTRE, DIRECTIONS_5[:2], 0.0, b, ir_len, FS, max_order=2, pitch=pitch)
        for M, F in ((ir_len, 1), (ir_len + 1000, 7), (1 << 40, 1), (ir_len, 1 << 62)):
            got = run_sphere(r, room, tc.BETAS, SOURCES_3, None, CENTRE, DIRECTIONS_5[:2], 0.0, b, ir_len, FS, max_order=2, pitch=pitch,
                             tail=dict(M=M, F=F, psi=psi, ln_env=tail_tables(3, ir_len)))
            assert np.array_equal(bits(got), bits(want)), ("the entry with mix >= ir_len differs from mix < 0", M, F, pitch)


def run_past_the_split(r):
    """The samples at and past the split carry the bits of al_ism_shoebox_bands_src's tail with ONE band handed psi_d, the same
    knots, seed and ids (k_ism_band_tail, whatever the capsule is)."""
    room, ir_len, M, F, sid0, cid0 = tc.ROOM, 256 + 1024 + 10, 100, 60, 7, 0xFFFFFFF0
    b, psi = physical(HEAD, FS)
    half = (len(psi) - 1) // 2
    ln_env = tail_tables(3, ir_len)
    got = run_sphere(r, room, tc.BETAS, SOURCES_3, None, CENTRE, DIRECTIONS_5[:2], 0.0, b, ir_len, FS, max_order=1,
                     tail=dict(M=M, F=F, psi=psi, ln_env=ln_env, sid0=sid0, cid0=cid0))
    mem, lib = r.mem, r.lib
    n, n_cap, pitch = 3, 2, shoebox.pitch_of(ir_len)
    per_pair = bc.per_pair_bytes(r, 1, half, ir_len, M, F)
    ws, out = mem.upload(np.full(per_pair * n * n_cap // 8, 7.5)), srcc._guarded(mem, n_cap * n * pitch)
    dev = [srcc._dev(mem, v) for v in (SOURCES_3, np.tile(CENTRE, (n_cap, 1)) + [[0.0, 0.0, 0.0], [0.3, 0.1, 0.2]], psi, ln_env)]
    lib.call("al_ism_shoebox_bands_src", mem.ptr(dev[0]), n, None, mem.ptr(dev[1]), n_cap, (ct.c_double * 3)(*room), (ct.c_double * 6)(*tc.BETAS),
             1, mem.ptr(dev[2]), half, (ct.c_double * 1)(0.0), sc.C_SOUND, FS, 1, ir_len, pitch, M, F, SEED, sid0, cid0, mem.ptr(dev[3]),
             ln_env.shape[1], mem.ptr(ws), per_pair * n * n_cap, mem.ptr(out) + 4 * sc.GUARD, mem.stream())
    want = srcc._unguard(mem, out, n_cap * n * pitch, (n_cap, n, pitch))
    split = (M + F + 255) // 256 * 256
    assert split == 256 and np.array_equal(bits(got[:, :, split:]), bits(want[:, :, split:]))
    assert np.all(got[:, :, split:ir_len] != 0.0) and not np.array_equal(bits(got[:, :, :split]), bits(want[:, :, :split]))


#               M    F    ir_len table       pairs  order pitch sid0        cid0        per_pass
TAIL_PARITY = [(M, F, 1000, "physical", "1x1", None, None, 0, 0, None) for M in (0, 300, 1000, 5000) for F in (1, 100)] + [
    (300, 100, 900, "random5", "3x5", 1, 1200, 7, 0xFFFFFFF0, 4), (100, 50, 256 + 1024 + 5, "physical", "1x1", 1, None, 0xFFFFFFF0, 9, None),
    (255, 1, 600, "random9", "3x5", 3, None, 1, 2, 1)]


def run_tail_parity(r, M, F, ir_len, table, pairs, order, pitch, sid0, cid0, per_pass):
    src, dirs = (SOURCES_3, DIRECTIONS_5) if pairs == "3x5" else (SOURCES_3[1:2], DIRECTIONS_5[3:4])
    if table == "physical":
        b, psi = physical(HEAD, FS)
    else:
        b = random_table(int(table[6:]), 16)
        psi = random_table(1, 16, seed=7)[0]
    spats, air = (srcc.SPATS_5[2:2 + len(src)], srcc.AIR) if pairs == "3x5" else (None, 0.0)
    ln_env = tail_tables(len(src), ir_len)
    rows = run_sphere(r, tc.ROOM, tc.BETAS, src, spats, CENTRE, dirs, air, b, ir_len, FS, max_order=order, pitch=pitch, pairs_per_pass=per_pass,
                      tail=dict(M=M, F=F, psi=psi, ln_env=ln_env, sid0=sid0, cid0=cid0))
    assert np.all(bits(rows[:, :, ir_len:]) == 0), "pad samples must be +0"
    h64, bound = restate_tail(tc.ROOM, tc.BETAS, air, src, spats, CENTRE, dirs, b, psi, ir_len, FS, M, F, ln_env, SEED, sid0, cid0, max_order=order)
    assert_within(rows[:, :, :ir_len], h64, bound, f"tail M={M} F={F} ir_len={ir_len} {table} {pairs} order={order}")
    if ir_len > M + F:
        assert np.all(rows[:, :, M + F: ir_len] != 0.0), "a tail sample is zero"


# ----------------------------------------------------------------------------- 4. identity
def run_identity(r):
    """A row alone, among many, at another pitch, with a workspace of one pair per pass and in two runs is bit-identical, without a
    tail and with one."""
    room, ir_len, M, F, sid0, cid0 = tc.ROOM, 700, 100, 50, 7, 3
    b, psi = physical(HEAD, FS)
    ln_env = tail_tables(3, ir_len)
    for tailed in (False, True):
        def run(ns=slice(0, 3), cs=slice(0, 5), **kw):
            ids = {k: kw.pop(k) for k in ("sid0", "cid0", "seed") if k in kw}
            tail = dict(dict(M=M, F=F, psi=psi, ln_env=ln_env[ns], sid0=sid0, cid0=cid0), **ids) if tailed else None
            return run_sphere(r, room, tc.BETAS, SOURCES_3[ns], srcc.SPATS_5[2:5][ns], CENTRE, DIRECTIONS_5[cs], srcc.AIR, b, ir_len, FS,
                              max_order=2, tail=tail, **kw)

        one = run()
        assert np.array_equal(bits(one), bits(run())), "two runs differ"
        for per_pass in (1, 4):
            assert np.array_equal(bits(run(pairs_per_pass=per_pass)), bits(one)), ("the bits depend on the workspace size", per_pass)
        wide = run(pitch=1024 + 256 + 4, pairs_per_pass=2)
        assert np.array_equal(bits(wide[:, :, :ir_len]), bits(one[:, :, :ir_len])) and np.all(bits(wide[:, :, ir_len:]) == 0)
        for ci, ni in ((0, 0), (3, 1), (4, 2)):
            alone = run(slice(ni, ni + 1), slice(ci, ci + 1), sid0=sid0 + ni, cid0=cid0 + ci)
            assert np.array_equal(bits(alone[0, 0]), bits(one[ci, ni])), (tailed, ci, ni)
        if tailed:
            other = run(slice(0, 1), slice(0, 1), seed=SEED + 1)
            assert np.array_equal(bits(other[0, 0, :M + 1 - 64]), bits(one[0, 0, :M + 1 - 64])) and np.all(other[0, 0, M + 1: ir_len] != one[0, 0, M + 1: ir_len])


# ----------------------------------------------------------------------------- 5. physics, the state and the scene
BIN_ROOM = (4.1, 3.3, 2.6)
BIN_HEAD = np.array([2.0, 1.4, 1.3])
BIN_TALKER = np.array([2.0, 2.6, 1.3])      # 1.2 m to the left (+y) of a listener who faces +x


def direct_path_lag(fs, radius=HEAD):
    """The lag in samples of the right ear's energy centroid behind the left's for a plane wave from the left (mu = cos 10 degrees
    and cos 170 degrees), from the restatement's tables alone; and the geometric a fs / c (cos 10 + 80 pi / 180)."""
    table, _ = physical(radius, fs)
    half = (table.shape[1] - 1) // 2
    ears = shoebox.binaural_directions()
    mu = ears @ np.array([0.0, 1.0, 0.0])
    assert np.allclose(mu, [np.cos(np.deg2rad(10.0)), np.cos(np.deg2rad(170.0))])
    h = legendre(table.shape[0], mu).T @ table                                # (2, taps): the ears' responses to the wave
    j = np.arange(-half, half + 1)
    centroid = (h * h) @ j / (h * h).sum(axis=1)
    return float(centroid[1] - centroid[0]), radius * fs / sc.C_SOUND * (np.cos(np.deg2rad(10.0)) + np.deg2rad(80.0)), (h * h).sum(axis=1)


def run_binaural_physics_restated():
    """ITD and ILD of the filters themselves, before any kernel: the band of the scene test follows these numbers."""
    for fs in (16000.0, 48000.0):
        lag, geometric, energy = direct_path_lag(fs)
        print(f"binaural direct path at fs={fs:.0f}: lag {lag:.3f} samples = {lag / geometric:.3f} of the geometric {geometric:.3f}; "
              f"left / right energy {energy[0] / energy[1]:.2f}")
        assert 1.0 <= lag / geometric <= 1.15 and energy[0] > energy[1]


def binaural_state(r, tail=None, ir_len=800, max_order=None):
    st = core.ShoeboxIRState(BIN_ROOM, betas=tc.BETAS, ir_len=ir_len, sample_rate=int(FS), max_order=max_order, renderer=r, tail=tail)
    st.add_binaural_listener("head", BIN_HEAD)
    st.add_emitters([BIN_TALKER], alias="talker")
    return st


def run_binaural_scene(r, monkeypatch, tmp_path):
    """A listener facing +x with a talker 1.2 m to the left, through Scene.generate(): the signs and the size of the interaural
    differences, the two-channel WAV, the JSON."""
    st = binaural_state(r)
    mic = st.microphones["head"]
    assert mic.n_capsules == 2 and mic.metadata["channel_layout_type"] == "binaural" and mic.metadata["capsule_names"] == ["left", "right"]
    assert mic.metadata["is_spherical"] is True and mic.metadata["sphere"]["radius"] == HEAD
    coords = np.asarray(mic.metadata["coordinates_absolute"])
    assert np.allclose(np.linalg.norm(coords - BIN_HEAD, axis=1), HEAD) and coords[0, 1] > BIN_HEAD[1] > coords[1, 1]      # left is +y
    scene = core.Scene(0.5, st, sample_rate=int(FS))
    clip = sc._clip(4000, 3)
    scene.add_event(core.Event("talk", clip, int(FS), snr=10.0, scene_start=0.1, n_emitters=1))

    def refuse(*a, **k):
        raise AssertionError("an IR tensor went through the host")

    monkeypatch.setattr(engine.Renderer, "upload_irs", refuse)
    audio = scene.generate(str(tmp_path), metadata_dcase=False)["head"]
    monkeypatch.undo()
    from scipy.io import wavfile

    rate, frames = wavfile.read(str(tmp_path / "audio_out_head.wav"))
    assert rate == int(FS) and frames.shape == (round(0.5 * FS), 2) and np.abs(frames).max() > 0 and audio.shape == (2, round(0.5 * FS))
    ir = np.asarray(st.irs["head"])[:, 0].astype(np.float64)                 # (2, ir_len)
    d = np.linalg.norm(BIN_TALKER - BIN_HEAD)
    arrival = d * FS / sc.C_SOUND
    # the direct path alone: the first reflection (the +y wall, 0.7 m behind the talker) arrives 65 samples later
    lo, hi = int(arrival) - 30, int(arrival) + 35
    win = ir[:, lo:hi]
    energy = (win * win).sum(axis=1)
    centroid = (win * win) @ np.arange(lo, hi) / energy
    lag, geometric, _ = direct_path_lag(FS)
    print(f"binaural scene: left / right direct energy {energy[0] / energy[1]:.2f}, lag {centroid[1] - centroid[0]:.3f} samples = "
          f"{(centroid[1] - centroid[0]) / geometric:.3f} of the geometric {geometric:.3f} (the filters alone: {lag / geometric:.3f})")
    assert energy[0] > energy[1]                                             # ILD: the near ear is louder
    assert 1.0 <= (centroid[1] - centroid[0]) / geometric <= 1.15            # ITD: the far ear lags by the creeping-wave path
    early = (ir[:, : int(0.02 * FS)] ** 2).sum(axis=1)
    assert early[0] > early[1]
    # the scene's JSON brings the listener back
    meta = json.loads((tmp_path / "metadata_out.json").read_text())
    assert meta["state"]["microphones"]["head"]["sphere"]["centre"] == BIN_HEAD.tolist()
    again = core.Scene.from_json(str(tmp_path / "metadata_out.json"), {"talk": clip})
    assert isinstance(again.state, core.ShoeboxIRState) and "head" in again.state._spheres
    again.state.renderer = r
    again.state.simulate()
    assert np.array_equal(bits(np.asarray(again.state.irs["head"])), bits(np.asarray(st.irs["head"])))


def run_state(r):
    """A sphere array beside an omni microphone: the rows against the restatement, the tail's channels numbered through the
    microphones, the JSON round trip, and a dictionary from before."""
    room, ir_len = sc.ROOMS["oblong"], 600
    tail = dict(mix_time=0.012, fade_time=0.004, rt60=None, seed=0x1234567890ABCDEF)           # M = 192, F = 64 at 16 kHz
    st = core.ShoeboxIRState(room, betas=tc.BETAS, ir_len=ir_len, sample_rate=sc.SR, max_order=3, renderer=r, tail=tail)
    st.add_microphone("mic000", sc.CAPSULES_3[2:])
    st.add_sphere_microphone("array", CENTRE, 2.0 * DIRECTIONS_5, radius=ARRAY, n_orders=6, half=16, capsule_names=list("abcde"))
    st.add_emitters(SOURCES_3[:2])
    mic = st.microphones["array"]
    assert mic.n_capsules == 5 and mic.metadata["is_spherical"] is True and mic.metadata["capsule_names"] == list("abcde")
    assert mic.metadata["sphere"] == dict(centre=CENTRE.tolist(), radius=ARRAY, n_orders=6, half=16, directions=DIRECTIONS_5.tolist())
    assert np.allclose(np.asarray(mic.metadata["coordinates_absolute"]), CENTRE + ARRAY * DIRECTIONS_5, rtol=0, atol=1e-15)
    st.simulate()
    t = st.irs["array"]
    assert isinstance(t, shoebox.DeviceIRTensor) and t.shape == (5, 2, ir_len)
    M, F = shoebox.tail_samples(st.tail, room, sc.SR)
    assert (M, F) == (192, 64)
    b, psi = shoebox.sphere_filters(ARRAY, float(sc.SR), n_orders=6, half=16), shoebox.sphere_diffuse_filter(ARRAY, float(sc.SR), n_orders=6, half=16)
    ln_env = np.tile(shoebox.tail_envelope(room, tc.BETAS, ir_len, float(sc.SR), M), (2, 1))
    h64, bound = restate_tail(room, tc.BETAS, 0.0, SOURCES_3[:2], None, CENTRE, DIRECTIONS_5, b, psi, ir_len, float(sc.SR), M, F, ln_env,
                              tail["seed"], 0, 1, max_order=3)                          # the array's capsules follow mic000's one
    assert_within(np.asarray(t), h64, bound, "state with a tail")
    d = json.loads(json.dumps(st.to_dict()))
    assert core.ShoeboxIRState.describes(d)
    again = core.ShoeboxIRState.from_dict(d, renderer=r)
    assert json.loads(json.dumps(again.to_dict())) == d
    again.simulate()
    for alias in ("mic000", "array"):
        assert np.array_equal(bits(np.asarray(again.irs[alias])), bits(np.asarray(st.irs[alias]))), alias
    # without the written directions they come from the coordinates (to rounding: within the bound, not bit for bit)
    del d["microphones"]["array"]["sphere"]["directions"]
    loose = core.ShoeboxIRState.from_dict(d, renderer=r)
    assert np.allclose(loose._spheres["array"]["directions"], DIRECTIONS_5, rtol=0, atol=1e-13)
    # A DICTIONARY FROM BEFORE (no sphere anywhere) loads unchanged and generates al_ism_shoebox's bits
    old = {"backend": "SHOEBOX", "sample_rate": sc.SR, "emitters": {"emitters000": sc.SOURCES_5[:2].tolist()},
           "microphones": {"mic000": {"micarray_type": "MicArray", "coordinates_absolute": sc.CAPSULES_3.tolist(), "n_capsules": 3}},
           "shoebox": {"room": list(room), "betas": list(sc.UNEQUAL_BETAS), "rt60": None, "ir_len": 300, "c": 343.0, "max_order": 2}}
    loaded = core.ShoeboxIRState.from_dict(json.loads(json.dumps(old)), renderer=r)
    assert not loaded._spheres and loaded.to_dict()["shoebox"] == old["shoebox"]
    loaded.simulate()
    want = sc.run_abi(r, room, sc.UNEQUAL_BETAS, sc.SOURCES_5[:2], sc.CAPSULES_3, 300, sc.SR, max_order=2)
    assert np.array_equal(bits(np.asarray(loaded.irs["mic000"])), bits(want[:, :, :300]))


def run_round_trip_directions(r=None):
    """The JSON round trip keeps the directions BIT FOR BIT on directions that are no fixed points of a division by their length:
    the default binaural ears, ears turned obliquely, 32 seeded random capsules (DIRECTIONS_5 of run_state happens to consist of
    fixed points).  check_directions is idempotent, whatever the length of what it is given.  With a renderer the rows generated from
    the dictionary have the bits of the first state's."""
    u64 = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)                           # noqa: E731
    rng = np.random.default_rng(2024)
    raw = rng.standard_normal((4096, 3)) * 10.0 ** rng.uniform(-3.0, 3.0, (4096, 1))
    once = shoebox.check_directions(raw)
    assert np.array_equal(u64(shoebox.check_directions(once)), u64(once)), "check_directions is not idempotent"
    assert np.abs((once * once).sum(axis=1) - 1.0).max() <= shoebox.UNIT_TOLERANCE
    assert np.abs(once - raw / np.linalg.norm(raw, axis=1)[:, None]).max() <= 4e-16
    far = shoebox.check_directions([[3e200, 4e200, 0.0], [3e-200, 0.0, -4e-200]])
    assert np.allclose(far, [[0.6, 0.8, 0.0], [0.6, 0.0, -0.8]], rtol=0, atol=1e-15)
    for ears in (shoebox.binaural_directions(), shoebox.binaural_directions((0.3, -0.7, 0.2), (0.1, 0.2, 0.9), 97.0)):
        assert np.array_equal(u64(shoebox.check_directions(ears)), u64(ears))                           # unit to rounding: taken as they are
    # dividing the default ears by their computed length again WOULD move them: the round trip must not do that
    ears = shoebox.binaural_directions()
    assert not np.array_equal(u64(ears / np.sqrt((ears * ears).sum(axis=1))[:, None]), u64(ears))
    st = core.ShoeboxIRState(BIN_ROOM, betas=tc.BETAS, ir_len=300, sample_rate=int(FS), max_order=2, renderer=r)
    st.add_binaural_listener("head", BIN_HEAD)
    st.add_binaural_listener("tilted", [1.0, 2.0, 1.1], forward=(0.3, -0.7, 0.2), up=(0.1, 0.2, 0.9), ear_angle_deg=97.0)
    st.add_sphere_microphone("array", [3.0, 1.0, 1.5], rng.standard_normal((32, 3)), radius=ARRAY, n_orders=6, half=16)
    st.add_emitters([BIN_TALKER])
    assert np.array_equal(u64(st._spheres["head"]["directions"]), u64(shoebox.binaural_directions()))
    d = json.loads(json.dumps(st.to_dict()))
    again = core.ShoeboxIRState.from_dict(d, renderer=r)
    assert json.loads(json.dumps(again.to_dict())) == d
    for alias in ("head", "tilted", "array"):
        assert np.array_equal(u64(again._spheres[alias]["directions"]), u64(st._spheres[alias]["directions"])), alias
        assert np.array_equal(u64(again._capsules[alias]), u64(st._capsules[alias])), alias
    third = core.ShoeboxIRState.from_dict(json.loads(json.dumps(again.to_dict())), renderer=r)
    assert json.loads(json.dumps(third.to_dict())) == d
    if r is not None:
        st.simulate()
        again.simulate()
        for alias in ("head", "tilted", "array"):
            assert np.array_equal(bits(np.asarray(again.irs[alias])), bits(np.asarray(st.irs[alias]))), alias


# ----------------------------------------------------------------------------- 6. refusals
def run_abi_refusals(r):
    mem, lib = r.mem, r.lib
    src, dirs = mem.upload(np.array([1.0, 1.0, 1.0])), mem.upload(np.array([0.0, 0.0, 1.0]))
    out = mem.upload(np.full(64, sc.SENTINEL, dtype=np.float32))
    table, psi, env = mem.upload(random_table(2, 8).reshape(-1)), mem.upload(random_table(1, 8)[0]), mem.upload(np.full(2, -3.0))
    per_pair = per_pair_bytes(r, 2, 8, 30)
    assert per_pair == 2 * 256 * 8 == per_pair_bytes(r, 2, 8, 1000, 10, 5) < per_pair_bytes(r, 2, 8, 1000)
    ws = mem.upload(np.full(per_pair // 8 + 2, 7.5))
    good = dict(sources=mem.ptr(src), n=1, spat=None, centre=(2.0, 1.5, 1.2), dirs=mem.ptr(dirs), n_cap=1, L=(3.0, 2.5, 2.0), beta=(0.5,) * 6,
                air=0.0, table=mem.ptr(table), n_orders=2, half=8, psi=mem.ptr(psi), c=343.0, fs=16000.0, order=-1, ir_len=30, pitch=32, mix=-1,
                fade=0, seed=1, sid0=0, cid0=0, env=mem.ptr(env), n_knots=2, ws=mem.ptr(ws), ws_bytes=per_pair, out=mem.ptr(out))

    def call(**change):
        a = dict(good, **change)
        vec = lambda v, n: None if v is None else (ct.c_double * n)(*v)                                     # noqa: E731
        return lib.call("al_ism_shoebox_sphere", a["sources"], a["n"], a["spat"], vec(a["centre"], 3), a["dirs"], a["n_cap"], vec(a["L"], 3),
                        vec(a["beta"], 6), a["air"], a["table"], a["n_orders"], a["half"], a["psi"], a["c"], a["fs"], a["order"], a["ir_len"],
                        a["pitch"], a["mix"], a["fade"], a["seed"], a["sid0"], a["cid0"], a["env"], a["n_knots"], a["ws"], a["ws_bytes"],
                        a["out"], mem.stream())

    # everything al_ism_shoebox refuses, with its messages
    old = [dict(L=(0.0, 2.5, 2.0)), dict(L=(3.0, 2.5, float("inf"))), dict(c=0.0), dict(c=float("nan")), dict(fs=-1.0),
           dict(beta=(0.5,) * 5 + (1.01,)), dict(beta=(-0.01,) + (0.5,) * 5), dict(beta=(float("nan"),) + (0.5,) * 5), dict(n=0), dict(n_cap=0),
           dict(ir_len=0), dict(pitch=28), dict(pitch=34, ir_len=33), dict(order=-2), dict(sources=None), dict(dirs=None), dict(out=None),
           dict(L=None), dict(beta=None), dict(centre=None)]
    for change in old:
        nd.raises_badarg(lambda: call(**change), "al_ism_shoebox_sphere failed", "al_ism_shoebox: ")
    new = [(dict(n_orders=0), "n_orders must be in 1 .. 64"), (dict(n_orders=65), "n_orders must be in 1 .. 64"), (dict(n_orders=-1), "n_orders must be"),
           (dict(half=0), "half must be in 1 .. 1024"), (dict(half=1025), "half must be in 1 .. 1024"), (dict(table=None), "null filter table"),
           (dict(centre=(2.0, float("nan"), 1.2)), "centre must be finite"), (dict(air=-1.0), "air must be finite"),
           (dict(air=float("inf")), "air must be finite"), (dict(ws=None), "workspace must be 16-byte aligned"),
           (dict(ws=mem.ptr(ws) + 8), "workspace must be 16-byte aligned"), (dict(ws_bytes=per_pair - 1), "workspace smaller than"),
           (dict(ws_bytes=0), "workspace smaller than"), (dict(ws_bytes=-per_pair), "workspace smaller than"),
           (dict(L=(2.0e-5, 2.5, 2.0), half=1024, ws_bytes=1 << 40), "mirror cells"),
           # with a tail
           (dict(mix=10, fade=5, psi=None), "null diffuse-field filter"), (dict(mix=10, fade=0), "fade must be >= 1"),
           (dict(mix=10, fade=5, sid0=-1), "must be >= 0"), (dict(mix=10, fade=5, cid0=1 << 32), "must not exceed 2^32"),
           (dict(mix=10, fade=5, n_knots=3), "n_knots must be"), (dict(mix=10, fade=5, env=None), "null envelope table"),
           (dict(mix=10, fade=5, out=mem.ptr(out) + 4), "out must be 16-byte aligned")]
    for change, needle in new:
        nd.raises_badarg(lambda: call(**change), "al_ism_shoebox_sphere failed", needle)
    assert np.all(np.asarray(mem.download(out)) == sc.SENTINEL), "a refused call wrote"
    assert np.all(np.asarray(mem.download(ws)) == 7.5), "a refused call wrote the workspace"
    for args in ((0, 8, 30, -1, 0), (65, 8, 30, -1, 0), (2, 0, 30, -1, 0), (2, 1025, 30, -1, 0), (2, 8, 0, -1, 0), (2, 8, 30, 5, 0)):
        assert lib.call("al_ism_shoebox_sphere_workspace_bytes", *args) == _hip.AL_E_BADARG, args
    assert lib.call("al_ism_shoebox_sphere_workspace_bytes", 64, 1024, 1, -1, 0) == 64 * (2048 + 256) * 8
    assert call() == 0
    assert call(ws_bytes=per_pair + 15) == 0                                 # part of a pair more: one pair per pass
    assert call(mix=10, fade=5) == 0 and call(psi=None, env=None, n_knots=0) == 0      # without a tail its arguments are not looked at
    assert call(order=0, beta=(0.0, 1.0) * 3) == 0


def run_python_errors(r):
    room = (3.0, 2.5, 2.0)
    ok = dict(room=room, betas=(0.5,) * 6, sources=[[1.0, 1.0, 1.0]], centre=[2.0, 1.5, 1.2], directions=[[0.0, 0.0, 1.0], [1.0, 1.0, 0.0]],
              radius=0.05, ir_len=64, sample_rate=16000)
    bad = [dict(centre=[2.96, 1.5, 1.2]), dict(centre=[2.0, 1.5, 0.04]), dict(centre=[2.0, 1.5]), dict(centre=[2.0, np.nan, 1.2]),     # not wholly inside
           dict(radius=0.0), dict(radius=-0.05), dict(radius=np.inf), dict(radius=1.3),
           dict(sources=[[2.0, 1.5, 1.29]]), dict(sources=[[1.0, 1.0, 1.0], [2.05, 1.5, 1.25]]),     # closer than 2 radius to the centre
           dict(directions=[[0.0, 0.0, 0.0]]), dict(directions=[[0.0, np.nan, 1.0]]), dict(directions=[[0.0, 1.0]]), dict(directions=[0.0, 0.0, 1.0]),
           dict(directions=np.zeros((0, 3))), dict(betas=np.full((6, 2), 0.5)), dict(betas=(1.5,) + (0.5,) * 5), dict(ir_len=0),
           dict(n_orders=3), dict(n_orders=65), dict(half=0), dict(half=1025), dict(workspace_cap=-1), dict(air=-1.0),
           dict(source_patterns=np.zeros((1, 4))), dict(tail=shoebox.ShoeboxTail(seed=1), capsule_id0=1 << 32),
           dict(tail=shoebox.ShoeboxTail(seed=1), betas=(0.0,) + (0.5,) * 5)]
    for change in bad:
        with pytest.raises(ValueError):
            shoebox.shoebox_sphere_irs_device(r, **dict(ok, **change))
    buf, strides, n = shoebox.shoebox_sphere_irs_device(r, **ok)
    assert strides == (64, 64) and n == 64
    buf, strides, n = shoebox.shoebox_sphere_irs_device(r, **dict(ok, ir_len=600, tail=shoebox.ShoeboxTail(seed=5), air=1e-3, n_orders=8))
    assert strides == (600, 600) and n == 600
    # the workspace cap does not change a bit, and unnormalised directions are the same capsules
    a = np.asarray(r.mem.download(shoebox.shoebox_sphere_irs_device(r, **dict(ok, ir_len=300))[0]))
    b = np.asarray(r.mem.download(shoebox.shoebox_sphere_irs_device(r, **dict(ok, ir_len=300, workspace_cap=0, directions=[[0.0, 0.0, 2.0], [1.0, 1.0, 0.0]]))[0]))
    assert np.array_equal(bits(a[:600]), bits(b[:600])) and np.abs(a[:600]).max() > 0
    for change in (dict(forward=(0.0, 0.0, 1.0)), dict(up=(0.0, 0.0, 0.0)), dict(ear_angle_deg=0.0), dict(ear_angle_deg=180.0), dict(forward=(1.0, 0.0))):
        with pytest.raises(ValueError):
            shoebox.binaural_directions(**change)
    ears = shoebox.binaural_directions((2.0, 0.0, 5.0), (0.0, 0.0, 3.0), 90.0)
    assert np.allclose(ears, [[0.0, 1.0, 0.0], [0.0, -1.0, 0.0]], rtol=0, atol=1e-15)
    # the state
    st = core.ShoeboxIRState(room, betas=(0.5,) * 6, ir_len=64, sample_rate=16000, renderer=r)
    st.add_emitters([[1.0, 1.0, 1.0]])
    for kw in (dict(centre=[2.96, 1.5, 1.2]), dict(centre=[1.05, 1.0, 1.0]), dict(directions=[[0.0, 0.0, 0.0]]), dict(radius=0.0), dict(n_orders=2),
               dict(capsule_names=["a"])):
        with pytest.raises(ValueError):
            st.add_sphere_microphone("m", **dict(dict(centre=[2.0, 1.5, 1.2], directions=[[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]], radius=0.05), **kw))
    with pytest.raises(ValueError):
        st.add_binaural_listener("h", [1.1, 1.0, 1.0])                       # the emitter is 10 cm from the head's centre
    st.add_binaural_listener("h", [2.0, 1.5, 1.2])
    with pytest.raises(KeyError):
        st.add_binaural_listener("h", [2.0, 1.5, 1.0])
    with pytest.raises(ValueError):
        st.add_emitters([[2.0, 1.5, 1.3]])                                   # inside 2 radius of the head that is there now
    banded = core.ShoeboxIRState(room, betas=np.full((6, 2), 0.5), bands=shoebox.ShoeboxBands((500.0, 2000.0), 8), ir_len=64, sample_rate=16000,
                                 renderer=r)
    with pytest.raises(ValueError, match="not yet"):
        banded.add_binaural_listener("h", [2.0, 1.5, 1.2])


# ----------------------------------------------------------------------------- 7. schedule independence
def run_shake_rows(r):
    """{name: rows} of one call without a tail and one with, both held to their restatement first: nine orders (three gathers per
    pass), half = 64, two passes over the workspace; with the tail k_ism_sphere_combine under the fade and k_ism_band_tail past it.
    tests/test_gpu_shoebox_sphere.py compares the rows of differently scheduled builds bit for bit."""
    room, src, dirs, b = sc.ROOMS["oblong"], SOURCES_3, DIRECTIONS_5[2:4], random_table(9, 64)
    psi = random_table(1, 64, seed=7)[0]
    plain = run_sphere(r, room, tc.BETAS, src, None, CENTRE, dirs, 0.0, b, 700, FS, max_order=3, pairs_per_pass=4)[:, :, :700]
    h64, bound = restate(room, tc.BETAS, 0.0, src, None, CENTRE, dirs, b, 700, FS, max_order=3)
    assert_within(plain, h64, bound, "schedule independence: no tail")
    ln_env = tail_tables(3, 1000)
    tailed = run_sphere(r, room, tc.BETAS, src, None, CENTRE, dirs, 0.0, b, 1000, FS, max_order=3, pairs_per_pass=4,
                        tail=dict(M=300, F=100, psi=psi, ln_env=ln_env))[:, :, :1000]
    h64_t, bound_t = restate_tail(room, tc.BETAS, 0.0, src, None, CENTRE, dirs, b, psi, 1000, FS, 300, 100, ln_env, SEED, 0, 0, max_order=3)
    assert_within(tailed, h64_t, bound_t, "schedule independence: tail")
    return {"sphere": plain, "sphere_tail": tailed}
