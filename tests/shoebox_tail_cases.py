"""Scenarios of the diffuse tail of the device shoebox IR generator (al_ism_shoebox_tail, shoebox.ShoeboxTail, shoebox.tail_envelope,
core.ShoeboxIRState(tail=...)) and the float64 numpy restatement of its definition (DESIGN.md "Shoebox IRs: the diffuse tail"; no
reference code computes this).  tests/test_hostemu_shoebox_tail.py runs them on the host-emulated kernels,
tests/test_gpu_shoebox_tail.py on the gfx950 build.

THE DEFINITION.  For t in [0, ir_len) of row (c, n), with the mixing sample M, the fade F and the knot table ln_env:
    x = clamp((t - M) / F, 0, 1), w_e = cos(pi x / 2), w_l = sin(pi x / 2)   (exactly (1, 0) for t <= M, (0, 1) for t >= M + F)
    e(t) = exp((1 - p) ln_env[k] + p ln_env[k + 1]), k = t // 256, p = (t % 256) / 256   (p == 0 reads knot k alone)
    g(t) = normal t % 4 of Philox-4x32-10 block (t // 4, source_id0 + n, 4, capsule_id0 + c) under key (seed lo, seed hi)
    h = w_e y_ism(t) + w_l e(t) g(t), no noise term where w_l == 0; float64, rounded to float32 once; pads +0.

THE BOUND (derived, not tuned), every sample, none excluded.  With h64 the restatement, y64 / A of tests/shoebox_cases.py:
    |h - h64| <= w_e 2^-30 A[t]  +  w_l e(t) (RTOL |g64(t)| + ATOL)  +  2^-24 |h64|  +  2^-150
  1. the image part: shoebox_cases' bound without its float32 rounding (the sum is not rounded on its own here), scaled by w_e;
  2. the draw: noise_draw_cases.RTOL / ATOL of one normal against its float64 restatement, as they stand, scaled by w_l e(t)
     (the float64 envelope and fade weights differ from numpy's by a few 1e-16, four orders below RTOL);
  3. the one rounding of the result to float32, half an ulp <= 2^-24 |value|; below the normal range half a subnormal step, 2^-150.
"""
import ctypes as ct
import functools
import json

import numpy as np
import pytest

from audiblelight_amd import _hip, batch, core, engine, shoebox
from oracle import synth_oracle as orc
from tests import noise_draw_cases as nd
from tests import shoebox_cases as sc

TAG = 4
FS = 16000.0
ROOM = sc.ROOMS["oblong"]
BETAS = (0.95, 0.9, 0.75, 0.8, 0.6, 0.85)          # all six positive and unequal
SEED = 0xA5A5F00D12345678
Y_LEN = 520                                          # the image oracle is computed once to this length: every scenario has M + F <= 513
bits = sc.bits


# ----------------------------------------------------------------------------- the restatement
@functools.lru_cache(maxsize=None)
def _block(seed, sid, cid, q):
    """The four N(0, 1) of the tail's Philox block q of (source sid, capsule cid), float64 (Box-Muller as noise_draw_cases._block)."""
    x = orc.philox4x32_10((q & 0xffffffff, sid & 0xffffffff, TAG, cid & 0xffffffff), (seed & 0xffffffff, seed >> 32))
    out = []
    for h in range(2):
        u1 = (np.float32(x[2 * h]) + np.float32(0.5)) * np.float32(2.0 ** -32)
        u2 = np.float32(x[2 * h + 1]) * np.float32(2.0 ** -32)
        rad = np.sqrt(-2.0 * np.log(np.float64(u1)))
        out += [rad * np.cos(2 * np.pi * np.float64(u2)), rad * np.sin(2 * np.pi * np.float64(u2))]
    return tuple(float(v) for v in out)


def restated_g(seed, sid, cid, n):
    return np.array([_block(int(seed), int(sid), int(cid), q) for q in range((n + 3) // 4)], dtype=np.float64).reshape(-1)[:n]


def weights(ir_len, M, F):
    x = np.clip((np.arange(ir_len) - float(M)) / float(F), 0.0, 1.0)
    mid = (x > 0.0) & (x < 1.0)
    w_e, w_l = (x <= 0.0).astype(np.float64), (x >= 1.0).astype(np.float64)
    w_e[mid], w_l[mid] = np.cos(0.5 * np.pi * x[mid]), np.sin(0.5 * np.pi * x[mid])
    return w_e, w_l


def envelope(ln_env, ir_len):
    t = np.arange(ir_len)
    k, p = t // 256, (t % 256) / 256.0
    ln_env = np.asarray(ln_env, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ln = np.where(p == 0.0, ln_env[k], (1.0 - p) * ln_env[k] + p * ln_env[k + 1])
        return np.exp(ln)


def restate(y64, A, ln_env, ir_len, M, F, seed, sid, cid):
    """(h64, bound) of one row; y64 and A need to reach min(ir_len, M + F) only."""
    w_e, w_l = weights(ir_len, M, F)
    y, a = np.zeros(ir_len), np.zeros(ir_len)
    m = min(ir_len, len(y64))
    assert m >= min(ir_len, M + F)
    y[:m], a[:m] = y64[:m], A[:m]
    e, g = envelope(ln_env, ir_len), restated_g(seed, sid, cid, ir_len)
    noise = np.where(w_l > 0.0, w_l * e * g, 0.0)
    h = w_e * y + noise
    bound = w_e * 2.0 ** -30 * a + np.where(w_l > 0.0, w_l * e * (nd.RTOL * np.abs(g) + nd.ATOL), 0.0) + 2.0 ** -24 * np.abs(h) + 2.0 ** -150
    return h, bound


WORST = {"fraction": 0.0}


def assert_rows(rows, y64, A, ln_env, ir_len, M, F, seed, sid0, cid0, what):
    C, N = rows.shape[:2]
    assert np.all(bits(rows[:, :, ir_len:]) == 0), (what, "pad samples must be +0")
    worst = 0.0
    for ci in range(C):
        for ni in range(N):
            h, bound = restate(y64[ci, ni], A[ci, ni], ln_env, ir_len, M, F, seed, sid0 + ni, cid0 + ci)
            err = np.abs(rows[ci, ni, :ir_len].astype(np.float64) - h)
            assert np.all(np.isfinite(rows[ci, ni])), what
            frac = float((err / bound).max())
            worst = max(worst, frac)
            assert np.all(err <= bound), (what, (ci, ni), "sample", int(np.argmax(err / bound)), "err / bound", frac)
    WORST["fraction"] = max(WORST["fraction"], worst)
    print(f"shoebox tail bound [{what}]: max err / bound {worst:.3f} (so far {WORST['fraction']:.3f})")


# ----------------------------------------------------------------------------- running the entry point
def run_tail_abi(r, sources, capsules, ir_len, M, F, seed=SEED, sid0=0, cid0=0, ln_env=None, max_order=None, pitch=None, room=ROOM,
                 betas=BETAS, fs=FS, c=sc.C_SOUND):
    """al_ism_shoebox_tail into a buffer with sc.GUARD sentinels on either side; the (C, N, pitch) rows, the guards checked."""
    mem, lib = r.mem, r.lib
    sources = np.ascontiguousarray(np.atleast_2d(sources), dtype=np.float64)
    capsules = np.ascontiguousarray(np.atleast_2d(capsules), dtype=np.float64)
    n, n_cap = len(sources), len(capsules)
    pitch = shoebox.pitch_of(ir_len) if pitch is None else pitch
    total = n_cap * n * pitch
    if ln_env is None:
        ln_env = shoebox.tail_envelope(room, betas, ir_len, fs, min(M, ir_len), c)
    ln_env = np.ascontiguousarray(ln_env, dtype=np.float64)
    out = mem.upload(np.full(total + 2 * sc.GUARD, sc.SENTINEL, dtype=np.float32))
    src_dev, cap_dev, env_dev = mem.upload(sources.reshape(-1)), mem.upload(capsules.reshape(-1)), mem.upload(ln_env)
    L, beta = (ct.c_double * 3)(*room), (ct.c_double * 6)(*betas)
    lib.call("al_ism_shoebox_tail", mem.ptr(src_dev), n, mem.ptr(cap_dev), n_cap, L, beta, float(c), float(fs),
             -1 if max_order is None else int(max_order), int(ir_len), int(pitch), int(M), int(F), int(seed), int(sid0), int(cid0),
             mem.ptr(env_dev), len(ln_env), mem.ptr(out) + 4 * sc.GUARD, mem.stream())
    host = np.asarray(mem.download(out))
    assert np.all(host[:sc.GUARD] == sc.SENTINEL) and np.all(host[sc.GUARD + total:] == sc.SENTINEL), "guard overwritten"
    assert not np.any(host[sc.GUARD: sc.GUARD + total] == sc.SENTINEL), "a sample was not written"
    return host[sc.GUARD: sc.GUARD + total].reshape(n_cap, n, pitch).copy(), ln_env


def points(pairs):
    return (sc.SOURCES_5, sc.CAPSULES_3) if pairs == "3x5" else (sc.SOURCES_5[1:2], sc.CAPSULES_3[:1])


def image_oracle(pairs, max_order):
    src, cap = points(pairs)
    y64, A, _ = sc.oracle(ROOM, BETAS, src, cap, Y_LEN, FS, max_order=max_order)
    return y64, A


# ----------------------------------------------------------------------------- 1. parity with the restatement
def _cfg(M, F, ir_len=1100, pairs="1x1", order=None, pitch=None, sid0=0, cid0=0):
    return (M, F, ir_len, pairs, order, pitch, sid0, cid0)


PARITY = (
    [_cfg(M, F) for M in (0, 1, 255, 256, 400) for F in (1, 100)]
    + [_cfg(400, F) for F in (111, 112, 113)]                      # M + F = 511, 512, 513: the split on either side of a tile edge
    + [_cfg(400, 100, ir_len=450), _cfg(300, 1000, ir_len=500)]    # M + F > ir_len: the fade is cut by the row end
    + [_cfg(400, 100, ir_len=512 + d) for d in (0, 1, 3, 4, 5)]    # the split of these is 512: no tail sample, then 1, 3, 4, 5
    + [_cfg(400, 100, ir_len=1500)]
    + [_cfg(400, 100, pitch=1400), _cfg(400, 100, ir_len=513, pitch=1024 + 512 + 8)]     # a pitch beyond pitch_of(ir_len)
    + [_cfg(400, 100, order=1), _cfg(0, 1, order=1)]
    # a row longer than one workgroup of k_ism_tail (4096 samples past the split at 256), the second one ending in a part quad
    + [_cfg(100, 50, ir_len=256 + 4096 + 5, order=1, sid0=0xFFFFFFF0, cid0=9)]
    + [_cfg(400, 100, pairs="3x5", sid0=7, cid0=3), _cfg(255, 1, pairs="3x5", order=1, pitch=1200, sid0=1, cid0=0xFFFFFFFD)]
)


def run_parity(r, M, F, ir_len, pairs, order, pitch, sid0, cid0):
    src, cap = points(pairs)
    y64, A = image_oracle(pairs, order)
    rows, ln_env = run_tail_abi(r, src, cap, ir_len, M, F, sid0=sid0, cid0=cid0, max_order=order, pitch=pitch)
    assert_rows(rows, y64, A, ln_env, ir_len, M, F, SEED, sid0, cid0, (M, F, ir_len, pairs, order, pitch))
    if ir_len > M + F:
        assert np.all(rows[:, :, M + F: ir_len] != 0.0), "a tail sample is zero"


# ----------------------------------------------------------------------------- 2. no tail: today's bits
def run_no_tail_is_todays_bits(r):
    src, cap = points("3x5")
    ir_len = 520
    for pitch in (None, 768 + 8):
        want = sc.run_abi(r, ROOM, BETAS, src, cap, ir_len, FS, max_order=3, pitch=pitch)
        for M, F in ((ir_len, 1), (ir_len, 100), (ir_len + 1000, 7), (1 << 40, 1), (ir_len, (1 << 62)), ((1 << 62), (1 << 62))):
            got, _ = run_tail_abi(r, src, cap, ir_len, M, F, max_order=3, pitch=pitch)
            assert np.array_equal(bits(got), bits(want)), ("tail with mix >= ir_len differs from al_ism_shoebox", M, F, pitch)
    # M = ir_len - 1: the last sample alone is at or below M too, so even that call has no noise in it
    got, _ = run_tail_abi(r, src[:1], cap[:1], ir_len, ir_len - 1, 5, max_order=3)
    assert np.array_equal(bits(got), bits(sc.run_abi(r, ROOM, BETAS, src[:1], cap[:1], ir_len, FS, max_order=3)))


# ----------------------------------------------------------------------------- 3. the identity of a row
def run_row_identity(r):
    src, cap = points("3x5")
    ir_len, M, F, sid0, cid0 = 700, 100, 50, 7, 3
    run = lambda s=src, m=cap, **k: run_tail_abi(r, s, m, ir_len, M, F, **dict(dict(sid0=sid0, cid0=cid0, max_order=2), **k))[0]   # noqa: E731
    one = run()
    assert np.array_equal(bits(one), bits(run())), "two runs differ"
    wide = run(pitch=1024 + 256 + 4)
    assert np.array_equal(bits(wide[:, :, :ir_len]), bits(one[:, :, :ir_len])) and np.all(bits(wide[:, :, ir_len:]) == 0)
    for ci, ni in ((0, 0), (1, 3), (2, 4)):
        alone = run(src[ni], cap[ci], sid0=sid0 + ni, cid0=cid0 + ci)
        assert np.array_equal(bits(alone[0, 0]), bits(one[ci, ni])), (ci, ni)
        # up to and including M the row is the image sum; every later sample carries noise of its own stream
        for what, other in (("seed", run(src[ni], cap[ci], sid0=sid0 + ni, cid0=cid0 + ci, seed=SEED ^ (1 << 32))),
                            ("seed low word", run(src[ni], cap[ci], sid0=sid0 + ni, cid0=cid0 + ci, seed=SEED + 1)),
                            ("source id", run(src[ni], cap[ci], sid0=sid0 + ni + 1, cid0=cid0 + ci)),
                            ("capsule id", run(src[ni], cap[ci], sid0=sid0 + ni, cid0=cid0 + ci + 1))):
            assert np.array_equal(bits(other[0, 0, :M + 1]), bits(alone[0, 0, :M + 1])), what
            assert np.all(other[0, 0, M + 1: ir_len] != alone[0, 0, M + 1: ir_len]), (what, "left some tail samples as they were")
    tails = one[:, :, M + F: ir_len].reshape(15, -1)
    for a in range(15):
        for b in range(a + 1, 15):
            assert np.all(tails[a] != tails[b]), ("two rows of one call share noise", a, b)


# ----------------------------------------------------------------------------- 4. the envelope table
def run_envelope_tables(r):
    src, cap = points("1x1")
    y64, A = image_oracle("1x1", 1)
    ir_len, M, F = 1300, 100, 60                     # the split is 256: k_ism_tail crosses the knots at 512, 768, 1024, 1280
    n_knots = shoebox.n_knots_of(ir_len)
    assert n_knots == 7
    rng = np.random.default_rng(3)
    # knots that do not lie on a line: an interpolation in the wrong interval, or with p of another sample, fails by far
    jagged = rng.uniform(-9.0, -2.0, n_knots)
    rows, _ = run_tail_abi(r, src, cap, ir_len, M, F, ln_env=jagged, max_order=1)
    assert_rows(rows, y64, A, jagged, ir_len, M, F, SEED, 0, 0, "jagged knots")
    # -inf everywhere: the image part under its fade, then exact zeros
    dead = np.full(n_knots, -np.inf)
    rows, _ = run_tail_abi(r, src, cap, ir_len, M, F, ln_env=dead, max_order=1)
    assert_rows(rows, y64, A, dead, ir_len, M, F, SEED, 0, 0, "-inf knots")
    assert np.all(rows[:, :, M + F:] == 0.0)
    # -inf from knot 3 on: samples 512 and below 768 ... the interval (512, 768) has one dead end and is zero, sample 512 is not
    half = jagged.copy()
    half[3:] = -np.inf
    rows, _ = run_tail_abi(r, src, cap, ir_len, M, F, ln_env=half, max_order=1)
    assert_rows(rows, y64, A, half, ir_len, M, F, SEED, 0, 0, "-inf from knot 3")
    assert np.all(rows[0, 0, 513:] == 0.0) and np.all(rows[0, 0, M + F: 513] != 0.0)


def run_envelope_law_properties():
    ir_len, fs, M = 3000, 16000.0, 700
    lin = shoebox.tail_envelope(ROOM, BETAS, ir_len, fs, M, rt60=0.3)
    assert lin.shape == (shoebox.n_knots_of(ir_len),) and lin.dtype == np.float64
    step = -(3.0 * np.log(10.0) / 0.3) * 256.0 / fs
    assert np.allclose(np.diff(lin), step, rtol=0, atol=1e-12)
    # level-matched at the mixing sample: the line through the knots passes through the image field's level at M
    at_mix = 0.5 * shoebox.tail_energy_law(ROOM, BETAS, fs)(M / fs)
    assert abs(lin[0] + step * M / 256.0 - at_mix) < 1e-12
    ism = shoebox.tail_envelope(ROOM, BETAS, ir_len, fs, M)
    assert np.all(np.diff(ism) < 0) and np.all(np.diff(ism, 2) > 0)     # decays, and ever more slowly: not an exponential
    sigma = np.sqrt(sc.C_SOUND / (4.0 * np.pi * np.prod(ROOM) * fs))
    assert abs(ism[0] - np.log(sigma)) < 1e-12                          # D(0) = 1
    rigid = shoebox.tail_envelope(ROOM, (1.0,) * 6, ir_len, fs, M)
    assert np.allclose(rigid, np.log(sigma), rtol=0, atol=1e-12)
    assert shoebox.default_mix_time((6.0, 5.0, 3.0)) == pytest.approx(0.0421, abs=1e-4)
    assert shoebox.default_mix_time((6.0, 5.0, 3.0)) == pytest.approx(np.sqrt(shoebox.MIXED_ECHO_DENSITY * 90.0 / (4 * np.pi * 343.0 ** 3)))
    t = shoebox.ShoeboxTail()
    mix, fade = shoebox.tail_samples(t, (6.0, 5.0, 3.0), 48000.0)
    assert (mix, fade) == (2022, 506)
    assert shoebox.tail_samples(shoebox.ShoeboxTail(mix_time=0.0), ROOM, fs) == (0, 1)     # the fade is at least one sample


# ----------------------------------------------------------------------------- 5. the envelope law against the image-source oracle
LAW_FS, LAW_LEN = 8000.0, 1600
LAW_ROOMS = {"6x5x3": ((6.0, 5.0, 3.0), (0.877,) * 6), "oblong": (ROOM, BETAS)}
LAW_WINDOWS_MS = ((30, 60), (60, 90), (100, 130), (150, 180))
# default_rng(1).uniform(0.15, 0.85, 3), eight draws: source, capsule, source, capsule, ... of four pairs, as fractions of the room
LAW_UNIT_POINTS = np.array([
    [0.5082751372901797, 0.8153245874281547, 0.2509117289037436], [0.8140546129960707, 0.3682820164073398, 0.4463285142808029],
    [0.7293918156743092, 0.4364393954584128, 0.5347155813711416], [0.16929137927014784, 0.6774591760723646, 0.5267003192534947],
    [0.38081220154936446, 0.701900092399883, 0.36223638050415147], [0.467448522636456, 0.24382918807301532, 0.4321790905129904],
    [0.2924186684733047, 0.33361933830929463, 0.6752552708410368], [0.34628613059022795, 0.48963368210214453, 0.836516039860867]])


def image_row(room, betas, s, r, ir_len, fs, c=sc.C_SOUND):
    """y64 of shoebox_cases.oracle_pair (the same arithmetic), vectorised over the images."""
    reach = c * (ir_len + sc.HALF) / fs
    ax = [sc._axis(s[i], r[i], room[i], betas[2 * i], betas[2 * i + 1], reach) for i in range(3)]
    Rx, Ry, Rz = np.meshgrid(ax[0][0], ax[1][0], ax[2][0], indexing="ij")
    gain = ax[0][2][:, None, None] * ax[1][2][None, :, None] * ax[2][2][None, None, :]
    d = np.sqrt(Rx * Rx + Ry * Ry + Rz * Rz)
    tau = d * fs / c
    keep = (tau - sc.HALF < ir_len) & (gain > 0.0)
    d, tau, gain = d[keep], tau[keep], gain[keep]
    a = gain / (4.0 * np.pi * d)
    t = np.ceil(tau - sc.HALF)[:, None] + np.arange(sc.TAPS + 1)[None, :]
    u = t - tau[:, None]
    ok = (np.abs(u) < sc.HALF) & (t >= 0) & (t < ir_len)
    taps = a[:, None] * 0.5 * (1.0 + np.cos(2.0 * np.pi * u / sc.TAPS)) * np.sinc(u)
    return np.bincount(t[ok].astype(np.int64), weights=taps[ok], minlength=ir_len)


def run_envelope_law_against_images():
    """A sanity band on the MODEL (not a tolerance on the kernel): the high-passed image-source energy in four windows, averaged
    over four pairs, within a factor of 2 of sigma^2 D; and the Sabine exponential is NOT within it."""
    assert np.array_equal(LAW_UNIT_POINTS, np.random.default_rng(1).uniform(0.15, 0.85, (8, 3)))
    t = np.arange(LAW_LEN)
    ratios = {}
    for name, (room, betas) in LAW_ROOMS.items():
        pts = LAW_UNIT_POINTS * np.asarray(room)[None, :]
        law = shoebox.tail_energy_law(room, betas, LAW_FS)
        model = np.exp([law(ti / LAW_FS) for ti in t])
        energy = np.zeros(LAW_LEN)
        for i in range(4):
            y = image_row(room, betas, pts[2 * i], pts[2 * i + 1], LAW_LEN, LAW_FS)
            if i == 0:     # the vectorised sum is the oracle's
                y_ref = sc.oracle_pair(room, betas, pts[0], pts[1], 400, LAW_FS)[0]
                assert np.abs(y[:400] - y_ref).max() <= 1e-12 * np.abs(y_ref).max()
            hp = y - np.convolve(y, np.ones(65) / 65.0, mode="same")      # the coherent mean of the method is not the tail's business
            energy += hp * hp / 4.0
        ratios[name] = [float(energy[int(a * 8): int(b * 8)].sum() / model[int(a * 8): int(b * 8)].sum()) for a, b in LAW_WINDOWS_MS]
        print(f"envelope law [{name}]: image energy / sigma^2 D in {LAW_WINDOWS_MS} ms = " + ", ".join(f"{v:.3f}" for v in ratios[name]))
        for v in ratios[name]:
            assert 0.5 <= v <= 2.0, (name, ratios[name])
    # Sabine in the oblong room: sigma^2 exp(-6 ln 10 t / T), T = 24 ln 10 V / (c S alpha), alpha the area mean of 1 - beta^2
    room, betas = LAW_ROOMS["oblong"]
    L, b = np.asarray(room), np.asarray(betas)
    areas = np.repeat([L[1] * L[2], L[0] * L[2], L[0] * L[1]], 2)
    T = 24.0 * np.log(10.0) * np.prod(L) / (sc.C_SOUND * float((areas * (1.0 - b * b)).sum()))
    sigma2 = sc.C_SOUND / (4.0 * np.pi * np.prod(L) * LAW_FS)
    sabine = sigma2 * np.exp(-6.0 * np.log(10.0) * t / LAW_FS / T)
    a, bnd = LAW_WINDOWS_MS[-1]
    law = shoebox.tail_energy_law(room, betas, LAW_FS)
    model_last = np.exp([law(ti / LAW_FS) for ti in t[a * 8: bnd * 8]]).sum()
    sabine_ratio = ratios["oblong"][-1] * model_last / sabine[a * 8: bnd * 8].sum()
    print(f"envelope law [oblong]: image energy / Sabine exponential (T = {T:.3f} s) in the last window = {sabine_ratio:.2f}")
    assert not 0.5 <= sabine_ratio <= 2.0, sabine_ratio
    return ratios


# ----------------------------------------------------------------------------- 6. refusals
def run_abi_refusals(r):
    mem, lib = r.mem, r.lib
    src, cap = mem.upload(np.array([1.0, 1.0, 1.0])), mem.upload(np.array([2.0, 1.5, 1.2]))
    out = mem.upload(np.full(64, sc.SENTINEL, dtype=np.float32))
    env = mem.upload(np.full(2, -3.0))
    good = dict(sources=mem.ptr(src), n=1, capsules=mem.ptr(cap), n_cap=1, L=(3.0, 2.5, 2.0), beta=(0.5,) * 6, c=343.0, fs=16000.0,
                order=-1, ir_len=30, pitch=32, mix=10, fade=5, seed=1, sid0=0, cid0=0, env=mem.ptr(env), n_knots=2, out=mem.ptr(out))

    def call(**change):
        a = dict(good, **change)
        L = None if a["L"] is None else (ct.c_double * 3)(*a["L"])
        beta = None if a["beta"] is None else (ct.c_double * 6)(*a["beta"])
        return lib.call("al_ism_shoebox_tail", a["sources"], a["n"], a["capsules"], a["n_cap"], L, beta, a["c"], a["fs"], a["order"],
                        a["ir_len"], a["pitch"], a["mix"], a["fade"], a["seed"], a["sid0"], a["cid0"], a["env"], a["n_knots"], a["out"],
                        mem.stream())

    # everything the plain entry refuses, with its messages
    old = [dict(L=(0.0, 2.5, 2.0)), dict(L=(3.0, 2.5, float("inf"))), dict(c=0.0), dict(c=float("nan")), dict(fs=-1.0),
           dict(beta=(0.5, 0.5, 1.01, 0.5, 0.5, 0.5)), dict(beta=(-0.01,) + (0.5,) * 5), dict(n=0), dict(n_cap=0), dict(ir_len=0),
           dict(pitch=28), dict(pitch=34, ir_len=33), dict(order=-2), dict(sources=None), dict(capsules=None), dict(out=None),
           dict(L=None), dict(beta=None)]
    for change in old:
        nd.raises_badarg(lambda: call(**change), "al_ism_shoebox_tail failed", "al_ism_shoebox: ")
    new = [(dict(mix=-1), "mix must be >= 0"), (dict(fade=0), "fade must be >= 1"), (dict(fade=-3), "fade must be >= 1"),
           (dict(sid0=-1), "source_id0 and capsule_id0 must be >= 0"), (dict(cid0=-1), "source_id0 and capsule_id0 must be >= 0"),
           (dict(sid0=1 << 32), "must not exceed 2^32"), (dict(cid0=1 << 32), "must not exceed 2^32"),
           (dict(sid0=(1 << 32) - 1, n=2), "must not exceed 2^32"), (dict(cid0=(1 << 32) - 1, n_cap=2), "must not exceed 2^32"),
           (dict(n_knots=1), "n_knots must be"), (dict(n_knots=3), "n_knots must be"), (dict(ir_len=257, pitch=260), "n_knots must be"),
           (dict(env=None), "null envelope table"), (dict(out=mem.ptr(out) + 4), "out must be 16-byte aligned")]
    for change, needle in new:
        nd.raises_badarg(lambda: call(**change), "al_ism_shoebox_tail: ", needle)
    assert np.all(np.asarray(mem.download(out)) == sc.SENTINEL), "a refused call wrote"
    assert call() == 0
    assert call(sid0=(1 << 32) - 1, cid0=(1 << 32) - 1, seed=(1 << 64) - 1, mix=0, fade=1) == 0     # the last id is a valid id


def run_python_errors(r):
    room, s, m = (3.0, 2.5, 2.0), [[1.0, 1.0, 1.0]], [[2.0, 1.5, 1.2]]
    Tail = shoebox.ShoeboxTail
    ok = dict(room=room, betas=(0.5,) * 6, sources=s, capsules=m, ir_len=600, sample_rate=16000, tail=Tail(seed=5))
    bad = [dict(betas=(0.0,) + (0.5,) * 5), dict(betas=(0.5,) * 5 + (0.0,)), dict(tail=Tail(mix_time=-0.01)), dict(tail=Tail(fade_time=-1.0)),
           dict(tail=Tail(mix_time=float("nan"))), dict(tail=Tail(fade_time=float("inf"))), dict(tail=Tail(rt60=0.0)),
           dict(tail=Tail(rt60=-0.5)), dict(tail=Tail(seed=1.5)), dict(tail=Tail(seed="7")), dict(tail=Tail(seed=None)),
           dict(tail=Tail(seed=-1)), dict(tail=Tail(seed=1 << 64)), dict(tail=Tail(seed=True)), dict(tail=dict(seed=1)), dict(tail=0.05),
           dict(source_id0=-1), dict(capsule_id0=-1), dict(source_id0=1.0), dict(source_id0=1 << 32), dict(capsule_id0=1 << 32)]
    for change in bad:
        with pytest.raises(ValueError):
            shoebox.shoebox_irs_device(r, **dict(ok, **change))
    buf, strides, n = shoebox.shoebox_irs_device(r, **ok)
    assert strides == (600, 600) and n == 600
    # a zero beta without a tail is still fine
    shoebox.shoebox_irs_device(r, **dict(ok, betas=(0.0,) + (0.5,) * 5, tail=None))
    for change in (dict(betas=(0.0,) + (0.5,) * 5), dict(tail=Tail(seed=1.5)), dict(tail=Tail(mix_time=-1.0)), dict(tail=dict(seed=2.5))):
        with pytest.raises(ValueError):
            core.ShoeboxIRState(**dict(dict(room=room, betas=(0.5,) * 6, tail=Tail()), **change))
    with pytest.raises(ValueError):
        shoebox.tail_envelope(room, (0.0,) + (0.5,) * 5, 600, 16000.0, 100)
    with pytest.raises(ValueError):
        shoebox.tail_envelope(room, (0.5,) * 6, 600, 16000.0, -1)
    with pytest.raises(ValueError):
        shoebox.tail_envelope(room, (0.5,) * 6, 600, 16000.0, 100, rt60=0.0)


# ----------------------------------------------------------------------------- 7. the state and the scene
MIC_A = sc.CAPSULES_3
MIC_B = np.array([[0.7, 2.6, 1.9], [0.75, 2.6, 1.9]])
STATE_TAIL = dict(mix_time=0.02, fade_time=0.005, rt60=None, seed=0x1234567890ABCDEF)      # M = 320, F = 80 at 16 kHz


def _tail_state(r, tail=STATE_TAIL, ir_len=1203, max_order=None):
    st = core.ShoeboxIRState(ROOM, betas=BETAS, ir_len=ir_len, sample_rate=sc.SR, max_order=max_order, renderer=r, tail=tail)
    st.add_microphone("mic000", MIC_A)
    st.add_microphone("mic001", MIC_B)
    st.add_emitters(sc.SOURCES_5[:1], alias="static")
    st.add_emitters(sc.SOURCES_5[1:4], alias="moving")
    return st


def run_state(r):
    st = _tail_state(r)
    assert isinstance(st.tail, shoebox.ShoeboxTail) and st.tail.seed == STATE_TAIL["seed"]
    st.simulate()
    M, F = shoebox.tail_samples(st.tail, ROOM, sc.SR)
    assert (M, F) == (320, 80)
    ln_env = shoebox.tail_envelope(ROOM, BETAS, 1203, sc.SR, M)
    first = {}
    for alias, caps, cid0 in (("mic000", MIC_A, 0), ("mic001", MIC_B, 3)):       # capsules are numbered through the microphones
        t = st.irs[alias]
        assert isinstance(t, shoebox.DeviceIRTensor) and t.shape == (len(caps), 4, 1203)
        y64, A, _ = sc.oracle(ROOM, BETAS, sc.SOURCES_5[:4], caps, Y_LEN, float(sc.SR))
        first[alias] = np.array(np.asarray(t))
        assert_rows(first[alias], y64, A, ln_env, 1203, M, F, STATE_TAIL["seed"], 0, cid0, f"state {alias}")
    a, b = first["mic000"][:2, :, M + F:], first["mic001"][:, :, M + F:]
    assert np.all(a != b), "two microphones of one state share their tail noise"
    # the JSON round trip regenerates the same bits
    d = json.loads(json.dumps(st.to_dict()))
    assert d["shoebox"]["tail"] == STATE_TAIL
    again = core.ShoeboxIRState.from_dict(d, renderer=r)
    assert again.tail == st.tail
    again.simulate()
    for alias in first:
        assert np.array_equal(bits(np.asarray(again.irs[alias])), bits(first[alias])), alias
    # a dictionary without the key loads as before: no tail, the bits of the plain entry
    del d["shoebox"]["tail"]
    plain = core.ShoeboxIRState.from_dict(d, renderer=r)
    assert plain.tail is None and "tail" not in plain.to_dict()["shoebox"]
    short = core.ShoeboxIRState(ROOM, betas=BETAS, ir_len=300, sample_rate=sc.SR, max_order=2, renderer=r)
    short.add_microphone("mic000", MIC_A)
    short.add_emitters(sc.SOURCES_5[:2])
    short.simulate()
    want = sc.run_abi(r, ROOM, BETAS, sc.SOURCES_5[:2], MIC_A, 300, sc.SR, max_order=2)
    assert np.array_equal(bits(np.asarray(short.irs["mic000"])), bits(want[:, :, :300]))
    # the rt60 model through the Python layer
    by_rate = _tail_state(r, tail=shoebox.ShoeboxTail(mix_time=0.02, fade_time=0.005, rt60=0.25, seed=9), ir_len=900)
    by_rate.simulate()
    ln_rate = shoebox.tail_envelope(ROOM, BETAS, 900, sc.SR, M, rt60=0.25)
    y64, A, _ = sc.oracle(ROOM, BETAS, sc.SOURCES_5[:4], MIC_B, Y_LEN, float(sc.SR))
    assert_rows(np.asarray(by_rate.irs["mic001"]), y64, A, ln_rate, 900, M, F, 9, 0, 3, "state rt60 model")


def _scene_state(r):
    st = core.ShoeboxIRState(ROOM, betas=(0.8, 0.9, 0.75, 0.85, 0.6, 0.7), ir_len=1203, sample_rate=sc.SR, renderer=r,
                             tail=shoebox.ShoeboxTail(mix_time=0.015, fade_time=0.004, seed=77))
    st.add_microphone("mic000", np.array([[2.0, 1.6, 1.2], [2.05, 1.6, 1.2], [2.0, 1.65, 1.2], [2.0, 1.6, 1.25]]))
    st.add_emitters([[0.8, 0.9, 1.0]], alias="static")
    st.add_emitters(np.linspace([3.2, 0.6, 1.5], [3.4, 2.8, 1.1], 3), alias="moving")
    return st


def run_end_to_end(r, monkeypatch, tmp_path):
    """shoebox_cases.run_end_to_end with a tail and no order limit: the scene renders with every host-to-device path of an IR tensor
    patched to raise, equals the same scene on StaticIRState(np.asarray(tensor)) bit for bit, and renders again from its JSON."""
    state = _scene_state(r)
    scene = sc._add_events(core.Scene(1.2, state, sample_rate=sc.SR))

    def refuse(*a, **k):
        raise AssertionError("an IR tensor went through the host")

    real_upload = engine.Renderer.upload_irs
    monkeypatch.setattr(engine.Renderer, "upload_irs", refuse)
    got = scene.generate()
    got = {k: np.array(v) for k, v in got.items()}
    tensor = state.irs["mic000"]
    assert tensor._host is None, "the render downloaded the IR tensor"
    path = tmp_path / "shoebox_tail_scene.json"
    scene.to_json(str(path))
    assert json.loads(path.read_text())["state"]["shoebox"]["tail"]["seed"] == 77
    clips = {a: e._raw for a, e in scene.events.items()}
    again = core.Scene.from_json(str(path), clips)
    assert isinstance(again.state, core.ShoeboxIRState) and again.state.tail == state.tail
    again.state.renderer = r
    got_again = sc._render(again)
    monkeypatch.setattr(engine.Renderer, "upload_irs", real_upload)

    host = np.asarray(tensor)
    assert np.all(host[:, :, 400:] != 0.0), "the rows have no tail"
    want = sc._render(sc._add_events(core.Scene(1.2, core.StaticIRState({"mic000": host}), sample_rate=sc.SR)))
    assert want["mic000"].shape == (4, round(1.2 * sc.SR)) and np.abs(want["mic000"]).max() > 0
    assert np.array_equal(bits(got["mic000"]), bits(want["mic000"]))
    assert np.array_equal(bits(got_again["mic000"]), bits(want["mic000"]))
    assert np.array_equal(bits(np.asarray(again.state.irs["mic000"])), bits(host))


def run_batch_driver(r, monkeypatch):
    """shoebox_cases.run_batch_driver with a tail: the pipelined driver stages the tensor without a copy or an H2D byte."""
    state = _scene_state(r)
    scene = sc._add_events(core.Scene(1.2, state, sample_rate=sc.SR))
    state.simulate()
    tensor = state.irs["mic000"]
    host_jobs = batch.scene_jobs(sc._add_events(core.Scene(1.2, core.StaticIRState({"mic000": np.asarray(tensor)}), sample_rate=sc.SR)),
                                 "h", renderer=r)
    jobs = batch.scene_jobs(scene, "d", renderer=r)
    real = engine.Renderer.upload_irs
    monkeypatch.setattr(engine.Renderer, "upload_irs", lambda *a, **k: (_ for _ in ()).throw(AssertionError("IR tensor uploaded")))
    got, want = {}, {}
    drv = batch.BatchDriver(r)
    rep = drv.run(jobs, on_scene=got.__setitem__)
    monkeypatch.setattr(engine.Renderer, "upload_irs", real)
    rep_host = drv.run(host_jobs, on_scene=want.__setitem__)
    assert rep_host.h2d_bytes - rep.h2d_bytes == tensor.nbytes and rep.h2d_bytes > 0
    assert np.array_equal(bits(got["d/mic000"]), bits(want["h/mic000"]))
