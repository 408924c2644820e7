"""Scenarios of the coherent diffuse tail of the device shoebox IR generator (al_ism_shoebox_coherent, shoebox.ShoeboxTail(coherent=True),
shoebox.diffuse_directions, shoebox.coherent_tail_tables) and the float64 numpy restatement of its definition (DESIGN.md "Shoebox IRs:
the coherent tail"; no reference code computes this).  tests/test_hostemu_shoebox_coherent.py runs them on the host-emulated kernels,
tests/test_gpu_shoebox_coherent.py on the gfx950 build.

THE DEFINITION.  Everything of shoebox_tail_cases and shoebox_source_cases stands but g(t).  With P plane waves, J taps, the tables
taps (rows, P, J) float64 and delays (rows, P) int32 (-256 <= D, D + J - 1 <= 256) and a group id:
    g(t) = sum_{p < P} sum_{j < J} taps[c, p, j] s_{n,p}(t - delays[c, p] - j)         row c, source n,
float64, p ascending outside, j ascending inside, one fma per term.  s_{n,p}(m) is normal m & 3 of the Philox-4x32-10 block with
counter ((uint32)(m >> 2), source_id0 + n, 5 + 256 p, group_id) under key (seed lo, seed hi), the shift arithmetic (a negative m
wraps), the normal a float32 Box-Muller as noise_draw_cases restates it.

THE BOUND (derived, not tuned), every sample, none excluded.  With h64 the restatement and s64 the float64 draws:
    |h - h64| <= w_e 2^-30 A[t]
               + w_l e(t) ( sum_{p,j} |taps| (RTOL |s64| + ATOL) + P J 2^-52 sum_{p,j} |taps s64| )
               + 2^-24 |h64| + 2^-150
the tail's bound with the draw tolerance of noise_draw_cases carried through the taps, and the float64 accumulation of P J terms.
"""
import ctypes as ct
import json

import numpy as np
import pytest

from audiblelight_amd import core, engine, shoebox
from oracle import synth_oracle as orc
from tests import noise_draw_cases as nd
from tests import shoebox_cases as sc
from tests import shoebox_source_cases as src
from tests import shoebox_tail_cases as tc

TAG = 5
FS = 16000.0
ROOM = tc.ROOM
BETAS = tc.BETAS
SEED = tc.SEED
Y_LEN = 520                      # the image oracle is computed once per receiver kind to this length: every scenario has M + F <= 513
REACH = 256
bits = sc.bits
WORST = {"fraction": 0.0}
SOURCES = sc.SOURCES_5[:2]
SPATS_2 = src.SPATS_5[3:5]       # the oblique cardioid and alpha = 0.25


# ----------------------------------------------------------------------------- the restatement
def philox(c0, c1, c2, c3, seed):
    """Philox-4x32-10 of the counters (c0 an array of uint32 values, the others numbers) under the 64-bit seed: (len(c0), 4) uint64
    words below 2^32."""
    mask = np.uint64(0xFFFFFFFF)
    c0 = np.asarray(c0, dtype=np.uint64) & mask
    c = [c0, np.full_like(c0, c1 & 0xFFFFFFFF), np.full_like(c0, c2 & 0xFFFFFFFF), np.full_like(c0, c3 & 0xFFFFFFFF)]
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack(c, axis=1)


def sequence(seed, sid, p, gid, lo, hi):
    """s_{n,p}(m) for m in [lo, hi), float64 (the Box-Muller of noise_draw_cases._block): lo may be negative."""
    q_lo, q_hi = lo >> 2, (hi + 3) >> 2
    x = philox(np.arange(q_lo, q_hi, dtype=np.int64) & 0xFFFFFFFF, sid, TAG + 256 * p, gid, seed)
    out = np.empty((len(x), 4))
    for h in range(2):
        u1 = (x[:, 2 * h].astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -32)
        u2 = x[:, 2 * h + 1].astype(np.float32) * np.float32(2.0 ** -32)
        rad = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
        out[:, 2 * h], out[:, 2 * h + 1] = rad * np.cos(2 * np.pi * u2.astype(np.float64)), rad * np.sin(2 * np.pi * u2.astype(np.float64))
    return out.reshape(-1)[lo - 4 * q_lo: hi - 4 * q_lo]


def restated_g(taps, delays, seed, sid, gid, n):
    """(g64, draw, accum) of one row for t in [0, n): the sum, sum |taps| (RTOL |s| + ATOL) and sum |taps s|; taps (P, J), delays (P,)."""
    P, J = taps.shape
    g, draw, accum = np.zeros(n), np.zeros(n), np.zeros(n)
    t = np.arange(n)
    for p in range(P):
        s = sequence(seed, sid, p, gid, -REACH, n + REACH)
        for j in range(J):
            x = s[t - int(delays[p]) - j + REACH]
            g += taps[p, j] * x
            draw += abs(taps[p, j]) * (nd.RTOL * np.abs(x) + nd.ATOL)
            accum += np.abs(taps[p, j] * x)
    return g, draw, accum


def restate(y64, A, ln_env, ir_len, M, F, taps, delays, seed, sid, gid):
    """(h64, bound) of one row; y64 and A need to reach min(ir_len, M + F) only."""
    w_e, w_l = tc.weights(ir_len, M, F)
    y, a = np.zeros(ir_len), np.zeros(ir_len)
    m = min(ir_len, len(y64))
    assert m >= min(ir_len, M + F)
    y[:m], a[:m] = y64[:m], A[:m]
    e = tc.envelope(ln_env, ir_len)
    g, draw, accum = restated_g(taps, delays, seed, sid, gid, ir_len)
    noise = np.where(w_l > 0.0, w_l * e * g, 0.0)
    h = w_e * y + noise
    PJ = taps.shape[0] * taps.shape[1]
    bound = (w_e * 2.0 ** -30 * a + np.where(w_l > 0.0, w_l * e * (draw + PJ * 2.0 ** -52 * accum), 0.0) + 2.0 ** -24 * np.abs(h)
             + 2.0 ** -150)
    return h, bound


def assert_rows(rows, y64, A, ln_env, ir_len, M, F, taps, delays, seed, sid0, gid, what):
    """rows (C, N, pitch) against the restatement; ln_env (C, N, n_knots)."""
    C, N = rows.shape[:2]
    assert np.all(bits(rows[:, :, ir_len:]) == 0), (what, "pad samples must be +0")
    worst = 0.0
    for ci in range(C):
        for ni in range(N):
            h, bound = restate(y64[ci, ni], A[ci, ni], ln_env[ci, ni], ir_len, M, F, taps[ci], delays[ci], seed, sid0 + ni, gid)
            assert np.all(np.isfinite(rows[ci, ni])), what
            err = np.abs(rows[ci, ni, :ir_len].astype(np.float64) - h)
            frac = float((err / bound).max())
            worst = max(worst, frac)
            assert np.all(err <= bound), (what, (ci, ni), "sample", int(np.argmax(err / bound)), "err / bound", frac)
    WORST["fraction"] = max(WORST["fraction"], worst)
    print(f"shoebox coherent bound [{what}]: max err / bound {worst:.3f} (so far {WORST['fraction']:.3f})")


# ----------------------------------------------------------------------------- running the entry point
def run_coherent(r, sources, spats, positions, rpats, air, ir_len, M, F, ln_env, taps, delays, gid=0, seed=SEED, sid0=0, cid0=0,
                 max_order=None, pitch=None, room=ROOM, betas=BETAS, fs=FS, c=sc.C_SOUND):
    """al_ism_shoebox_coherent into a buffer with sc.GUARD sentinels on either side: the (P K, N, pitch) rows, the guards checked.
    ln_env (rows, N, n_knots), taps (rows, P, J), delays (rows, P)."""
    mem, lib = r.mem, r.lib
    sources = np.ascontiguousarray(np.atleast_2d(sources), dtype=np.float64)
    positions = np.ascontiguousarray(np.atleast_2d(positions), dtype=np.float64)
    n, n_pos = len(sources), len(positions)
    K = 1 if rpats is None else np.asarray(rpats).shape[1]
    rows = n_pos * K
    pitch = shoebox.pitch_of(ir_len) if pitch is None else pitch
    total = rows * n * pitch
    taps = np.ascontiguousarray(taps, dtype=np.float64)
    delays = np.ascontiguousarray(delays, dtype=np.int32)
    assert taps.shape[:2] == delays.shape == (rows, taps.shape[1]) and np.shape(ln_env) == (rows, n, shoebox.n_knots_of(ir_len))
    assert delays.min() >= -REACH and delays.max() + taps.shape[2] - 1 <= REACH, "the tables' contract"
    out = src._guarded(mem, total)
    src_dev, pos_dev, spat_dev, pat_dev = src._dev(mem, sources), src._dev(mem, positions), src._dev(mem, spats), src._dev(mem, rpats)
    env_dev, taps_dev, delays_dev = src._dev(mem, ln_env), src._dev(mem, taps), mem.upload(delays.reshape(-1))
    L, beta = (ct.c_double * 3)(*room), (ct.c_double * 6)(*betas)
    lib.call("al_ism_shoebox_coherent", mem.ptr(src_dev), n, src._ptr(mem, spat_dev), mem.ptr(pos_dev), n_pos, src._ptr(mem, pat_dev), K, L,
             beta, float(air), float(c), float(fs), -1 if max_order is None else int(max_order), int(ir_len), int(pitch), int(M), int(F),
             int(seed), int(sid0), int(cid0), mem.ptr(env_dev), np.shape(ln_env)[2], mem.ptr(taps_dev), mem.ptr(delays_dev), taps.shape[1],
             taps.shape[2], int(gid), mem.ptr(out) + 4 * sc.GUARD, mem.stream())
    return src._unguard(mem, out, total, (rows, n, pitch))


def receivers(kind):
    """(positions, rpats) of a configuration: three omni capsules, two points with one cardioid each (K = 1), one FOA point (K = 4)."""
    if kind == "omni3":
        return sc.CAPSULES_3, None
    if kind == "k1":
        return sc.CAPSULES_3[:2], np.stack([shoebox.cardioid((1.0, 0.2, -0.3)), shoebox.first_order(0.25, (0.0, 1.0, 1.0))])[:, None, :]
    assert kind == "foa"
    return sc.CAPSULES_3[:1], shoebox.foa_patterns()[None, :, :]


def random_tables(rng, rows, P, J):
    """Seeded random tables with Var g about 1: the entry takes any table.  The delays cover the whole range and hold both of its
    ends and 0."""
    taps = rng.standard_normal((rows, P, J)) / np.sqrt(P * J)
    delays = rng.integers(-REACH, REACH - (J - 1) + 1, (rows, P)).astype(np.int32)
    flat = delays.reshape(-1)
    flat[0], flat[-1], flat[len(flat) // 2] = -REACH, REACH - (J - 1), 0
    return taps, delays


def jagged_env(rng, rows, n, ir_len):
    """Knots that do not lie on a line, one table per (row, source)."""
    return rng.uniform(-9.0, -2.0, (rows, n, shoebox.n_knots_of(ir_len)))


def _cfg(P=7, J=2, M=100, F=50, ir_len=1100, kind="omni3", pitch=None, sid0=0, cid0=0, gid=0, source=False, order=1, tables="random"):
    return (P, J, M, F, ir_len, kind, pitch, sid0, cid0, gid, source, order, tables)


PARITY = (
    [_cfg(P=P, J=8) for P in (1, 2, 7, 64, 256)]
    + [_cfg(J=J) for J in (1, 2, 32)] + [_cfg(P=256, J=32, ir_len=600)]
    + [_cfg(M=155 + d, F=100) for d in (0, 1, 2)]                       # M + F = 255, 256, 257: the split on either side of a tile edge
    + [_cfg(M=0, F=1), _cfg(M=300, F=1000, ir_len=500)]                 # noise from sample 1 on (m < 0 there); a fade cut by the row end
    + [_cfg(M=0, F=1, ir_len=1), _cfg(ir_len=257), _cfg(ir_len=256 + 1024 + 5), _cfg(J=8, ir_len=1400, order=None)]   # two workgroups of k_ism_ctail
    + [_cfg(pitch=1400), _cfg(ir_len=513, M=400, F=100, pitch=1024 + 512 + 8)]
    + [_cfg(sid0=0xFFFFFFF0, cid0=9, gid=0xFFFFFFFF), _cfg(kind="k1", gid=3), _cfg(P=64, J=8, kind="foa", gid=1)]
    + [_cfg(kind="omni3", source=True, gid=7), _cfg(kind="foa", source=True, order=None)]
    + [_cfg(P=64, J=8, kind="omni3", tables="model"), _cfg(P=64, J=8, kind="foa", tables="model")]
)


def run_parity(r, P, J, M, F, ir_len, kind, pitch, sid0, cid0, gid, source, order, tables):
    positions, rpats = receivers(kind)
    spats, air = (SPATS_2, src.AIR) if source else (None, 0.0)
    y64, A, _ = src.oracle(ROOM, BETAS, air, SOURCES, spats, positions, rpats, Y_LEN, FS, max_order=order)
    rows = y64.shape[0]
    rng = np.random.default_rng([P, J, rows])
    if tables == "random":
        taps, delays = random_tables(rng, rows, P, J)
    else:
        K = 1 if rpats is None else rpats.shape[1]
        taps, delays = shoebox.coherent_tail_tables(np.repeat(positions, K, axis=0), None if rpats is None else rpats.reshape(-1, 4), None,
                                                    FS, sc.C_SOUND, P, J // 2)
    ln_env = jagged_env(rng, rows, len(SOURCES), ir_len)
    got = run_coherent(r, SOURCES, spats, positions, rpats, air, ir_len, M, F, ln_env, taps, delays, gid, sid0=sid0, cid0=cid0,
                       max_order=order, pitch=pitch)
    assert_rows(got, y64, A, ln_env, ir_len, M, F, taps, delays, SEED, sid0, gid, (P, J, M, F, ir_len, kind, pitch, source, order, tables))
    if ir_len > M + F:
        assert np.all(got[:, :, M + F: ir_len] != 0.0), "a tail sample is zero"


def run_philox_restatement():
    """The vectorised Philox of this file against the oracle's, negative block numbers included."""
    q = np.array([0, 1, 5, 0xFFFFFFFF, -1 & 0xFFFFFFFF, -64 & 0xFFFFFFFF])
    got = philox(q, 0xFFFFFFF1, TAG + 256 * 255, 0xFFFFFFFF, SEED)
    for i, qi in enumerate(q):
        want = orc.philox4x32_10((int(qi), 0xFFFFFFF1, TAG + 256 * 255, 0xFFFFFFFF), (SEED & 0xFFFFFFFF, SEED >> 32))
        assert tuple(int(v) for v in got[i]) == tuple(int(v) for v in want)
    # tag 5 + 256 * 0 with the group id in the fourth word is the tail's block of capsule `gid` under tag 5
    s = sequence(SEED, 3, 0, 9, -8, 8)
    x = orc.philox4x32_10((0xFFFFFFFE, 3, TAG, 9), (SEED & 0xFFFFFFFF, SEED >> 32))       # m = -8 .. -5: block -2
    u1 = (np.float32(x[0]) + np.float32(0.5)) * np.float32(2.0 ** -32)
    u2 = np.float32(x[1]) * np.float32(2.0 ** -32)
    assert s[0] == float(np.sqrt(-2.0 * np.log(np.float64(u1))) * np.cos(2 * np.pi * np.float64(u2)))


# ----------------------------------------------------------------------------- 2. ties without the restatement
def _tie_setup(rows=3, P=7, J=4, ir_len=2500, seed=11):
    rng = np.random.default_rng(seed)
    taps, delays = random_tables(rng, rows, P, J)
    return taps, delays, jagged_env(rng, rows, len(SOURCES), ir_len)


def run_direct_against_ctail(r):
    """The same rows with M + F at 200 and at 1000: samples 1000 .. 1023 are the direct evaluator's in the second run and k_ism_ctail's
    in the first, and from 1024 on k_ism_ctail's tiles start at another sample.  Bit for bit."""
    ir_len = 2500
    taps, delays, ln_env = _tie_setup(ir_len=ir_len)
    run = lambda M: run_coherent(r, SOURCES, None, sc.CAPSULES_3, None, 0.0, ir_len, M, 50, ln_env, taps, delays, 5, max_order=0)   # noqa: E731
    early, late = run(150), run(950)
    assert np.array_equal(bits(early[:, :, 1000:]), bits(late[:, :, 1000:]))
    assert np.all(early[:, :, 1000:ir_len] != 0.0)
    assert not np.array_equal(bits(early[:, :, 900:1000]), bits(late[:, :, 900:1000]))      # the fades differ


def run_one_wave_is_shared(r):
    """P = 1, J = 1, tap 1, delay 0: g(t) = s(t) for every row, so rows with one knot table are bit-identical past M + F."""
    ir_len, M, F = 1500, 100, 50
    taps, delays = np.ones((3, 1, 1)), np.zeros((3, 1), dtype=np.int32)
    ln_env = np.tile(np.random.default_rng(2).uniform(-9.0, -2.0, shoebox.n_knots_of(ir_len)), (3, 2, 1))
    got = run_coherent(r, SOURCES, None, sc.CAPSULES_3, None, 0.0, ir_len, M, F, ln_env, taps, delays, 2, max_order=1)
    for ci in (1, 2):
        assert np.array_equal(bits(got[ci, :, M + F:]), bits(got[0, :, M + F:]))
    assert not np.array_equal(bits(got[0, 0, M + F:]), bits(got[0, 1, M + F:])), "two sources share a sequence"
    e = tc.envelope(ln_env[0, 0], ir_len)
    s = sequence(SEED, 0, 0, 2, 0, ir_len)
    assert np.all(np.abs(got[0, 0, M + F: ir_len] - e[M + F:] * s[M + F:]) <= e[M + F:] * (nd.RTOL * np.abs(s[M + F:]) + nd.ATOL) * 1.01)


def run_no_tail_is_the_source_entry(r):
    ir_len = 520
    positions, rpats = receivers("k1")
    taps, delays, ln_env = _tie_setup(rows=2, ir_len=ir_len)
    for pitch in (None, 768 + 8):
        want = src.run_src(r, ROOM, BETAS, SOURCES, SPATS_2, positions, rpats, src.AIR, ir_len, FS, max_order=3, pitch=pitch)
        for M, F in ((ir_len, 1), (ir_len + 1000, 7), (1 << 40, 1), (ir_len - 1, 5)):
            got = run_coherent(r, SOURCES, SPATS_2, positions, rpats, src.AIR, ir_len, M, F, ln_env, taps, delays, 1, max_order=3, pitch=pitch)
            assert np.array_equal(bits(got), bits(want)), ("mix >= ir_len differs from al_ism_shoebox_src", M, F, pitch)


def run_row_identity(r):
    """A row's bits depend on its own rows of the tables, source_id0 + n and the group id: alone, among many, at another pitch, twice."""
    ir_len, M, F, sid0, gid = 1400, 100, 50, 7, 3
    taps, delays, ln_env = _tie_setup(ir_len=ir_len)
    run = lambda s, m, t, d, e, **k: run_coherent(r, s, None, m, None, 0.0, ir_len, M, F, e, t, d, **dict(dict(gid=gid, sid0=sid0, max_order=1), **k))   # noqa: E731
    one = run(SOURCES, sc.CAPSULES_3, taps, delays, ln_env)
    assert np.array_equal(bits(one), bits(run(SOURCES, sc.CAPSULES_3, taps, delays, ln_env))), "two runs differ"
    wide = run(SOURCES, sc.CAPSULES_3, taps, delays, ln_env, pitch=1024 + 512 + 4, cid0=77)      # capsule_id0 enters no draw
    assert np.array_equal(bits(wide[:, :, :ir_len]), bits(one[:, :, :ir_len])) and np.all(bits(wide[:, :, ir_len:]) == 0)
    for ci, ni in ((0, 0), (1, 1), (2, 0)):
        sel = (slice(ci, ci + 1), slice(ni, ni + 1))
        alone = run(SOURCES[ni], sc.CAPSULES_3[ci], taps[ci:ci + 1], delays[ci:ci + 1], ln_env[sel], sid0=sid0 + ni)
        assert np.array_equal(bits(alone[0, 0]), bits(one[ci, ni])), (ci, ni)
        for what, other in (("seed", dict(seed=SEED ^ (1 << 32))), ("source id", dict(sid0=sid0 + ni + 1)), ("group id", dict(gid=gid + 1))):
            got = run(SOURCES[ni], sc.CAPSULES_3[ci], taps[ci:ci + 1], delays[ci:ci + 1], ln_env[sel], **dict(dict(sid0=sid0 + ni), **other))
            assert np.array_equal(bits(got[0, 0, :M + 1]), bits(alone[0, 0, :M + 1])), what
            assert np.all(got[0, 0, M + 1: ir_len] != alone[0, 0, M + 1: ir_len]), (what, "left some tail samples as they were")
    # nine rows: two blocks of rows in k_ism_ctail; row 8 alone is row 8 among the nine
    rng = np.random.default_rng(5)
    caps = np.concatenate([sc.CAPSULES_3 + [0.0, 0.1 * i, 0.05 * i] for i in range(3)])
    t9, d9 = random_tables(rng, 9, 7, 4)
    e9 = jagged_env(rng, 9, 1, ir_len)
    nine = run(SOURCES[:1], caps, t9, d9, e9)
    last = run(SOURCES[:1], caps[8], t9[8:], d9[8:], e9[8:])
    assert np.array_equal(bits(last[0]), bits(nine[8]))


def run_one_row_is_todays_tail(r):
    """A call with one row through Python: the bits of today's ShoeboxTail, whatever `coherent` says."""
    kw = dict(room=ROOM, betas=BETAS, sources=SOURCES, capsules=sc.CAPSULES_3[:1], ir_len=900, sample_rate=FS, max_order=1, capsule_id0=4)
    Tail = shoebox.ShoeboxTail
    get = lambda tail: np.asarray(r.mem.download(shoebox.shoebox_irs_device(r, tail=tail, **kw)[0]))[: 2 * 900]      # noqa: E731
    a, b = get(Tail(mix_time=0.01, seed=5)), get(Tail(mix_time=0.01, seed=5, coherent=True))
    assert np.array_equal(bits(a), bits(b)) and np.all(a[400:900] != 0.0)


def run_shake_rows(r):
    """The rows the schedule-perturbed builds repeat: nine rows of a random table, 64 plane waves in chunks, two tiles of k_ism_ctail."""
    rng = np.random.default_rng(8)
    caps = np.concatenate([sc.CAPSULES_3 + [0.0, 0.1 * i, 0.05 * i] for i in range(3)])
    taps, delays = random_tables(rng, 9, 64, 8)
    ln_env = jagged_env(rng, 9, 2, 1500)
    return {"coherent": run_coherent(r, SOURCES, None, caps, None, 0.0, 1500, 100, 50, ln_env, taps, delays, 6, max_order=1)}


# ----------------------------------------------------------------------------- 3. what the numbers mean
DIRECTIONS = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.6, 0.64, 0.48), (2.0 ** -0.5, 2.0 ** -0.5, 0.0), (-0.3, 0.2, 0.93))


def run_directions():
    """diffuse_directions(64): the plane-wave mean of exp(i kd u . e) against sin(kd) / (kd), real by antipody; first and second moments."""
    u = shoebox.diffuse_directions(64)
    assert u.shape == (64, 3) and np.allclose((u * u).sum(axis=1), 1.0, rtol=0, atol=1e-15) and np.array_equal(u[32:], -u[:32])
    kd = np.linspace(0.0, 4.0, 401)
    worst_re = worst_im = 0.0
    for e in DIRECTIONS:
        e = np.asarray(e) / np.sqrt(np.dot(e, e))
        model = np.exp(1j * kd[:, None] * (u @ e)[None, :]).mean(axis=1)
        worst_re = max(worst_re, float(np.abs(model.real - np.sinc(kd / np.pi)).max()))
        worst_im = max(worst_im, float(np.abs(model.imag).max()))
    second = float(np.abs(3.0 / 64.0 * u.T @ u - np.eye(3)).max())
    print(f"diffuse_directions(64): |Re - sinc| <= {worst_re:.4f}, |Im| <= {worst_im:.1e}, |3/P sum u u^T - I| <= {second:.4f}")
    assert worst_re <= 0.02 and worst_im <= 1e-12
    assert np.abs(u.sum(axis=0)).max() <= 1e-12
    assert second <= 0.02
    for bad in (0, 1, 7, 258, 2.0, True):
        with pytest.raises(ValueError):
            shoebox.diffuse_directions(bad)


def run_table_properties():
    """coherent_tail_tables: shapes, Var g = 1 per row, the delays of a capsule on either side of the origin, the centroid default."""
    pos = np.array([[2.0, 1.6, 1.2], [2.1, 1.63, 1.22]])
    taps, delays = shoebox.coherent_tail_tables(pos, None, pos[0], FS, sc.C_SOUND, 32, 4)
    assert taps.shape == (2, 32, 8) and taps.dtype == np.float64 and delays.shape == (2, 32) and delays.dtype == np.int32
    assert np.allclose((taps * taps).sum(axis=(1, 2)), 1.0, rtol=0, atol=1e-14)
    # delta = 0: one tap, at j = H - 1 (numpy's sinc is 4e-17 and not 0 at the other integers)
    assert np.all(delays[0] == -3) and np.allclose(taps[0, :, 3], 32 ** -0.5, rtol=0, atol=1e-15) and np.abs(np.delete(taps[0], 3, axis=1)).max() < 1e-16
    u = shoebox.diffuse_directions(32)
    delta = -((pos[1] - pos[0]) @ u.T) * FS / sc.C_SOUND
    assert np.array_equal(delays[1], np.floor(delta).astype(np.int32) - 3)
    centre = shoebox.coherent_tail_tables(pos, None, None, FS, sc.C_SOUND, 32, 4)
    mid = shoebox.coherent_tail_tables(pos, None, pos.mean(axis=0), FS, sc.C_SOUND, 32, 4)
    assert np.array_equal(centre[0], mid[0]) and np.array_equal(centre[1], mid[1])
    foa = shoebox.coherent_tail_tables(np.repeat(pos[:1], 4, axis=0), shoebox.foa_patterns(), None, FS, sc.C_SOUND, 64, 4)[0]
    assert np.allclose((foa * foa).sum(axis=(1, 2)), 1.0, rtol=0, atol=1e-14)
    lag0 = np.einsum("pj,cpj->c", foa[0], foa[1:])      # W against Y, Z, X at lag 0: the first moment of the directions
    assert np.abs(lag0).max() <= 0.02


def predicted_xcorr(taps_a, delays_a, taps_b, delays_b, lags):
    """E[g_a(t) g_b(t + l)]: the sum over p, j, j' with D_a + j = D_b + j' - l of taps_a taps_b."""
    J = taps_a.shape[1]
    out = np.zeros(len(lags))
    for i, lag in enumerate(lags):
        for p in range(len(taps_a)):
            for j in range(J):
                jb = int(delays_a[p]) + j - int(delays_b[p]) + lag
                if 0 <= jb < J:
                    out[i] += taps_a[p, j] * taps_b[p, jb]
    return out


XCORR_N = 16384
XCORR_OFFSET = np.array([0.1, 0.03, 0.02])
XCORR_SEED = 20241


def sample_xcorr(a, b, lags):
    n = len(a)
    return np.array([np.dot(a[max(0, -l): n - max(0, l)], b[max(0, l): n - max(0, -l)]) / n for l in lags])


def run_pair_xcorr(r):
    """Two omnis at a point and (0.1, 0.03, 0.02) from it, 16 kHz, 32 plane waves, half_taps 4, a flat envelope (all knots 0), M = 0:
    the sample cross-correlation of XCORR_N samples past the fade at lags -8 .. 8 lies within 5 / sqrt(N) of what the tables predict
    (a curve that peaks at 0.179), and the same rows under the independent tail stay below 5 / sqrt(N) at every lag.  XCORR_SEED was
    fixed after the statistic was checked on the CPU emulation (worst deviation 2.35 / sqrt(N) there, 1.82 / sqrt(N) for the independent
    rows): the draws are a function of the seed."""
    pos = np.stack([sc.CAPSULES_3[0], sc.CAPSULES_3[0] + XCORR_OFFSET])
    taps, delays = shoebox.coherent_tail_tables(pos, None, None, FS, sc.C_SOUND, 32, 4)
    ir_len, lags = XCORR_N + 4, np.arange(-8, 9)
    ln_env = np.zeros((2, 1, shoebox.n_knots_of(ir_len)))
    got = run_coherent(r, SOURCES[:1], None, pos, None, 0.0, ir_len, 0, 1, ln_env, taps, delays, 0, seed=XCORR_SEED, max_order=0)
    a, b = got[0, 0, 4:ir_len].astype(np.float64), got[1, 0, 4:ir_len].astype(np.float64)
    want = predicted_xcorr(taps[0], delays[0], taps[1], delays[1], lags)
    dev = np.abs(sample_xcorr(a, b, lags) - want) * np.sqrt(XCORR_N)
    print(f"coherent pair: predicted xcorr peaks at {np.abs(want).max():.3f}; worst deviation {dev.max():.2f} / sqrt(N); "
          f"variances {a.var():.3f}, {b.var():.3f}")
    assert 0.1 < np.abs(want).max() < 0.3
    assert dev.max() <= 5.0
    assert abs(a.var() - 1.0) <= 5.0 * np.sqrt(2.0 / XCORR_N) * 3 and abs(b.var() - 1.0) <= 5.0 * np.sqrt(2.0 / XCORR_N) * 3
    ind = src.run_src(r, ROOM, BETAS, SOURCES[:1], None, pos, None, 0.0, ir_len, FS, max_order=0,
                      tail=dict(M=0, F=1, ln_env=ln_env, seed=XCORR_SEED))
    ia, ib = ind[0, 0, 4:ir_len].astype(np.float64), ind[1, 0, 4:ir_len].astype(np.float64)
    ind_dev = np.abs(sample_xcorr(ia, ib, lags)) * np.sqrt(XCORR_N)
    print(f"independent pair: worst |xcorr| {ind_dev.max():.2f} / sqrt(N)")
    assert ind_dev.max() <= 5.0


PAIR_POINT = np.array([2.0, 1.6, 1.2])
PAIR_TAIL = dict(mix_time=0.02, fade_time=0.005, seed=4242)      # M + F = 400 at 16 kHz: the late window (80 ms past the onset) is all tail


def _late(st, pm, rows):
    """(start of the late window, its effective length N_eff = (sum w)^2 / sum w^2 with w the product of the two rows' envelopes)."""
    start = int(pm.t0[0, 0]) + int(round(0.08 * st.sample_rate))
    M, _ = shoebox.tail_samples(st.tail, st.room, st.sample_rate, st.c)
    w = np.prod([tc.envelope(shoebox.tail_envelope(st.room, st.betas, st.ir_len, float(st.sample_rate), M, st.c, pattern=row), st.ir_len)[start:]
                 for row in rows], axis=0)
    return start, float(w.sum() ** 2 / (w * w).sum())


def run_state_pair_metrics(r):
    """Two omnis 2 cm apart at 16 kHz, ir_len 3000, measured by pair_metrics(): peak_l of the late window lies within 5 / sqrt(N_eff) of
    the peak of the curve the tables predict, N_eff = (sum e^2)^2 / sum e^4 over the late window; with coherent=False it stays below
    0.25.  c / (2 d) lies above the Nyquist frequency, so sin(kd) / (kd) averaged over the band is 0.63; the tables of half_taps = 4
    predict 0.761 (0.696 with 8, 0.663 with 16: the short interpolation kernel rolls off below the Nyquist frequency, where the
    coherence is lowest).  The seed was fixed after the figures were seen on the CPU emulation (0.775 against 0.761, 0.064 for the
    independent tail, 5 / sqrt(N_eff) = 0.164)."""
    pos = np.stack([PAIR_POINT, PAIR_POINT + [0.02, 0.0, 0.0]])
    got = {}
    for coherent in (True, False):
        st = core.ShoeboxIRState(ROOM, betas=BETAS, ir_len=3000, sample_rate=sc.SR, renderer=r, tail=shoebox.ShoeboxTail(coherent=coherent, **PAIR_TAIL))
        st.add_microphone("pair", pos)
        st.add_emitters(SOURCES[:1])
        st.simulate()
        pm = st.pair_metrics(max_lag=8)["pair"]
        got[coherent] = float(pm.peak_l[0, 0])
    start, n_eff = _late(st, pm, [None, None])
    taps, delays = shoebox.coherent_tail_tables(pos, None, None, float(sc.SR), st.c, 64, 4)
    curve = predicted_xcorr(taps[0], delays[0], taps[1], delays[1], np.arange(-8, 9))
    want = float(curve[np.argmax(np.abs(curve))])
    print(f"state pair at 2 cm: peak_l {got[True]:.3f} (tables: {want:.3f}), independent tail {got[False]:.3f}; late window from {start}, "
          f"N_eff {n_eff:.0f}, 5 / sqrt(N_eff) = {5.0 / np.sqrt(n_eff):.3f}")
    assert abs(want - 0.761) < 0.001      # the figure DESIGN.md quotes
    assert abs(got[True] - want) <= 5.0 / np.sqrt(n_eff)
    assert abs(got[False]) < 0.25


def run_foa_lag0(r):
    """One FOA point: the late-window correlation at lag 0 between W and each of Y, Z, X.  The tables predict |.| <= 0.02 (the first
    moment of the directions); the measured value lies within 5 / sqrt(N_eff) of the prediction."""
    st = core.ShoeboxIRState(ROOM, betas=BETAS, ir_len=3000, sample_rate=sc.SR, renderer=r, tail=shoebox.ShoeboxTail(coherent=True, **PAIR_TAIL))
    st.add_foa_listener("foa", PAIR_POINT)
    st.add_emitters(SOURCES[:1])
    st.simulate()
    pairs = np.array([[0, 1], [0, 2], [0, 3]])
    pm = st.pair_metrics(pairs=pairs, max_lag=0)["foa"]
    foa = shoebox.foa_patterns()
    taps, delays = shoebox.coherent_tail_tables(np.repeat(PAIR_POINT[None, :], 4, axis=0), foa, None, float(sc.SR), st.c, 64, 4)
    for i, (a, b) in enumerate(pairs):
        want = predicted_xcorr(taps[a], delays[a], taps[b], delays[b], [0])[0]
        _, n_eff = _late(st, pm, [foa[a], foa[b]])
        print(f"FOA W against channel {b}: late peak at lag 0 {pm.peak_l[i, 0]:+.3f} (tables: {want:+.4f}), 5 / sqrt(N_eff) = {5.0 / np.sqrt(n_eff):.3f}")
        assert abs(want) <= 0.02
        assert abs(pm.peak_l[i, 0] - want) <= 5.0 / np.sqrt(n_eff)


# ----------------------------------------------------------------------------- 4. refusals and plumbing
def run_abi_refusals(r):
    mem, lib = r.mem, r.lib
    s, m = mem.upload(np.array([1.0, 1.0, 1.0])), mem.upload(np.array([2.0, 1.5, 1.2, 2.1, 1.5, 1.2]))
    out = mem.upload(np.full(128, sc.SENTINEL, dtype=np.float32))
    env, taps, delays = mem.upload(np.full(4, -3.0)), mem.upload(np.full(2 * 2 * 2, 0.5)), mem.upload(np.zeros(4, dtype=np.int32))
    good = dict(sources=mem.ptr(s), n=1, spat=None, receivers=mem.ptr(m), n_rec=2, pat=None, K=1, L=(3.0, 2.5, 2.0), beta=(0.5,) * 6, air=0.0,
                c=343.0, fs=16000.0, order=-1, ir_len=30, pitch=32, mix=10, fade=5, seed=1, sid0=0, cid0=0, env=mem.ptr(env), n_knots=2,
                taps=mem.ptr(taps), delays=mem.ptr(delays), P=2, J=2, gid=0, out=mem.ptr(out))

    def call(**change):
        a = dict(good, **change)
        L = None if a["L"] is None else (ct.c_double * 3)(*a["L"])
        beta = None if a["beta"] is None else (ct.c_double * 6)(*a["beta"])
        return lib.call("al_ism_shoebox_coherent", a["sources"], a["n"], a["spat"], a["receivers"], a["n_rec"], a["pat"], a["K"], L, beta,
                        a["air"], a["c"], a["fs"], a["order"], a["ir_len"], a["pitch"], a["mix"], a["fade"], a["seed"], a["sid0"], a["cid0"],
                        a["env"], a["n_knots"], a["taps"], a["delays"], a["P"], a["J"], a["gid"], a["out"], mem.stream())

    old = [(dict(L=(0.0, 2.5, 2.0)), "al_ism_shoebox: "), (dict(c=float("nan")), "al_ism_shoebox: "), (dict(beta=(0.5,) * 5 + (1.01,)), "al_ism_shoebox: "),
           (dict(n=0), "al_ism_shoebox: "), (dict(ir_len=0), "al_ism_shoebox: "), (dict(pitch=34, ir_len=33), "al_ism_shoebox: "),
           (dict(order=-2), "al_ism_shoebox: "), (dict(sources=None), "null pointer"), (dict(out=None), "null pointer"),
           (dict(air=-1.0), "air must be finite"), (dict(air=float("inf")), "air must be finite"), (dict(K=2), "n_channels == 1"),
           (dict(K=0), "n_channels"), (dict(fade=0), "fade must be >= 1"), (dict(sid0=-1), "must be >= 0"), (dict(cid0=1 << 32), "must not exceed 2^32"),
           (dict(n_knots=3), "n_knots must be"), (dict(env=None), "null envelope table"), (dict(out=mem.ptr(out) + 4), "16-byte aligned")]
    new = [(dict(mix=-1), "mix must be >= 0"), (dict(P=0), "n_waves must be in 1 .. 256"), (dict(P=257), "n_waves must be in 1 .. 256"),
           (dict(J=0), "n_taps must be in 1 .. 32"), (dict(J=33), "n_taps must be in 1 .. 32"), (dict(taps=None), "null tap or delay table"),
           (dict(delays=None), "null tap or delay table"), (dict(gid=-1), "group_id must be in [0, 2^32)"),
           (dict(gid=1 << 32), "group_id must be in [0, 2^32)")]
    for change, needle in old + new:
        nd.raises_badarg(lambda: call(**change), "al_ism_shoebox_coherent failed", needle)
    for change, needle in new:
        nd.raises_badarg(lambda: call(**change), "al_ism_shoebox_coherent: ", needle)
    assert np.all(np.asarray(mem.download(out)) == sc.SENTINEL), "a refused call wrote"
    assert call() == 0
    assert call(gid=(1 << 32) - 1, sid0=(1 << 32) - 1, seed=(1 << 64) - 1, mix=0, fade=1) == 0
    assert r.lib.call("al_abi_version") == 6


def run_python_errors(r, monkeypatch):
    """Every ValueError of the Python layer, raised before anything is uploaded."""
    Tail = shoebox.ShoeboxTail
    room, s = (3.0, 2.5, 2.0), [[1.0, 1.0, 1.0]]
    m = [[2.0, 1.5, 1.2], [2.05, 1.5, 1.2]]
    ok = dict(room=room, betas=(0.5,) * 6, sources=s, capsules=m, ir_len=600, sample_rate=16000, tail=Tail(seed=5, coherent=True))
    real = r.mem.upload
    monkeypatch.setattr(r.mem, "upload", lambda *a, **k: (_ for _ in ()).throw(AssertionError("uploaded before the check")))
    bad = [dict(tail=Tail(coherent=True, n_waves=63)), dict(tail=Tail(coherent=True, n_waves=0)), dict(tail=Tail(coherent=True, n_waves=258)),
           dict(tail=Tail(coherent=True, n_waves=64.0)), dict(tail=Tail(coherent=True, half_taps=0)), dict(tail=Tail(coherent=True, half_taps=17)),
           dict(tail=Tail(coherent=True, half_taps=True)), dict(tail=Tail(coherent=1)), dict(tail=Tail(n_waves=3)),
           dict(capsules=[[0.2, 0.2, 0.2], [2.9, 2.4, 1.9]], sample_rate=48000),                 # 4 m apart at 48 kHz: 580 samples
           dict(patterns=np.array([[[0.0, 1.0, 0.0, 0.0]], [[0.0, 0.0, 0.0, 1e-300]]]), tail=Tail(coherent=True, n_waves=2)),
           dict(origin=(0.0, 0.0)), dict(origin=(float("nan"), 0.0, 0.0))]
    for change in bad:
        with pytest.raises(ValueError):
            shoebox.shoebox_irs_device(r, **dict(ok, **change))
    with pytest.raises(ValueError, match="array within .* m of its origin at this sample rate"):
        shoebox.shoebox_irs_device(r, **dict(ok, capsules=[[0.2, 0.2, 0.2], [2.9, 2.4, 1.9]], sample_rate=48000))
    with pytest.raises(ValueError, match="not yet"):
        shoebox.shoebox_irs_device(r, **dict(ok, betas=np.full((6, 2), 0.5), bands=shoebox.ShoeboxBands(centres=(500.0, 2000.0), half=64)))
    with pytest.raises(ValueError, match="not yet"):
        shoebox.shoebox_sphere_irs_device(r, room, (0.5,) * 6, s, (2.0, 1.5, 1.2), [[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]], 0.05, 600, 16000,
                                          tail=Tail(coherent=True))
    # (above: the two directions of P = 2 lie in the xy plane, so a z dipole hears neither)  a pattern that hears no plane wave has no tail
    with pytest.raises(ValueError, match="zero towards every plane wave"):
        shoebox.coherent_tail_tables(np.zeros((1, 3)), np.array([[0.0, 0.0, 0.0, 0.0]]), None, 16000.0, 343.0, 2, 1)
    for change in (dict(tail=Tail(coherent=True, n_waves=5)), dict(tail=dict(coherent=True, half_taps=40))):
        with pytest.raises(ValueError):
            core.ShoeboxIRState(**dict(dict(room=room, betas=(0.5,) * 6), **change))
    st = core.ShoeboxIRState(room, betas=(0.5,) * 6, tail=Tail(coherent=True))
    with pytest.raises(ValueError, match="not yet"):
        st.add_sphere_microphone("ball", (2.0, 1.5, 1.2), [[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]], 0.05)
    monkeypatch.setattr(r.mem, "upload", real)
    buf, strides, n = shoebox.shoebox_irs_device(r, **ok)
    assert strides == (600, 600) and n == 600


def run_tail_dictionaries():
    Tail = shoebox.ShoeboxTail
    assert Tail(seed=3).to_dict() == dict(mix_time=None, fade_time=None, rt60=None, seed=3)
    assert Tail(seed=3, n_waves=32).to_dict() == dict(mix_time=None, fade_time=None, rt60=None, seed=3)      # not coherent: the old keys
    d = Tail(seed=3, coherent=True, n_waves=32, half_taps=2).to_dict()
    assert d == dict(mix_time=None, fade_time=None, rt60=None, seed=3, coherent=True, n_waves=32, half_taps=2)
    assert Tail.from_dict(json.loads(json.dumps(d))) == Tail(seed=3, coherent=True, n_waves=32, half_taps=2)
    old = Tail.from_dict(dict(mix_time=0.02, fade_time=0.005, rt60=None, seed=9))
    assert old == Tail(mix_time=0.02, fade_time=0.005, seed=9) and (old.coherent, old.n_waves, old.half_taps) == (False, 64, 4)


MIC_A = np.array([[2.0, 1.6, 1.2], [2.05, 1.6, 1.2], [2.0, 1.65, 1.2], [2.0, 1.6, 1.25]])
MIC_B = np.array([[0.7, 2.6, 1.9]])
STATE_TAIL = dict(mix_time=0.015, fade_time=0.004, rt60=None, seed=77)      # M = 240, F = 64 at 16 kHz


def _state(r, tail, ir_len=1203):
    st = core.ShoeboxIRState(ROOM, betas=(0.8, 0.9, 0.75, 0.85, 0.6, 0.7), ir_len=ir_len, sample_rate=sc.SR, renderer=r, tail=tail)
    st.add_microphone("mic000", MIC_A)
    st.add_microphone("mic001", MIC_B)
    st.add_emitters([[0.8, 0.9, 1.0]], alias="static")
    st.add_emitters(np.linspace([3.2, 0.6, 1.5], [3.4, 2.8, 1.1], 3), alias="moving")
    return st


def run_state(r):
    """A state with a group of four and a single capsule: the dictionaries, the round trip, the rows against the ABI."""
    plain = _state(r, STATE_TAIL)
    assert plain.to_dict()["shoebox"]["tail"] == STATE_TAIL      # key for key what it was
    st = _state(r, dict(STATE_TAIL, coherent=True))
    d = json.loads(json.dumps(st.to_dict()))
    assert d["shoebox"]["tail"] == dict(STATE_TAIL, coherent=True, n_waves=64, half_taps=4)
    st.simulate()
    plain.simulate()
    rows = {k: np.array(np.asarray(v)) for k, v in st.irs.items()}
    M, F = shoebox.tail_samples(st.tail, ROOM, sc.SR)
    assert (M, F) == (240, 64)
    # the single capsule is today's row; the group of four is not, past the mixing sample
    assert np.array_equal(bits(rows["mic001"]), bits(np.asarray(plain.irs["mic001"])))
    old = np.asarray(plain.irs["mic000"])
    assert np.array_equal(bits(rows["mic000"][:, :, :M + 1]), bits(old[:, :, :M + 1])) and np.all(rows["mic000"][:, :, M + 1:] != old[:, :, M + 1:])
    # the group's rows are the entry's with the tables of the microphone, group id 0 (its capsule_id0)
    sources = st.emitter_positions
    taps, delays = shoebox.coherent_tail_tables(MIC_A, None, None, float(sc.SR), st.c, 64, 4)
    ln_env = np.tile(shoebox.tail_envelope(ROOM, st.betas, 1203, float(sc.SR), M), (4, len(sources), 1))
    want = run_coherent(r, sources, None, MIC_A, None, 0.0, 1203, M, F, ln_env, taps, delays, 0, seed=77, betas=st.betas, fs=float(sc.SR))
    assert np.array_equal(bits(rows["mic000"]), bits(want[:, :, :1203]))
    again = core.ShoeboxIRState.from_dict(d, renderer=r)
    assert again.tail == st.tail
    again.simulate()
    for alias in rows:
        assert np.array_equal(bits(np.asarray(again.irs[alias])), bits(rows[alias])), alias
    del d["shoebox"]["tail"]["coherent"], d["shoebox"]["tail"]["n_waves"], d["shoebox"]["tail"]["half_taps"]      # a dictionary from before
    before = core.ShoeboxIRState.from_dict(d, renderer=r)
    assert before.tail == plain.tail and before.to_dict()["shoebox"]["tail"] == STATE_TAIL
    # capsules 0 and 1 of the group (5 cm apart, one envelope) are related past the fade as the tables predict, within 5 / sqrt(N_eff)
    # with N_eff = (sum e^2)^2 / sum e^4; those of the plain state are unrelated within the same
    late = lambda t: t[:, 0, M + F:].astype(np.float64) / np.sqrt((t[:, 0, M + F:].astype(np.float64) ** 2).sum(axis=1))[:, None]      # noqa: E731
    e2 = tc.envelope(ln_env[0, 0], 1203)[M + F:] ** 2
    tol = 5.0 / np.sqrt(e2.sum() ** 2 / (e2 * e2).sum())
    want0 = predicted_xcorr(taps[0], delays[0], taps[1], delays[1], [0])[0]
    got0, old0 = late(rows["mic000"])[0] @ late(rows["mic000"])[1], late(old)[0] @ late(old)[1]
    print(f"state pair at 5 cm: lag-0 correlation {got0:.3f} (tables: {want0:.3f}), independent tail {old0:.3f}, 5 / sqrt(N_eff) = {tol:.3f}")
    assert abs(got0 - want0) <= tol and abs(old0) <= tol


def run_end_to_end(r, monkeypatch, tmp_path):
    """Scene.generate() on the two-microphone state with every host-to-device path of an IR tensor patched to raise: equal to the same
    scene on StaticIRState(np.asarray(tensor)) bit for bit, and again from its JSON."""
    state = _state(r, dict(STATE_TAIL, coherent=True))
    scene = sc._add_events(core.Scene(1.2, state, sample_rate=sc.SR))
    real_upload = engine.Renderer.upload_irs
    monkeypatch.setattr(engine.Renderer, "upload_irs", lambda *a, **k: (_ for _ in ()).throw(AssertionError("an IR tensor went through the host")))
    got = {k: np.array(v) for k, v in scene.generate().items()}
    assert all(t._host is None for t in state.irs.values()), "the render downloaded an IR tensor"
    path = tmp_path / "shoebox_coherent_scene.json"
    scene.to_json(str(path))
    assert json.loads(path.read_text())["state"]["shoebox"]["tail"]["coherent"] is True
    again = core.Scene.from_json(str(path), {a: e._raw for a, e in scene.events.items()})
    assert isinstance(again.state, core.ShoeboxIRState) and again.state.tail == state.tail
    again.state.renderer = r
    got_again = sc._render(again)
    monkeypatch.setattr(engine.Renderer, "upload_irs", real_upload)
    host = {k: np.asarray(t) for k, t in state.irs.items()}
    want = sc._render(sc._add_events(core.Scene(1.2, core.StaticIRState(host), sample_rate=sc.SR)))
    for alias, n_ch in (("mic000", 4), ("mic001", 1)):
        assert want[alias].shape == (n_ch, round(1.2 * sc.SR)) and np.abs(want[alias]).max() > 0
        assert np.array_equal(bits(got[alias]), bits(want[alias])) and np.array_equal(bits(got_again[alias]), bits(want[alias]))
