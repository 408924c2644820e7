"""Scenarios of the device shoebox IR generator (al_ism_shoebox, audiblelight_amd/shoebox.py, core.ShoeboxIRState) and the float64
numpy oracle of its definition (DESIGN.md "Shoebox IRs"; no reference code computes this).  tests/test_hostemu_shoebox.py runs
them on the host-emulated kernel, tests/test_gpu_shoebox.py on the gfx950 build.

THE BOUND (derived, not tuned).  With y64 the oracle's float64 sum and A[t] the sum of |a_i| over the images that have a tap at t,
    |y - y64| <= 2^-24 |y64| + 2^-30 A[t]       for every sample, none excluded.
The first term is the one rounding to float32.  The second covers float64 tau (tau ~ 1e5 samples x eps64 ~ 1e-11 samples, times a
tap slope of at most about pi) and libm differences between the two evaluations of the tap, with margin; it stays about 100 times
below float32 resolution, so a float32 delay, a dropped tap or a wrong wall count fails by orders of magnitude.
"""
import ctypes as ct
import functools
import json

import numpy as np
import pytest

from audiblelight_amd import _hip, batch, core, engine, shoebox
from audiblelight_amd import synthesize as syn

C_SOUND = 343.0
HALF = 40.5
TAPS = 81


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ----------------------------------------------------------------------------- the oracle: the definition, in float64
def _axis(s, r, L, beta0, beta1, reach):
    """Every (m, p) of one axis whose image can lie within ``reach``: offsets R, reflection counts k0 + k1, gains beta0^k0 beta1^k1."""
    M = int(np.ceil(reach / L)) + 1
    m = np.repeat(np.arange(-M, M + 1), 2)
    p = np.tile(np.array([0, 1]), 2 * M + 1)
    R = (1 - 2 * p) * s + 2.0 * m * L - r
    k0, k1 = np.abs(m - p), np.abs(m)
    with np.errstate(divide="ignore"):
        gain = np.float64(beta0) ** k0 * np.float64(beta1) ** k1      # numpy: 0.0 ** 0 == 1.0
    return R, k0 + k1, gain


def oracle_pair(room, betas, s, r, ir_len, fs, c=C_SOUND, max_order=None):
    """(y64[ir_len], A[ir_len], n_images) of one source and one capsule."""
    reach = c * (ir_len + HALF) / fs
    ax = [_axis(s[i], r[i], room[i], betas[2 * i], betas[2 * i + 1], reach) for i in range(3)]
    Rx, Ry, Rz = np.meshgrid(ax[0][0], ax[1][0], ax[2][0], indexing="ij")
    order = ax[0][1][:, None, None] + ax[1][1][None, :, None] + ax[2][1][None, None, :]
    gain = ax[0][2][:, None, None] * ax[1][2][None, :, None] * ax[2][2][None, None, :]
    d = np.sqrt(Rx * Rx + Ry * Ry + Rz * Rz)
    tau = d * fs / c
    keep = tau - HALF < ir_len                     # (the others have no tap below ir_len: left out early, nothing else)
    keep &= gain > 0.0                             # a wall of beta = 0 in its path: no image
    if max_order is not None:
        keep &= order <= max_order
    d, tau, gain = d[keep], tau[keep], gain[keep]
    a = gain / (4.0 * np.pi * d)
    y, A, used = np.zeros(ir_len), np.zeros(ir_len), 0
    for ai, ti in zip(a, tau):
        lo, hi = int(np.ceil(ti - HALF)), int(np.floor(ti + HALF))
        t = np.arange(max(lo, 0), min(hi, ir_len - 1) + 1)
        u = t - ti
        t, u = t[np.abs(u) < HALF], u[np.abs(u) < HALF]
        if t.size == 0:
            continue
        used += 1
        y[t] += ai * 0.5 * (1.0 + np.cos(2.0 * np.pi * u / TAPS)) * np.sinc(u)
        A[t] += abs(ai)
    return y, A, used


@functools.lru_cache(maxsize=None)
def _oracle_cached(room, betas, sources, capsules, ir_len, fs, c, max_order):
    C, N = len(capsules), len(sources)
    y, A, used = np.zeros((C, N, ir_len)), np.zeros((C, N, ir_len)), np.zeros((C, N), dtype=np.int64)
    for ci in range(C):
        for ni in range(N):
            y[ci, ni], A[ci, ni], used[ci, ni] = oracle_pair(room, betas, sources[ni], capsules[ci], ir_len, fs, c, max_order)
    for arr in (y, A, used):
        arr.flags.writeable = False
    return y, A, used


def oracle(room, betas, sources, capsules, ir_len, fs, c=C_SOUND, max_order=None):
    """Computed once per scenario and shared (read-only)."""
    as_t = lambda v: tuple(float(x) for x in np.ravel(v))                                   # noqa: E731
    pts = lambda v: tuple(tuple(float(x) for x in row) for row in np.atleast_2d(v))           # noqa: E731
    return _oracle_cached(as_t(room), as_t(betas), pts(sources), pts(capsules), int(ir_len), float(fs), float(c), max_order)


def assert_within_bound(y, y64, A, what=None):
    y = np.asarray(y, dtype=np.float64)
    err = np.abs(y - y64)
    bound = 2.0 ** -24 * np.abs(y64) + 2.0 ** -30 * A
    worst = float((err - bound).max())
    scale = float(np.max(err / np.where(bound > 0, bound, 1.0) * (bound > 0))) if np.any(bound > 0) else 0.0
    print(f"shoebox bound [{what}]: max err {err.max():.3e}, max err / bound {scale:.3f}")
    assert np.all(err <= bound), (what, "worst excess", worst, "at", np.unravel_index(np.argmax(err - bound), err.shape))


# ----------------------------------------------------------------------------- running the entry point
GUARD = 64
SENTINEL = np.float32(7.5)


def run_abi(r, room, betas, sources, capsules, ir_len, fs, c=C_SOUND, max_order=None, pitch=None):
    """al_ism_shoebox straight into a buffer with GUARD sentinels on either side; returns the (C, N, pitch) rows, after asserting
    that the guards are intact."""
    mem, lib = r.mem, r.lib
    sources = np.ascontiguousarray(np.atleast_2d(sources), dtype=np.float64)
    capsules = np.ascontiguousarray(np.atleast_2d(capsules), dtype=np.float64)
    n, n_cap = len(sources), len(capsules)
    pitch = shoebox.pitch_of(ir_len) if pitch is None else pitch
    total = n_cap * n * pitch
    out = mem.upload(np.full(total + 2 * GUARD, SENTINEL, dtype=np.float32))
    src_dev, cap_dev = mem.upload(sources.reshape(-1)), mem.upload(capsules.reshape(-1))
    room = np.ascontiguousarray(room, dtype=np.float64)
    betas = np.ascontiguousarray(betas, dtype=np.float64)
    lib.call("al_ism_shoebox", mem.ptr(src_dev), n, mem.ptr(cap_dev), n_cap, room.ctypes.data_as(ct.POINTER(ct.c_double)),
             betas.ctypes.data_as(ct.POINTER(ct.c_double)), float(c), float(fs), -1 if max_order is None else int(max_order),
             int(ir_len), int(pitch), mem.ptr(out) + 4 * GUARD, mem.stream())
    host = np.asarray(mem.download(out))
    assert np.all(host[:GUARD] == SENTINEL) and np.all(host[GUARD + total: 2 * GUARD + total] == SENTINEL), "guard overwritten"
    return host[GUARD: GUARD + total].reshape(n_cap, n, pitch).copy()


def check_against_oracle(r, room, betas, sources, capsules, ir_len, fs, c=C_SOUND, max_order=None, what=None):
    rows = run_abi(r, room, betas, sources, capsules, ir_len, fs, c, max_order)
    assert np.all(bits(rows[:, :, ir_len:]) == 0), "pad samples must be +0"
    y64, A, used = oracle(room, betas, sources, capsules, ir_len, fs, c, max_order)
    assert_within_bound(rows[:, :, :ir_len], y64, A, what)
    return rows[:, :, :ir_len], y64, A, used


# ----------------------------------------------------------------------------- 1. anechoic
def run_anechoic(r):
    room, fs, ir_len = (5.0, 4.0, 3.0), 16000.0, 700
    s, m = np.array([1.3, 2.9, 1.1]), np.array([3.7, 0.8, 1.9])
    y, y64, A, used = check_against_oracle(r, room, np.zeros(6), s, m, ir_len, fs, what="anechoic")
    assert used[0, 0] == 1
    d = np.linalg.norm(s - m)
    tau = d * fs / C_SOUND
    peak = int(round(tau))
    assert int(np.argmax(np.abs(y[0, 0]))) == peak
    t = np.arange(ir_len)
    inside = np.abs(t - tau) < HALF
    assert inside.sum() in (80, 81)
    assert np.all(bits(y[0, 0][~inside]) == 0), "everything outside the 81 taps must be exactly zero"
    a = 1.0 / (4.0 * np.pi * d)
    u = t[inside] - tau
    taps = a * 0.5 * (1.0 + np.cos(2.0 * np.pi * u / TAPS)) * np.sinc(u)
    assert np.abs(y[0, 0][inside] - taps).max() <= 2.0 ** -23 * a


# ----------------------------------------------------------------------------- 2. general parity
UNEQUAL_BETAS = (0.0, 0.9, 0.75, 1.0, 0.6, 0.85)     # one wall at 0, one at 1, all six different
ROOMS = {"cubic": (3.0, 3.0, 3.0), "oblong": (4.1, 3.3, 2.6)}
SOURCES_5 = np.array([[0.4, 0.5, 0.6], [2.6, 0.3, 2.2], [1.5, 2.7, 0.2], [0.9, 1.1, 2.4], [2.2, 2.1, 1.3]])
CAPSULES_3 = np.array([[1.31, 1.42, 1.2], [1.35, 1.40, 1.24], [2.8, 2.9, 0.3]])
PARITY = [(room, order, pairs, fs) for room in ROOMS for order in (0, 1, 3, None) for pairs in ("1x1", "3x5")
          for fs in (16000, 48000)
          # the whole cross at 16 kHz; at 48 kHz one room per order keeps the suite quick (same code path, other tau scale)
          if fs == 16000 or (room == "oblong" and pairs == "1x1") or (room == "cubic" and pairs == "3x5" and order in (1, None))]


def parity_ir_len(order, fs):
    # unlimited order: about (4 pi / 3) (c ir_len / fs)^3 / V images per pair, some 500 here (15 m of path); with an order limit the
    # row is long enough for every image of order 3 (32 m)
    return int((0.0437 if order is None else 0.094) * fs)


def run_parity(r, room, order, pairs, fs):
    L = ROOMS[room]
    src, cap = (SOURCES_5, CAPSULES_3) if pairs == "3x5" else (SOURCES_5[1:2], CAPSULES_3[:1])
    ir_len = parity_ir_len(order, fs)
    y, y64, A, used = check_against_oracle(r, L, UNEQUAL_BETAS, src, cap, ir_len, fs, max_order=order,
                                           what=f"{room} order={order} {pairs} fs={fs}")
    if order == 0:
        assert np.all(used == 1)
    elif order is None:
        assert 100 < used.max() < 8000, used.max()    # (the wall at beta = 0 removes half the lattice)
    assert np.abs(y).max() > 0


# ----------------------------------------------------------------------------- 3. edges
EDGE_LEN = (1, 5, 80, 81, 255, 256, 257, 1000)


def run_edge_length(r, ir_len):
    """Row lengths around the tap count and the tile; the direct tap and early reflections straddle the end of the row and (from 257
    on) the tile boundary at 256."""
    room, fs = (2.4, 2.0, 1.7), 16000.0
    src = np.array([[0.5, 0.6, 0.7], [2.0, 1.5, 1.1]])
    cap = np.array([[1.9, 1.2, 0.9], [0.52, 0.63, 0.74]])     # the second capsule is 5 cm from the first source
    y, y64, A, used = check_against_oracle(r, room, (0.8, 0.7, 0.9, 0.6, 0.5, 0.95), src, cap, ir_len, fs,
                                           what=f"edge ir_len={ir_len}")
    assert np.abs(y).max() > 0
    if ir_len >= 256:     # some image has taps on both sides of sample 256 and some image is cut by the end of the row
        for ci in range(2):
            for ni in range(2):
                assert A[ci, ni, min(255, ir_len - 1)] > 0 and A[ci, ni, ir_len - 1] > 0


def run_close_capsule(r):
    """A capsule 1 cm from the source: tau = 0.47 samples, the taps at t < 0 are dropped."""
    room, fs, ir_len = (3.0, 2.5, 2.2), 16000.0, 300
    s = np.array([1.0, 1.2, 1.1])
    m = s + np.array([0.01, 0.0, 0.0])
    y, y64, A, used = check_against_oracle(r, room, np.full(6, 0.7), s, m, ir_len, fs, max_order=2, what="capsule at 1 cm")
    assert int(np.argmax(np.abs(y[0, 0]))) == 0 and y[0, 0, 0] > 1.0 / (4 * np.pi * 0.01) * 0.5


def run_crowded_tile(r):
    """A small room, a long row and no max_order: far more images touch the last tile than one chunk of lattice columns or one
    LDS list (128 entries) holds."""
    room, fs, ir_len = (2.0, 1.6, 1.2), 16000.0, 600
    y, y64, A, used = check_against_oracle(r, room, (0.9, 0.95, 0.85, 0.9, 0.97, 0.8), np.array([0.7, 0.5, 0.4]),
                                           np.array([1.4, 1.1, 0.8]), ir_len, fs, what="crowded tile")
    assert used[0, 0] > 2000, used
    assert (A[0, 0, 512:] > 0).all()


# ----------------------------------------------------------------------------- 4. determinism
def run_determinism(r):
    L, fs, ir_len = ROOMS["oblong"], 16000.0, 520
    one = run_abi(r, L, UNEQUAL_BETAS, SOURCES_5, CAPSULES_3, ir_len, fs, max_order=5)
    two = run_abi(r, L, UNEQUAL_BETAS, SOURCES_5, CAPSULES_3, ir_len, fs, max_order=5)
    assert np.array_equal(bits(one), bits(two)), "two runs differ"
    for ci, ni in ((0, 0), (1, 3), (2, 4)):
        alone = run_abi(r, L, UNEQUAL_BETAS, SOURCES_5[ni], CAPSULES_3[ci], ir_len, fs, max_order=5)
        assert np.array_equal(bits(alone[0, 0]), bits(one[ci, ni])), (ci, ni)
    # a wider pitch moves every row and adds a tile of pad samples only: same bits, zeros behind
    wide = run_abi(r, L, UNEQUAL_BETAS, SOURCES_5[:2], CAPSULES_3[:2], ir_len, fs, max_order=5, pitch=768 + 8)
    assert np.array_equal(bits(wide[:, :, :ir_len]), bits(one[:2, :2, :ir_len])) and np.all(bits(wide[:, :, ir_len:]) == 0)


# ----------------------------------------------------------------------------- 5. refusals
def run_abi_refusals(r):
    mem, lib = r.mem, r.lib
    src, cap = mem.upload(np.array([1.0, 1.0, 1.0])), mem.upload(np.array([2.0, 1.5, 1.2]))
    out = mem.upload(np.full(64, SENTINEL, dtype=np.float32))
    good = dict(sources=mem.ptr(src), n=1, capsules=mem.ptr(cap), n_cap=1, L=(3.0, 2.5, 2.0), beta=(0.5,) * 6, c=343.0, fs=16000.0,
                order=-1, ir_len=30, pitch=32, out=mem.ptr(out))

    def call(**change):
        a = dict(good, **change)
        L = None if a["L"] is None else (ct.c_double * 3)(*a["L"])
        beta = None if a["beta"] is None else (ct.c_double * 6)(*a["beta"])
        return lib.call("al_ism_shoebox", a["sources"], a["n"], a["capsules"], a["n_cap"], L, beta, a["c"], a["fs"], a["order"],
                        a["ir_len"], a["pitch"], a["out"], mem.stream())

    bad = [dict(L=(0.0, 2.5, 2.0)), dict(L=(3.0, -1.0, 2.0)), dict(L=(3.0, 2.5, float("inf"))), dict(L=(float("nan"), 2.5, 2.0)),
           dict(c=0.0), dict(c=float("nan")), dict(c=float("inf")), dict(fs=-1.0), dict(fs=float("inf")),
           dict(beta=(0.5, 0.5, 1.01, 0.5, 0.5, 0.5)), dict(beta=(-0.01,) + (0.5,) * 5), dict(beta=(0.5,) * 5 + (float("nan"),)),
           dict(n=0), dict(n_cap=0), dict(ir_len=0), dict(pitch=28), dict(pitch=34, ir_len=33), dict(order=-2),
           dict(sources=None), dict(capsules=None), dict(out=None), dict(L=None), dict(beta=None)]
    for change in bad:
        with pytest.raises(_hip.HipError, match=r"al_ism_shoebox failed \(-1\): al_ism_shoebox: "):
            call(**change)
    assert np.all(np.asarray(mem.download(out)) == SENTINEL), "a refused call wrote"
    assert call() == 0
    assert call(order=0, beta=(0.0, 1.0) * 3) == 0


def run_python_errors(r):
    room, betas = (3.0, 2.5, 2.0), (0.5,) * 6
    s, m = [[1.0, 1.0, 1.0]], [[2.0, 1.5, 1.2]]
    ok = dict(room=room, betas=betas, sources=s, capsules=m, ir_len=64, sample_rate=16000)
    bad = [dict(room=(3.0, 2.5)), dict(room=(3.0, 0.0, 2.0)), dict(room=(3.0, np.nan, 2.0)), dict(betas=(0.5,) * 5),
           dict(betas=(1.5,) + (0.5,) * 5), dict(betas=(np.nan,) + (0.5,) * 5), dict(sources=[1.0, 1.0, 1.0]),
           dict(sources=[[1.0, 1.0]]), dict(sources=np.zeros((0, 3))), dict(sources=[[np.inf, 1.0, 1.0]]),
           dict(sources=[[0.0, 1.0, 1.0]]), dict(sources=[[1.0, 2.5, 1.0]]), dict(capsules=[[1.0, 1.0, 2.1]]),
           dict(capsules=[[1.0, 1.0, -0.1]]), dict(capsules=[[1.005, 1.0, 1.0]]), dict(ir_len=0), dict(ir_len=10.5),
           dict(sample_rate=0), dict(c=-343.0), dict(max_order=-1), dict(max_order=1.5)]
    for change in bad:
        with pytest.raises(ValueError):
            shoebox.shoebox_irs_device(r, **dict(ok, **change))
    buf, strides, n = shoebox.shoebox_irs_device(r, **ok)
    assert strides == (64, 64) and n == 64
    with pytest.raises(ValueError):
        shoebox.betas_from_absorption([0.1, 1.2])
    assert np.allclose(shoebox.betas_from_absorption([0.0, 0.36, 1.0]), [1.0, 0.8, 0.0])
    with pytest.raises(ValueError):
        core.ShoeboxIRState(room, betas=betas, rt60=0.4)
    with pytest.raises(ValueError):
        core.ShoeboxIRState(room)
    with pytest.raises(ValueError):
        core.ShoeboxIRState(room, betas=(2.0,) * 6)
    st = core.ShoeboxIRState(room, betas=betas, ir_len=64, sample_rate=16000, renderer=r)
    with pytest.raises(ValueError):
        st.add_microphone("m", [[4.0, 1.0, 1.0]])
    with pytest.raises(ValueError):
        st.add_emitters([[1.0, 1.0, 2.0]])


def run_rt60_round_trip():
    room, c = (6.0, 5.0, 3.0), 343.0
    V, S = 90.0, 2 * (30.0 + 18.0 + 15.0)
    for rt60 in (0.3, 0.6, 1.2):
        b = shoebox.betas_from_rt60(room, rt60, c)
        assert b.shape == (6,) and np.all(b == b[0])
        alpha = 1.0 - b[0] ** 2
        assert 24.0 * np.log(10.0) * V / (c * S * alpha) == pytest.approx(rt60, rel=1e-12)      # Sabine: 0.161 V / (S alpha) at 343 m/s
    with pytest.raises(ValueError, match="Sabine"):
        shoebox.betas_from_rt60(room, 0.05, c)


# ----------------------------------------------------------------------------- 6. the lazy tensor and the state
def run_state_and_tensor(r):
    st = core.ShoeboxIRState((4.1, 3.3, 2.6), betas=UNEQUAL_BETAS, ir_len=333, sample_rate=16000, max_order=3, renderer=r)
    assert st.name == "SHOEBOX" and st.num_emitters == 0 and len(st.microphones) == 0
    st.add_microphone("mic000", CAPSULES_3)
    st.add_emitters(SOURCES_5[:1])
    st.add_emitters(SOURCES_5[1:4])
    assert st.num_emitters == 4 and st.microphones["mic000"].n_capsules == 3
    with pytest.raises(AttributeError):
        st.irs
    st.simulate()
    t = st.get_irs()["mic000"]
    assert isinstance(t, shoebox.DeviceIRTensor) and st.irs["mic000"] is t
    assert t.shape == (3, 4, 333) and t.dtype == np.float32 and t.ndim == 3 and t.size == 3 * 4 * 333 and t.nbytes == 4 * t.size
    buf, strides = t.result()
    assert strides == (4 * 336, 336)
    host = np.asarray(t)
    assert host.shape == t.shape and host.dtype == np.float32 and np.shares_memory(np.asarray(t), host) and t._host is host   # downloaded once
    assert np.array_equal(t[1, 2:4, :], host[1, 2:4, :])
    y64, A, _ = oracle((4.1, 3.3, 2.6), UNEQUAL_BETAS, SOURCES_5[:4], CAPSULES_3, 333, 16000.0, max_order=3)
    assert_within_bound(host, y64, A, "state")
    d = json.loads(json.dumps(st.to_dict()))
    assert d["backend"] == "SHOEBOX" and d["sample_rate"] == 16000 and d["shoebox"]["room"] == [4.1, 3.3, 2.6]
    assert d["shoebox"]["max_order"] == 3 and d["shoebox"]["betas"] == list(UNEQUAL_BETAS) and d["shoebox"]["ir_len"] == 333
    assert [len(v) for v in d["emitters"].values()] == [1, 3]
    assert d["microphones"]["mic000"]["n_capsules"] == 3 and d["microphones"]["mic000"]["coordinates_absolute"] == CAPSULES_3.tolist()
    st.add_emitters(SOURCES_5[4:])         # a change drops the tensors
    with pytest.raises(AttributeError):
        st.irs
    by_rt60 = core.ShoeboxIRState((6.0, 5.0, 3.0), rt60=0.5, ir_len=64, sample_rate=16000, renderer=r)
    assert np.allclose(by_rt60.betas, shoebox.betas_from_rt60((6.0, 5.0, 3.0), 0.5))


# ----------------------------------------------------------------------------- 7. end to end
SR = 16000


def _clip(n, seed):
    rng = np.random.default_rng(seed)
    return (0.3 * rng.standard_normal(n) * np.hanning(n)).astype(np.float32)


def _shoebox_state(r):
    st = core.ShoeboxIRState((4.1, 3.3, 2.6), betas=(0.8, 0.9, 0.75, 0.85, 0.6, 0.7), ir_len=1203, sample_rate=SR, max_order=4, renderer=r)
    st.add_microphone("mic000", np.array([[2.0, 1.6, 1.2], [2.05, 1.6, 1.2], [2.0, 1.65, 1.2], [2.0, 1.6, 1.25]]))
    st.add_emitters([[0.8, 0.9, 1.0]], alias="static")
    st.add_emitters(np.linspace([3.2, 0.6, 1.5], [3.4, 2.8, 1.1], 3), alias="moving")
    return st


def _add_events(scene):
    scene.add_event(core.Event("static", _clip(6000, 1), SR, snr=12.0, scene_start=0.1, n_emitters=1))
    scene.add_event(core.Event("moving", _clip(9000, 2), SR, snr=9.0, scene_start=0.4, n_emitters=3))
    return scene


def _render(scene):
    syn.render_audio_for_all_scene_events(scene)
    syn.generate_scene_audio_from_events(scene)
    return {k: np.array(v) for k, v in scene.audio.items()}


def run_end_to_end(r, monkeypatch, tmp_path):
    """One static and one moving event on a ShoeboxIRState: rendered with every host-to-device path of an IR tensor patched to
    raise, equal bit for bit to the same scene on StaticIRState(np.asarray(tensor)), through render_merged / scene_jobs, and from
    its own JSON without IR arrays."""
    state = _shoebox_state(r)
    scene = _add_events(core.Scene(1.2, state, sample_rate=SR))

    def refuse(*a, **k):
        raise AssertionError("an IR tensor went through the host")

    real_upload = engine.Renderer.upload_irs
    monkeypatch.setattr(engine.Renderer, "upload_irs", refuse)
    got = _render(scene)
    tensor = state.irs["mic000"]
    assert tensor._host is None, "the render downloaded the IR tensor"
    jobs = batch.scene_jobs(scene, "s", renderer=r)
    assert len(jobs) == 1 and jobs[0].irs is tensor
    merged = batch.render_merged(r, jobs)
    # two scenes in one launch sequence: the tensors are joined on the device
    twice = batch.render_merged(r, jobs + batch.scene_jobs(scene, "again", renderer=r))
    # JSON round trip, no IR arrays
    path = tmp_path / "shoebox_scene.json"
    scene.to_json(str(path))
    clips = {a: e._raw for a, e in scene.events.items()}
    again = core.Scene.from_json(str(path), clips)
    assert isinstance(again.state, core.ShoeboxIRState) and again.state.num_emitters == 4
    again.state.renderer = r
    got_again = _render(again)
    assert tensor._host is None
    monkeypatch.setattr(engine.Renderer, "upload_irs", real_upload)

    host = np.asarray(tensor)
    static_scene = _add_events(core.Scene(1.2, core.StaticIRState({"mic000": host}), sample_rate=SR))
    want = _render(static_scene)
    assert want["mic000"].shape == (4, round(1.2 * SR)) and np.abs(want["mic000"]).max() > 0
    assert np.array_equal(bits(got["mic000"]), bits(want["mic000"]))
    assert np.array_equal(bits(got_again["mic000"]), bits(want["mic000"]))
    want_merged = batch.render_merged(r, batch.scene_jobs(static_scene, "s", renderer=r))
    assert np.array_equal(bits(merged[0]), bits(want_merged[0]))
    assert np.array_equal(bits(twice[0]), bits(want_merged[0])) and np.array_equal(bits(twice[1]), bits(want_merged[0]))
    # with tensors given, from_json behaves as before: a static state
    as_before = core.Scene.from_json(str(path), clips, {"mic000": host})
    assert isinstance(as_before.state, core.StaticIRState)
    with pytest.raises(KeyError):
        meta = json.loads(path.read_text())
        del meta["state"]["shoebox"]
        core.Scene.from_dict(meta, clips, {})


def run_batch_driver(r, monkeypatch):
    """The pipelined driver (torch memory provider only) stages a DeviceIRTensor without a copy and counts no H2D bytes for it."""
    state = _shoebox_state(r)
    scene = _add_events(core.Scene(1.2, state, sample_rate=SR))
    state.simulate()
    tensor = state.irs["mic000"]
    host_jobs = batch.scene_jobs(_add_events(core.Scene(1.2, core.StaticIRState({"mic000": np.asarray(tensor)}), sample_rate=SR)), "h",
                                 renderer=r)
    jobs = batch.scene_jobs(scene, "d", renderer=r)

    real = engine.Renderer.upload_irs
    monkeypatch.setattr(engine.Renderer, "upload_irs", lambda *a, **k: (_ for _ in ()).throw(AssertionError("IR tensor uploaded")))
    got = {}
    drv = batch.BatchDriver(r)
    rep = drv.run(jobs, on_scene=got.__setitem__)
    monkeypatch.setattr(engine.Renderer, "upload_irs", real)
    want = {}
    rep_host = drv.run(host_jobs, on_scene=want.__setitem__)
    assert rep_host.h2d_bytes - rep.h2d_bytes == tensor.nbytes and rep.h2d_bytes > 0     # the clips still travel
    assert np.array_equal(bits(got["d/mic000"]), bits(want["h/mic000"]))
