"""Scenarios of the device dynamics FX (Compressor, Limiter) and of their entry points ``al_fx_compressor`` and
``al_fx_limiter``, shared by tests/test_hostemu_dynamics_fx.py (host emulation) and tests/test_gpu_dynamics_fx.py (gfx950 build).
Every scenario takes the renderer ``r`` the package is set to.

The oracle is a plain float64 restatement of the definitions written HERE (DESIGN.md "Dynamics FX": JUCE's dsp::Compressor,
dsp::BallisticsFilter in peak mode and dsp::Limiter as pedalboard 0.9.17 wraps them and as this project reads them; NOT checked
against a running pedalboard), as sample loops in the compare / select form, so the package is not checked against itself.

The bound is the one the filter and delay / modulation FX are held to: 1e-5 on the relative RMS and on max-abs / peak; the
expected residue is the float32 rounding of the output (6e-8).

Most inputs are burst-modulated noise (``bursts``): a kernel that ignored the threshold or one of the two coefficients must not
pass, so ``assert_exercised`` checks FROM THE ORACLE ALONE that in every parity case both branches of the envelope are taken and
the envelope is below and above the threshold on at least 5 % of the samples each, in every stage.
"""
import collections
import ctypes as ct
import json
import math
import os

import numpy as np
import pytest

from audiblelight_amd import _hip, augmentation as aug, core
from oracle import synth_oracle as orc
from tests import delay_mod_fx_cases as dmc
from tests import kernel_edges as ke
from tests.conftest import assert_parity, parity_errors

FS = (16000, 24000, 44100, 48000)
TOL = 1e-5
TILE = _hip.DYN_TILE        # csrc/al_dynfx.h DYN_TILE = 1024
assert TILE == 1024
EDGE_N = (1, 2, 3, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE + 1, 16385)
CLIP_10S = 10 * 48000
KINDS = {"compressor": _hip.FXB_COMPRESSOR, "limiter": _hip.FXB_LIMITER}
LIMITER_STAGE1 = (-10.0, 4.0, 2.0, 200.0)


# ----------------------------------------------------------------------------- the oracle
def cte(ms, fs):
    return 0.0 if ms < 1e-3 else math.exp(-2.0 * math.pi * 1000.0 / (ms * fs))


Stage = collections.namedtuple("Stage", "y env threshold attacks releases")


def ref_stage(x, fs, threshold_db, ratio, attack_ms, release_ms):
    """One compressor stage: a = |x|, c = cA if a > e else cR, e = a + c (e - a), g = 1 if e < T else (e / T)^(1/ratio - 1)."""
    x = np.asarray(x, dtype=np.float64)
    T = 10.0 ** (threshold_db / 20.0)
    cA, cR = cte(attack_ms, fs), cte(release_ms, fs)
    e, attacks = 0.0, 0
    env = [0.0] * len(x)
    for t, a in enumerate(np.abs(x).tolist()):
        if a > e:
            e = a + cA * (e - a)
            attacks += 1
        else:
            e = a + cR * (e - a)
        env[t] = e
    env = np.array(env)
    with np.errstate(divide="ignore"):
        g = np.where(env < T, 1.0, (env / T) ** (1.0 / ratio - 1.0))
    return Stage(g * x, env, T, attacks, len(x) - attacks)


def ref_compressor(x, fs, threshold_db, ratio, attack_ms, release_ms):
    return ref_stage(x, fs, threshold_db, ratio, attack_ms, release_ms).y


def limiter_gain(threshold_db):
    return 10.0 ** (10.0 * (1.0 - 1.0 / 4.0) / 40.0) * 10.0 ** (-threshold_db / 20.0)


def ref_limiter_parts(x, fs, threshold_db, release_ms):
    """(stage 1, stage 2, the un-clamped output): stage 2's 0.001 ms attack is cA = 0."""
    s1 = ref_stage(x, fs, *LIMITER_STAGE1)
    s2 = ref_stage(s1.y, fs, threshold_db, 1000.0, 0.0, release_ms)
    return s1, s2, limiter_gain(threshold_db) * s2.y


def ref_limiter(x, fs, threshold_db, release_ms):
    return np.clip(ref_limiter_parts(x, fs, threshold_db, release_ms)[2], -1.0, 1.0)


def ref_fx(fx, x):
    p, fs = fx.params, fx.sample_rate
    if isinstance(fx, aug.Compressor):
        return ref_compressor(x, fs, p["threshold_db"], p["ratio"], p["attack_ms"], p["release_ms"])
    if isinstance(fx, aug.Limiter):
        return ref_limiter(x, fs, p["threshold_db"], p["release_ms"])
    return dmc.ref_fx(fx, x)


def stages_of(fx, x):
    p, fs = fx.params, fx.sample_rate
    if isinstance(fx, aug.Compressor):
        return [ref_stage(x, fs, p["threshold_db"], p["ratio"], p["attack_ms"], p["release_ms"])]
    return list(ref_limiter_parts(x, fs, p["threshold_db"], p["release_ms"])[:2])


def assert_exercised(stages, what=None):
    """Both branches taken, the envelope below and above the threshold on >= 5 % of the samples each, in every stage."""
    for k, s in enumerate(stages):
        n = len(s.env)
        below = int(np.count_nonzero(s.env < s.threshold))
        assert s.attacks > 0 and s.releases > 0, (what, k, s.attacks, s.releases)
        assert below >= 0.05 * n and n - below >= 0.05 * n, (what, k, below / n)


def bursts(n, seed, fs=48000, period=300):
    """Uniform noise in (-1, 1) times a gate: 0.003 over the first 30 % of the clip (an envelope that starts at zero stays
    under every threshold of the cases there, -40 dB = 0.01 included), then 0.8 and 0.003 in turns of ``period`` samples (three
    loud turns for each quiet one, so that a slow release still leaves the envelope over the threshold)."""
    x = np.random.default_rng(seed).uniform(-1, 1, n)
    t = np.arange(n)
    loud = (t >= int(0.3 * n)) & ((t // period) % 4 != 3)
    return (x * np.where(loud, 0.8, 0.003)).astype(np.float32)


def check(got, want, what=None, tol=TOL):
    rms, mx = parity_errors(got, want)
    print(f"dynamics {what}: rel rms {rms:.3g} max/peak {mx:.3g} (bound {tol:g})")
    assert rms <= tol and mx <= tol, (what, rms, mx)
    return rms, mx


def check_fx(fx, x, what=None):
    assert_exercised(stages_of(fx, x), what=(what, fx))
    got = fx(x)
    assert got.dtype == np.float32 and got.shape == x.shape
    check(got, ref_fx(fx, x), what=(what, fx))
    return got


# ----------------------------------------------------------------------------- 1. every class at every rate
def class_cases(fs):
    return [
        ("compressor", aug.Compressor(fs, threshold_db=-30, ratio=4, attack_ms=5, release_ms=120)),
        ("compressor_cA_gt_cR", aug.Compressor(fs, threshold_db=-20, ratio=20, attack_ms=100, release_ms=50)),
        ("compressor_attack_0", aug.Compressor(fs, threshold_db=-30, ratio=8, attack_ms=0, release_ms=120)),
        ("compressor_release_0", aug.Compressor(fs, threshold_db=-30, ratio=8, attack_ms=5, release_ms=0.0005)),
        ("limiter", aug.Limiter(fs, threshold_db=-25, release_ms=300)),
        ("limiter_fast", aug.Limiter(fs, threshold_db=-40, release_ms=50)),
    ]


def run_class_parity(fs, seconds=1.0):
    x = bursts(int(seconds * fs), fs, fs)
    for label, fx in class_cases(fs):
        if label == "compressor_cA_gt_cR":
            assert cte(100, fs) > cte(50, fs)
        check_fx(fx, x, what=(fs, label))
    # ratio 1: the identity, bit for bit (the envelope and the threshold are exercised all the same)
    ident = aug.Compressor(fs, threshold_db=-40, ratio=1, attack_ms=1, release_ms=1100)
    assert_exercised(stages_of(ident, x), what=(fs, "ratio 1"))
    ke.assert_bits_equal(ident(x), x, (fs, "ratio 1"))


def run_defaults_drawn(fs, seconds=1.0, seeds=range(3)):
    x = bursts(int(seconds * fs), fs + 1, fs)
    for seed in seeds:
        for cls in (aug.Compressor, aug.Limiter):
            np.random.seed(seed)
            check_fx(cls(fs), x, what=(fs, seed))


# ----------------------------------------------------------------------------- 2. guarded edge lengths, both entries
COMP_ARGS = (-30.0, 4.0, 5.0, 120.0)
LIM_ARGS = (-25.0, 300.0)


def call(r, kind, src, dst, n, fs, *args):
    return r.lib.call("al_fx_compressor" if kind == "compressor" else "al_fx_limiter", src, dst, n, float(fs), *args, r.mem.stream())


def ref_kind(kind, x, fs, *args):
    return ref_compressor(x, fs, *args) if kind == "compressor" else ref_limiter(x, fs, *args)


def run_edge_lengths(r, n, shift=0, fs=48000):
    x = ke.signal(n, 600 + n, special=True)
    src = ke.dev(r, x)
    for kind, args in (("compressor", COMP_ARGS), ("compressor", (-20.0, 20.0, 100.0, 50.0)), ("limiter", LIM_ARGS)):
        out = ke.Guarded(r, n, shift=shift)
        call(r, kind, r.mem.ptr(src), out.ptr, n, fs, *args)
        check(out.get(), ref_kind(kind, x, fs, *args), what=(kind, n, args))


# ----------------------------------------------------------------------------- 3. the Limiter's structure
def run_limiter_structure(fs=48000, n=20000):
    x = bursts(n, 21, fs)
    for threshold_db, release_ms in ((-25, 300.0), (-40, 50.0), (-20, 1100.0)):
        fx = aug.Limiter(fs, threshold_db=threshold_db, release_ms=release_ms)
        s1, s2, loud = ref_limiter_parts(x, fs, threshold_db, release_ms)
        assert np.count_nonzero(np.abs(loud) > 1.0) > 100, "the clamp is not reached"
        got = check_fx(fx, x, what=("limiter structure", threshold_db, release_ms))
        assert np.max(np.abs(got)) <= 1.0
        assert np.count_nonzero(np.abs(got) == 1.0) > 100
        # the composition, spelled out: stage 1 -> stage 2 on its output -> gain -> clamp
        y1 = ref_compressor(x, fs, *LIMITER_STAGE1)
        y2 = ref_compressor(y1, fs, threshold_db, 1000.0, 0.0, release_ms)
        check(got, np.clip(limiter_gain(threshold_db) * y2, -1.0, 1.0), what="composition")


# ----------------------------------------------------------------------------- 4. silence and tiny input
def run_silence_and_tiny(fs=44100, n=3 * TILE + 17):
    zeros = np.zeros(n, dtype=np.float32)
    tiny = (np.random.default_rng(8).uniform(-1, 1, n) * 0.004).astype(np.float32)     # under -40 dB = 0.01 throughout
    comp = aug.Compressor(fs, threshold_db=-40, ratio=20, attack_ms=1, release_ms=50)
    lim = aug.Limiter(fs, threshold_db=-40, release_ms=50)
    for fx in (comp, lim):
        ke.assert_bits_equal(fx(zeros), zeros, ("silence", fx))
    assert np.max(stages_of(comp, tiny)[0].env) < 0.01
    ke.assert_bits_equal(comp(tiny), tiny, "below the threshold")
    s1, s2 = stages_of(lim, tiny)
    assert np.max(s1.env) < s1.threshold and np.max(s2.env) < s2.threshold
    check(lim(tiny), limiter_gain(-40) * tiny.astype(np.float64), what="limiter below both thresholds: the gain alone")


# ----------------------------------------------------------------------------- 5. a batch equals the single-clip launches
BATCH_N = (1, 700, 2 * TILE + 1, TILE, 5003)


def specs(kind):
    rows = {"compressor": [(48000, -30.0, 4.0, 5.0, 120.0), (44100, -20.0, 20.0, 100.0, 50.0), (16000, -35.0, 8.0, 0.0, 300.0),
                           (24000, -40.0, 1.0, 1.0, 1100.0), (48000, -25.0, 12.0, 30.0, 0.0005)],
            "limiter": [(48000, -25.0, 300.0), (44100, -40.0, 50.0), (16000, -20.0, 1100.0), (24000, -33.0, 120.0),
                        (48000, -30.0, 0.0)]}[kind]
    return [dict(n=n, x=bursts(n, 50 + n, period=150) if n > 64 else ke.signal(n, 50 + n), args=(float(row[0]),) + row[1:])
            for n, row in zip(BATCH_N, rows)]


def job_array(kind, jobs):
    arr = (_hip.FXB_JOBS[KINDS[kind]] * max(len(jobs), 1))()
    names = [f for f, _ in _hip.FXB_JOBS[KINDS[kind]]._fields_[3:]]
    for job, (src, dst, n, args) in zip(arr, jobs):
        job.src, job.dst, job.n = src, dst, n
        for name, value in zip(names, args):
            setattr(job, name, value)
    return arr


def pack(r, kind, jobs):
    arr = job_array(kind, jobs)
    per = r.lib.call("al_fx_batch_desc_bytes", KINDS[kind])
    assert per > 0 and per % 8 == 0
    table = np.zeros(len(jobs) * per, dtype=np.uint8)
    r.lib.call("al_fx_batch_pack", KINDS[kind], ct.cast(arr, ct.c_void_p), len(jobs), table.ctypes.data)
    return table


def run_batch_equals_singles(r, kind):
    batch = specs(kind)
    assert min(s["n"] for s in batch) == 1 and any(1 < s["n"] < TILE for s in batch) and len({s["n"] for s in batch}) == 5
    want = []
    for i, spec in enumerate(batch):
        src = ke.dev(r, spec["x"])
        out = ke.Guarded(r, spec["n"], shift=i % 2)
        call(r, kind, r.mem.ptr(src), out.ptr, spec["n"], *spec["args"])
        want.append(out.get())
    srcs = [ke.dev(r, spec["x"]) for spec in batch]
    outs = [ke.Guarded(r, spec["n"], shift=i % 2) for i, spec in enumerate(batch)]
    table = pack(r, kind, [(r.mem.ptr(s), o.ptr, spec["n"], spec["args"]) for s, o, spec in zip(srcs, outs, batch)])
    device_table = r.mem.upload(table)
    r.lib.call("al_fx_batch_launch", KINDS[kind], r.mem.ptr(device_table), len(batch), r.mem.stream())
    for i, (out, w, spec) in enumerate(zip(outs, want, batch)):
        got = out.get()
        assert np.array_equal(ke.bits(got), ke.bits(w)), (kind, "job", i, spec["n"])
        check(got, ref_kind(kind, spec["x"], *spec["args"]), what=("batched", kind, spec["n"]))


def run_batch_refusals(r):
    n = 256
    x = ke.dev(r, dmc.noise(4 * n, 3))
    xp = r.mem.ptr(x)
    poison = np.full(n, 0.625, dtype=np.float32)
    outs = [ke.Guarded(r, n, init=poison) for _ in range(3)]
    good = {"compressor": (48000.0,) + COMP_ARGS, "limiter": (48000.0,) + LIM_ARGS}

    def refused(kind, jobs, match, job):
        with pytest.raises(_hip.HipError, match=match):
            pack(r, kind, jobs)
        err = r.lib.last_error()
        assert err.startswith(f"al_fx_batch_pack: job {job}: "), err
        return err

    for kind, entry in (("compressor", "al_fx_compressor"), ("limiter", "al_fx_limiter")):
        g = good[kind]
        clean = [(xp + 4 * n * k, outs[k].ptr, n, g) for k in range(3)]
        bad_fs = (float("nan"),) + g[1:]
        bad_threshold = (g[0], -200.0) + g[2:]
        for bad, why in (((None, outs[2].ptr, n, g), "null pointer"), ((xp, outs[2].ptr, 0, g), "n must be >= 1"),
                         ((xp + 8 * n, xp + 8 * n + 8, n, g), "dst overlaps src"), ((xp + 8 * n, outs[2].ptr, n, bad_fs), "fs must be finite and > 0"),
                         ((xp + 8 * n, outs[2].ptr, n, bad_threshold), "threshold_db must be finite and > -200")):
            err = refused(kind, clean[:2] + [bad], why, 2)
            assert entry in err
        refused(kind, [(xp, outs[0].ptr, n, bad_fs), clean[1]], "fs must be finite", 0)
        # a dst range that overlaps the src or dst range of ANOTHER job
        base = outs[0].ptr
        refused(kind, [clean[0], (base, outs[1].ptr, n, g)], "dst overlaps src or dst of job 1", 0)
        refused(kind, [clean[0], (xp + 4 * n, base, n, g)], "dst overlaps src or dst of job 1", 0)
        refused(kind, [clean[1], clean[0], (base + 4 * (n - 2), outs[2].ptr, 2, g)], "dst overlaps src or dst of job 2", 1)
        big = ke.dev(r, np.zeros(4 * n, np.float32))
        bp = r.mem.ptr(big)
        assert len(pack(r, kind, [(bp, bp + 4 * n, n, g), (bp + 8 * n, bp + 12 * n, n, g)])) > 0     # adjacent ranges
    r.mem.synchronize()
    for out in outs:
        ke.assert_bits_equal(out.get(), poison, "a refused batch wrote")


# ----------------------------------------------------------------------------- 6. C ABI refusals
def run_abi_refusals(r):
    n = 256
    x = ke.dev(r, dmc.noise(n, 3))
    y = r.mem.empty(n)
    xp, yp = r.mem.ptr(x), r.mem.ptr(y)
    nan, inf = float("nan"), float("inf")

    def refused(match, kind, src, dst, nn, *args):
        entry = "al_fx_compressor" if kind == "compressor" else "al_fx_limiter"
        with pytest.raises(_hip.HipError, match=match):
            call(r, kind, src, dst, nn, *args)
        assert match in r.lib.last_error() and entry in r.lib.last_error(), r.lib.last_error()

    for kind, good in (("compressor", (48000.0,) + COMP_ARGS), ("limiter", (48000.0,) + LIM_ARGS)):
        refused("null pointer", kind, None, yp, n, *good)
        refused("null pointer", kind, xp, None, n, *good)
        refused("n must be >= 1", kind, xp, yp, 0, *good)
        refused("n must be >= 1", kind, xp, yp, -3, *good)
        refused("dst overlaps src", kind, xp, xp, n, *good)
        refused("dst overlaps src", kind, xp, xp + 4 * (n - 1), n, *good)
        for bad in (nan, inf, 0.0, -48000.0):
            refused("fs must be finite and > 0", kind, xp, yp, n, bad, *good[1:])
        for bad in (nan, inf, -inf, -200.0, -250.0):
            refused("threshold_db must be finite and > -200", kind, xp, yp, n, good[0], bad, *good[2:])
        for bad in (nan, inf, -1.0):
            refused("release_ms must be finite and >= 0", kind, xp, yp, n, *good[:-1], bad)
    good = (48000.0,) + COMP_ARGS
    for bad in (nan, inf, 0.0, 0.999, -4.0):
        refused("ratio must be finite and >= 1", "compressor", xp, yp, n, *good[:2], bad, *good[3:])
    for bad in (nan, inf, -1.0):
        refused("attack_ms must be finite and >= 0", "compressor", xp, yp, n, *good[:3], bad, good[4])
    for bad in (100.0, 250.0):
        refused("threshold_db must be < 100", "limiter", xp, yp, n, 48000.0, bad, 300.0)
    # accepted at the edges: adjacent buffers, ratio = 1, attack_ms = 0, release_ms = 0, a threshold just over -200 dB
    big = r.mem.empty(2 * n)
    big[:] = 0.25
    bp = r.mem.ptr(big)
    assert call(r, "compressor", bp, bp + 4 * n, n, *good) == 0
    assert call(r, "limiter", bp, bp + 4 * n, n, 48000.0, *LIM_ARGS) == 0
    assert call(r, "compressor", xp, yp, n, 48000.0, -30.0, 1.0, 0.0, 0.0) == 0
    assert call(r, "compressor", xp, yp, n, 48000.0, -199.0, 4.0, 5.0, 120.0) == 0
    assert call(r, "limiter", xp, yp, n, 48000.0, 99.0, 0.0) == 0
    r.mem.synchronize()


# ----------------------------------------------------------------------------- 7. the classes
KEYS = {aug.Compressor: ["threshold_db", "ratio", "attack_ms", "release_ms"], aug.Limiter: ["threshold_db", "release_ms"]}


def run_class_api():
    assert all(c in aug.ALL_EVENT_AUGMENTATIONS for c in KEYS)
    C, L = aug.Compressor, aug.Limiter
    assert C.RATIOS == [4, 8, 12, 20]
    assert (C.MIN_THRESHOLD_DB, C.MAX_THRESHOLD_DB, C.MIN_ATTACK, C.MAX_ATTACK, C.MIN_RELEASE, C.MAX_RELEASE) == (-40, -20, 1, 100, 50, 1100)
    assert (L.MIN_THRESHOLD_DB, L.MAX_THRESHOLD_DB, L.MIN_RELEASE, L.MAX_RELEASE) == (-40, -20, 50, 1100)
    ranges = {"threshold_db": (-40, -20), "attack_ms": (1, 100), "release_ms": (50, 1100)}
    for cls, keys in KEYS.items():
        for seed in range(20):
            np.random.seed(seed)
            a = cls(44100)
            np.random.seed(seed)
            b = cls(44100)
            assert a == b and a.to_dict() == b.to_dict()
            assert list(a.params) == keys
            d = a.to_dict()
            assert d["name"] == cls.__name__ and d["sample_rate"] == 44100
            assert isinstance(d["threshold_db"], int)
            for key in keys:
                if key == "ratio":
                    assert d[key] in C.RATIOS and isinstance(d[key], int)
                else:
                    lo, hi = ranges[key]
                    assert lo <= d[key] <= hi, (cls, key, d[key])
                assert getattr(a, key) == d[key]
            again = aug.Augmentation.from_dict(json.loads(json.dumps(d)))
            assert type(again) is cls and again == a and again.to_dict() == d
        assert cls(44100).host_dtype(np.dtype(np.float64)) == np.float32
        assert cls(44100, threshold_db=17.9).threshold_db == -17          # truncated, then made negative
        with pytest.raises(ValueError, match="positive"):
            cls(44100, release_ms=-1.0)
        with pytest.raises(TypeError):
            cls(44100, release_ms="slow")
    # the draws come in the reference's order: threshold, ratio (np.random.choice), attack, release
    np.random.seed(7)
    want = (-abs(int(np.random.uniform(-40, -20))), int(np.random.choice(C.RATIOS)), float(np.random.uniform(1, 100)),
            float(np.random.uniform(50, 1100)))
    np.random.seed(7)
    assert tuple(C(48000).params.values()) == want
    with pytest.raises(ValueError):
        C(44100, ratio=0)
    with pytest.raises(ValueError):
        C(44100, ratio=-2)
    assert C(44100, ratio=1).ratio == 1
    # the reference's on-disk layout loads
    for d in (dict(name="Compressor", sample_rate=44100, threshold_db=-30, ratio=4, attack_ms=10.0, release_ms=200.0),
              dict(name="Limiter", sample_rate=48000, threshold_db=-25, release_ms=300.0)):
        fx = aug.Augmentation.from_dict(d)
        assert type(fx).__name__ == d["name"] and fx.to_dict() == d


# ----------------------------------------------------------------------------- 8. a chain on an Event, and in a scene
def chains(sr):
    return [[aug.Compressor(sr, threshold_db=-30, ratio=4, attack_ms=5.0, release_ms=120.0),
             aug.LowpassFilter(sr, cutoff_frequency_hz=2500.0),
             aug.Limiter(sr, threshold_db=-25, release_ms=300.0)],
            [aug.Limiter(sr, threshold_db=-32, release_ms=80.0), aug.Invert(sr)]]


def oracle_chain(raw, fxs):
    y = np.asarray(raw, dtype=np.float64)
    for fx in fxs:
        y = ref_fx(fx, y)
    return orc.peak_normalise_clip(y)


def run_event_chain(r, monkeypatch):
    sr = 16000
    rng = np.random.default_rng(5)
    raws = [bursts(9000, 31, sr) * np.float32(0.9), (rng.standard_normal(7000) * 0.3).astype(np.float32)]
    fxs = chains(sr)

    def no_host_fx(self, *a, **k):
        raise AssertionError(f"{self.name} ran as a host FX call")

    monkeypatch.setattr(aug.Augmentation, "process", no_host_fx)    # the foreign-callables branch calls aug(out)
    for raw, chain in zip(raws, fxs):
        got = core.Event("dyn", raw, sr, augmentations=chain).load_audio()
        want = oracle_chain(raw, chain)
        check(got, want, what="load_audio")
        assert_parity(got, want)
    # through a scene render: one upload (the staging arena), zero downloads, one launch per pending kind
    C, L = 3, 500
    irs = (rng.standard_normal((C, 2, L)) * np.exp(-np.arange(L) / 100.0)).astype(np.float32)
    scene = core.Scene(1.5, core.StaticIRState({"mic000": irs}), sample_rate=sr, ref_db=-65)
    for i, (x, c) in enumerate(zip(raws, fxs)):
        scene.add_event(core.Event(f"e{i}", x, sr, snr=8.0 + 3 * i, scene_start=0.2 * i, augmentations=c))
    calls = []
    real = r.lib.call

    def counting(name, *args):
        calls.append((name, args))
        return real(name, *args)

    monkeypatch.setattr(r.lib, "call", counting)
    scene.generate()
    monkeypatch.setattr(r.lib, "call", real)
    launches = collections.Counter((args[0], args[2]) for name, args in calls if name == "al_fx_batch_launch")
    # wave 1: e0's Compressor, e1's Limiter; wave 2: e0's low-pass; wave 3: e0's Limiter
    assert launches == {(_hip.FXB_COMPRESSOR, 1): 1, (_hip.FXB_LIMITER, 1): 2, (_hip.FXB_SOS, 1): 1}, launches
    assert not [name for name, _ in calls if name in ("al_fx_compressor", "al_fx_limiter")]
    spatials = []
    for i, ev in enumerate(scene.events.values()):
        want = orc.render_event(oracle_chain(raws[i], fxs[i]), irs[:, [i], :].astype(np.float64), ev.snr, sr=sr)["spatial"]
        spatials.append(want)
        assert_parity(ev.spatial_audio["mic000"], want, what=ev.alias)
        clip = ev._last_chain
        assert clip.uploads == 1 and clip.downloads == 0
    ref = orc.mix_scene(spatials, [(e.scene_start, e.scene_end) for e in scene.events.values()], 1.5, sr, keep_padded=False)
    assert_parity(scene.audio["mic000"], ref["scene"])


def run_scene_batches_by_kind(r, monkeypatch):
    """Four events whose chains all start with a dynamics FX: the pending jobs go out as ONE launch per kind."""
    sr = 16000
    fxs = [[aug.Compressor(sr, threshold_db=-30 + i, ratio=4, attack_ms=5.0, release_ms=120.0)] if i % 2 == 0 else
           [aug.Limiter(sr, threshold_db=-25 - i, release_ms=300.0)] for i in range(4)]
    clips = [aug.DeviceClip(r, bursts(3000 + 501 * i, 60 + i, sr)) for i in range(4)]
    want = [aug.run_chain(aug.DeviceClip(r, bursts(3000 + 501 * i, 60 + i, sr)), fxs[i], False).host() for i in range(4)]
    calls = []
    real = r.lib.call

    def counting(name, *args):
        calls.append((name, args))
        return real(name, *args)

    monkeypatch.setattr(r.lib, "call", counting)
    done = aug.run_chains(clips, fxs)
    monkeypatch.setattr(r.lib, "call", real)
    launches = collections.Counter((args[0], args[2]) for name, args in calls if name == "al_fx_batch_launch")
    assert launches == {(_hip.FXB_COMPRESSOR, 2): 1, (_hip.FXB_LIMITER, 2): 1}, launches
    for i, (clip, w) in enumerate(zip(done, want)):
        assert np.array_equal(ke.bits(clip.host()), ke.bits(w)), i


# ----------------------------------------------------------------------------- 9. a reference scene JSON naming both
def run_scene_json(tmp_path):
    here = os.path.join(os.path.dirname(__file__), "golden")
    z = np.load(os.path.join(here, "reference_scene_arrays.npz"))
    meta = json.load(open(os.path.join(here, "reference_scene.json")))
    sr = meta["sample_rate"]
    injected = {
        "event000": [dict(name="Compressor", sample_rate=sr, threshold_db=-30, ratio=4, attack_ms=10.0, release_ms=200.0)],
        "event001": [dict(name="Limiter", sample_rate=sr, threshold_db=-25, release_ms=300.0)],
    }
    for alias, extra in injected.items():
        meta["events"][alias]["augmentations"] = meta["events"][alias]["augmentations"] + extra
    path = tmp_path / "scene_with_dynamics.json"
    path.write_text(json.dumps(meta))
    clips = {a: z[f"clip_{a}"] for a in meta["events"]}
    irs = {m: z[f"irs_{m}"] for m in meta["state"]["microphones"]}
    scene = core.Scene.from_json(str(path), clips, irs)
    assert type(scene.events["event000"].augmentations[-1]).__name__ == "Compressor"
    assert type(scene.events["event001"].augmentations[-1]).__name__ == "Limiter"
    out = scene.generate()
    cols = {"event000": 0, "event001": 1}          # one emitter each, the first two IR columns
    for mic in irs:
        old, new, slots = [], [], []
        for alias, col in cols.items():
            ev = scene.events[alias]
            want_clip = oracle_chain(clips[alias], ev.augmentations)
            want = orc.render_event(want_clip, irs[mic][:, [col], :].astype(np.float64), ev.snr, ref_db=meta["ref_db"],
                                    sr=sr)["spatial"]
            assert_parity(ev.spatial_audio[mic], want, what=(mic, alias))
            old.append(z[f"spatial_{mic}_{alias}"].astype(np.float64))
            new.append(want)
            slots.append((ev.scene_start, ev.scene_end))
        # the reference's scene with the two plain contributions replaced by the oracle-processed ones
        swap = (orc.mix_scene(new, slots, meta["duration"], sr, keep_padded=False)["scene"].astype(np.float64)
                - orc.mix_scene(old, slots, meta["duration"], sr, keep_padded=False)["scene"])
        assert_parity(out[mic], z[f"scene_{mic}"].astype(np.float64) + swap, what=mic)


# ----------------------------------------------------------------------------- 10. one long clip
def run_long(r, kind, n=CLIP_10S, fs=48000):
    x = bursts(n, 77, fs, period=2000)
    args = COMP_ARGS if kind == "compressor" else LIM_ARGS
    fx = aug.Compressor(fs, *args) if kind == "compressor" else aug.Limiter(fs, *args)
    assert_exercised(stages_of(fx, x), what=("long", kind))
    src = ke.dev(r, x)
    dst = r.mem.empty(n)
    call(r, kind, r.mem.ptr(src), r.mem.ptr(dst), n, fs, *args)
    r.mem.synchronize()
    check(np.asarray(r.mem.download(dst))[:n], ref_kind(kind, x, fs, *args), what=("long", kind, n))
