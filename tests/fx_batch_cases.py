"""Scenarios of the batched FX launches (``al_fx_batch_desc_bytes`` / ``al_fx_batch_pack`` / ``al_fx_batch_launch``,
``augmentation.run_chains``, ``core.stage_event_chains``), shared by tests/test_hostemu_fx_batch.py (host emulation) and
tests/test_gpu_fx_batch.py (gfx950 build).  Every scenario takes the renderer ``r`` the package is set to.

The claim under test is equality, not accuracy: workgroup b of a batched launch renders the bits the single-clip entry renders
for job b.  So the reference of scenario 1 is the same jobs run one by one through ``al_fx_sos`` / ``al_fx_chorus`` /
``al_fx_phaser`` / ``al_fx_apply(FX_DEEMPH)``, compared with ``np.array_equal`` on the bit patterns; on top of that every batched
output meets the float64 bound its own case module holds the single-clip output to (tests/filter_fx_cases.py,
tests/delay_mod_fx_cases.py, tests/kernel_edges.py), and every dst is a guarded buffer.

De-emphasis and the 1-sample clip: ``al_fx_apply`` refuses an emphasis filter on fewer than two samples (the extrapolation term
reads x[1]), and the batch refuses what the single-clip entry refuses, so no de-emphasis batch can hold a 1-sample clip.  The
smallest clip that launches, n = 2, stands in its place (as in tests/shake_standalone.py fx_deemph), and the refusal of n = 1 with
its job index is asserted in ``run_refusals``.
"""
import collections
import ctypes as ct
import random

import numpy as np
import pytest
from scipy import signal as sps

from audiblelight_amd import _hip, augmentation as aug, core
from oracle import synth_oracle as orc
from tests import delay_mod_fx_cases as dmc
from tests import filter_fx_cases as ffc
from tests import kernel_edges as ke
from tests import shake_standalone as ss
from tests.conftest import assert_parity, rel_rms

KINDS = {"sos": _hip.FXB_SOS, "chorus": _hip.FXB_CHORUS, "phaser": _hip.FXB_PHASER, "deemph": _hip.FXB_DEEMPH}
SOS_LONG, SOS_SHORT = sorted({n for n, *_ in ss.SOS_ROWS}, reverse=True)     # 50001 (run 64, 4 tiles), 1025 (run 16, 1 tile)


# ----------------------------------------------------------------------------- the jobs of scenario 1
def specs(kind):
    """The jobs of one batch: dicts with n, the input x and the parameters of the single-clip entry.  Lengths from the edge
    lists of the case modules; a 1-sample clip beside the longest (de-emphasis: 2, see the module docstring)."""
    if kind == "sos":      # (n, sections, fs of the section formulas): 1, 3 and 16 sections in one batch
        rows = [(1, 3, 48000), (SOS_LONG, 3, 44100), (17, 1, 48000), (SOS_SHORT, 16, 48000), (SOS_SHORT, 1, 24000)]
        assert ss.sos_geometry(SOS_LONG) == (4, 782) and ss.sos_geometry(SOS_SHORT) == (1, 65)
        return [dict(n=n, x=ke.signal(n, 1000 + n + k), rows=ffc.edge_rows(k, fs), k=k) for n, k, fs in rows]
    if kind == "chorus":   # the feedback rows of shake_standalone.CHORUS_ROWS (n % B != 0, the fs = 16000 row first), and n = 1
        rows = [row for row in ss.CHORUS_ROWS if row[5] > 0] + [(1, 44100, 4.0, 0.3, 7.0, 0.25, 0.8, 0, None)]
        rows = [(n + 6 * (i % 2),) + tuple(rest) for i, (n, *rest) in enumerate(rows)]     # four distinct lengths (rows 1, 3: six samples more)
        assert rows[0][1] == 16000 and all(n % b for n, *_, b in rows[:-1])
        return [dict(n=n, x=ke.signal(n, 700 + n + i), args=(float(fs), rate, depth, centre, fb, mix))
                for i, (n, fs, rate, depth, centre, fb, mix, _, _) in enumerate(rows)]
    if kind == "phaser":   # 1, 5, run 4 with a last run of 3 samples, run 16 with a last run of 2 samples
        rows = [(1, 48000, 8.0, 0.9, 900.0, 0.7, 0.6), (ss.PHASER_ROWS[2][0], 44100, 2.2, 0.8, 1300.0, 0.0, 0.5),
                (5, 16000, 10.0, 1.0, 260.0, 0.85, 1.0), (ss.PHASER_ROWS[0][0], 48000, 5.5, 0.6, 6500.0, 0.7, 0.7)]
        assert rows[1][0] % 4 and rows[3][0] % 4
        return [dict(n=n, x=ke.signal(n, 800 + n), args=(float(fs), rate, depth, fc, fb, mix)) for n, fs, rate, depth, fc, fb, mix in rows]
    assert kind == "deemph"    # 1024 runs of ceil(n / 1024): 2 live runs; run 2, the last of 1 sample; run 49, the last of 21; run 1
    out = []
    for n, c in ((2, 0.97), (50001, 0.9), (1025, 0.97), (1023, 0.5)):
        x = ke.signal(n, 2 + n)
        x[:2] = (0.875, -0.625)     # kernel_edges.run_fx_deemphasis: the extrapolation term as large as the signal
        out.append(dict(n=n, x=x, c=float(np.float32(c))))
    return out


def check_float64(kind, spec, got):
    """The bound the kind's case module asserts on the single-clip output, on a batched one."""
    x64 = spec["x"].astype(np.float64)
    if kind == "sos":       # filter_fx_cases.run_sos_edges
        rows, k = spec["rows"], spec["k"]
        want = sps.sosfilt(rows / rows[:, 3:4], x64)
        ke.record("batched sos cascade", ke.peak_error(got, want), 1e-6 * k)
        if spec["n"] >= 64:
            assert rel_rms(got, want) <= 1e-6 * k
    elif kind == "chorus":  # delay_mod_fx_cases.run_chorus_case
        dmc.check(got, dmc.ref_chorus(spec["x"], *spec["args"]), what=("batched chorus", spec["n"]))
    elif kind == "phaser":  # delay_mod_fx_cases.run_phaser_case
        dmc.check(got, dmc.ref_phaser(spec["x"], *spec["args"]), what=("batched phaser", spec["n"]))
    else:                   # kernel_edges.run_fx_deemphasis
        c = spec["c"]
        ref = orc.fx_deemphasis(spec["x"], c)
        ke.record("batched fx_deemphasis (err/peak * (1-c) / eps)", ke.peak_error(got, ref) * (1 - c) / ke.EPS, 2.0)
        assert_parity(got, ref, what=("batched deemphasis", spec["n"]))


# ----------------------------------------------------------------------------- the two ways to run a job
def buffers(r, spec, in_place, shift):
    """(src pointer, guarded dst, keep-alive)"""
    out = ke.Guarded(r, spec["n"], shift=shift, init=spec["x"] if in_place else None)
    if in_place:
        return out.ptr, out, None
    src = ke.dev(r, spec["x"])
    return r.mem.ptr(src), out, src


def run_single(r, kind, spec, in_place=False, shift=0):
    """One job through the single-clip entry into a guarded buffer."""
    src, out, _keep = buffers(r, spec, in_place, shift)
    if kind == "sos":
        rows = np.ascontiguousarray(spec["rows"])
        r.lib.call("al_fx_sos", src, out.ptr, spec["n"], rows.ctypes.data, len(rows), r.mem.stream())
    elif kind == "deemph":
        ke.fx(r, _hip.FX_DEEMPH, src, out.ptr, spec["n"], spec["c"])
    else:
        r.lib.call("al_fx_chorus" if kind == "chorus" else "al_fx_phaser", src, out.ptr, spec["n"], *spec["args"], r.mem.stream())
    return out.get()


def job_array(kind, jobs):
    """The public job structs of ``kind`` from [(src, dst, n, spec)]; returns (array, keep-alive)."""
    arr = (_hip.FXB_JOBS[KINDS[kind]] * max(len(jobs), 1))()
    keep = []
    for job, (src, dst, n, spec) in zip(arr, jobs):
        job.src, job.dst, job.n = src, dst, n
        if kind == "sos":
            keep.append(np.ascontiguousarray(spec["rows"], dtype=np.float64))
            job.sos, job.n_sections = keep[-1].ctypes.data, spec.get("n_sections", len(keep[-1]))
        elif kind == "deemph":
            job.coef = spec["c"]
        else:
            job.fs, job.rate_hz, job.depth, job.centre, job.feedback, job.mix = spec["args"]
    return arr, keep


def pack(r, kind, jobs, count=None):
    """al_fx_batch_pack of [(src, dst, n, spec)]; the packed host table."""
    arr, _keep = job_array(kind, jobs)
    count = len(jobs) if count is None else count
    per = r.lib.call("al_fx_batch_desc_bytes", KINDS[kind])
    assert per > 0 and per % 8 == 0
    table = np.zeros(max(count, 1) * per, dtype=np.uint8)
    r.lib.call("al_fx_batch_pack", KINDS[kind], ct.cast(arr, ct.c_void_p), count, table.ctypes.data)
    return table


def run_batch(r, kind, batch, in_place=False):
    """The jobs as ONE launch; the outputs in job order (guards checked)."""
    bufs = [buffers(r, spec, in_place, shift=i % 2) for i, spec in enumerate(batch)]
    table = pack(r, kind, [(src, out.ptr, spec["n"], spec) for (src, out, _), spec in zip(bufs, batch)])
    device_table = r.mem.upload(table)
    r.lib.call("al_fx_batch_launch", KINDS[kind], r.mem.ptr(device_table), len(batch), r.mem.stream())
    return [out.get() for _, out, _ in bufs]


_singles = {}


def singles(r, kind, in_place=False):
    """The jobs of ``specs(kind)`` one by one, computed once per library."""
    key = (r.lib.path, kind, in_place)
    if key not in _singles:
        _singles[key] = [run_single(r, kind, spec, in_place, shift=i % 2) for i, spec in enumerate(specs(kind))]
    return _singles[key]


# ----------------------------------------------------------------------------- 1. a batch equals the single-clip launches
def run_batch_equals_singles(r, kind, in_place=False):
    batch = specs(kind)
    assert len(batch) >= 4 and len({s["n"] for s in batch}) >= 4
    assert min(s["n"] for s in batch) == (2 if kind == "deemph" else 1) and max(s["n"] for s in batch) <= 50001
    want = singles(r, kind, in_place)
    got = run_batch(r, kind, batch, in_place)
    for i, (g, w, spec) in enumerate(zip(got, want, batch)):
        ke.assert_bits_equal(g, w, (kind, "job", i, spec["n"]))
        assert np.array_equal(ke.bits(g), ke.bits(w))
        check_float64(kind, spec, g)
    return got


def run_batch_of_one(r, kind, index=2):
    spec = specs(kind)[index]
    got, = run_batch(r, kind, [spec])
    ke.assert_bits_equal(got, singles(r, kind)[index], (kind, "count == 1"))
    check_float64(kind, spec, got)


# ----------------------------------------------------------------------------- 2. refusals
def run_refusals(r):
    lib = r.lib
    n = 256
    poison = np.full(n, 0.625, dtype=np.float32)
    x = ke.dev(r, ffc.noise(4 * n, 3))
    xp = r.mem.ptr(x)
    outs = [ke.Guarded(r, n, init=poison) for _ in range(3)]
    ok_rows = np.array([[0.2, 0.3, 0.1, 1.0, -0.5, 0.2]])
    good = {"sos": dict(rows=ok_rows), "chorus": dict(args=(48000.0, 2.0, 0.5, 7.0, 0.5, 0.5)),
            "phaser": dict(args=(48000.0, 2.0, 0.5, 1000.0, 0.5, 0.5)), "deemph": dict(c=0.97)}

    def refused(kind, jobs, match, job=None, count=None):
        with pytest.raises(_hip.HipError, match=match):
            pack(r, kind, jobs, count)
        err = lib.last_error()
        assert err.startswith("al_fx_batch_pack: "), err
        if job is not None:
            assert f"job {job}: " in err, err
        return err

    def single_error(kind, src, dst, nn, spec):
        """What the single-clip entry says to the same arguments (it refuses: nothing is launched)."""
        with pytest.raises(_hip.HipError):
            if kind == "sos":
                rows = np.ascontiguousarray(spec["rows"], dtype=np.float64)
                lib.call("al_fx_sos", src, dst, nn, rows.ctypes.data, spec.get("n_sections", len(rows)), r.mem.stream())
            elif kind == "deemph":
                ke.fx(r, _hip.FX_DEEMPH, src, dst, nn, spec["c"])
            else:
                lib.call("al_fx_chorus" if kind == "chorus" else "al_fx_phaser", src, dst, nn, *spec["args"], r.mem.stream())
        return lib.last_error()

    def clean(kind, k):
        return (xp + 4 * n * k, outs[k].ptr, n, good[kind])

    # the batch as a whole
    assert lib.call("al_fx_batch_desc_bytes", 0) == -1 and lib.call("al_fx_batch_desc_bytes", 5) == -1
    for kind in KINDS:
        refused(kind, [clean(kind, 0)], "count must be >= 1", count=0)
        refused(kind, [clean(kind, 0)], "count must be >= 1", count=-3)
    arr, _ = job_array("sos", [clean("sos", 0)])
    table = np.zeros(4096, dtype=np.uint8)
    for bad_kind in (0, 5, -1):
        with pytest.raises(_hip.HipError, match="unknown kind"):
            lib.call("al_fx_batch_pack", bad_kind, ct.cast(arr, ct.c_void_p), 1, table.ctypes.data)
        with pytest.raises(_hip.HipError, match="unknown kind"):
            lib.call("al_fx_batch_launch", bad_kind, xp, 1, r.mem.stream())
    with pytest.raises(_hip.HipError, match="null pointer"):
        lib.call("al_fx_batch_pack", _hip.FXB_SOS, None, 1, table.ctypes.data)
    with pytest.raises(_hip.HipError, match="null pointer"):
        lib.call("al_fx_batch_pack", _hip.FXB_SOS, ct.cast(arr, ct.c_void_p), 1, None)
    for args in ((None, 1), (xp, 0), (xp, -1)):
        with pytest.raises(_hip.HipError, match="needs a table and count >= 1"):
            lib.call("al_fx_batch_launch", _hip.FXB_PHASER, *args, r.mem.stream())

    # anything the single-clip entry refuses: bad job 2 of 3 (and once job 0), with the single-clip entry's own words
    def bad_jobs(kind):
        src, dst = xp + 4 * n * 2, outs[2].ptr
        g = good[kind]
        yield None, dst, n, g
        yield src, None, n, g
        yield src, dst, 0, g
        if kind == "sos":
            yield src, dst, n, dict(rows=ok_rows, n_sections=0)
            yield src, dst, n, dict(rows=np.repeat(ok_rows, 17, 0))
            yield src, dst, n, dict(rows=[[1.0, 0.0, 0.0, 0.0, 0.5, 0.0]])                        # a0 == 0
            yield src, dst, n, dict(rows=[[1.0, np.nan, 0.0, 1.0, 0.5, 0.0]])
            yield src, dst, n, dict(rows=[[1.0, 0.0, 0.0, 1e-320, 0.5, 0.0]])                     # non-finite after the division
            yield src, dst, n, dict(rows=np.concatenate([ok_rows, [[1.0, 0.0, 0.0, 1.0, -1.0, 0.0]]]))   # section 1: pole at z = 1
        elif kind == "deemph":
            yield src, src, n, g             # out of place only
            yield src, dst, 1, g             # the extrapolation term needs x[1]
        else:
            yield src, src + 8, n, g         # dst overlaps src
            for i in range(6):
                for bad in (float("nan"), float("inf"), -1.0):
                    args = list(g["args"])
                    args[i] = bad
                    yield src, dst, n, dict(args=tuple(args))
            yield src, dst, n, dict(args=g["args"][:4] + (1.0, 0.5))                              # feedback >= 1
            yield src, dst, n, dict(args=((999.0 if kind == "chorus" else 40.0),) + g["args"][1:])  # fs out of range

    for kind in KINDS:
        for bad in bad_jobs(kind):
            said = single_error(kind, *bad)
            assert said and "al_fx_batch_pack" not in said
            err = refused(kind, [clean(kind, 0), clean(kind, 1), bad], "job 2", job=2)
            assert err == f"al_fx_batch_pack: job 2: {said}", (err, said)
        first = next(iter(bad_jobs(kind)))
        refused(kind, [first, clean(kind, 1)], "job 0", job=0)

    # a Chorus without feedback belongs to the grid-wide kernel
    ff = dict(args=good["chorus"]["args"][:4] + (0.0, 0.5))
    err = refused("chorus", [clean("chorus", 0), (xp + 4 * n, outs[1].ptr, n, ff)], "feedback == 0", job=1)
    assert "grid-wide" in err

    # a dst range that overlaps the src or dst range of ANOTHER job
    for kind in KINDS:
        g = good[kind]
        base = outs[0].ptr
        a, b = (xp, base, n, g), (xp + 4 * n, outs[1].ptr, n, g)
        refused(kind, [a, (base, outs[1].ptr, n, g)], "dst overlaps src or dst of job 1", job=0)      # dst 0 is src 1
        refused(kind, [a, (xp + 4 * n, base, n, g)], "dst overlaps src or dst of job 1", job=0)       # the same dst twice
        # the last two samples only: as another job's dst, as another job's src
        refused(kind, [a, b, (xp + 8 * n, base + 4 * (n - 2), 2, g)], "dst overlaps src or dst of job 2", job=0)
        refused(kind, [b, a, (base + 4 * (n - 2), outs[2].ptr, 2, g)], "dst overlaps src or dst of job 2", job=1)
    # SOS: in place within a job is allowed, the same buffer in two jobs is not
    inplace = (outs[0].ptr, outs[0].ptr, n, good["sos"])
    refused("sos", [inplace, inplace], "dst overlaps src or dst of job 1", job=0)
    assert len(pack(r, "sos", [inplace, (outs[1].ptr, outs[1].ptr, n, good["sos"])])) > 0
    # adjacent ranges are accepted: dst 0 ends where src 1 begins
    big = ke.dev(r, np.zeros(4 * n, np.float32))
    bp = r.mem.ptr(big)
    for kind in KINDS:
        g = good[kind]
        assert len(pack(r, kind, [(bp, bp + 4 * n, n, g), (bp + 8 * n, bp + 12 * n, n, g)])) > 0
    # nothing was launched: every dst still holds what it held, guards included
    r.mem.synchronize()
    for out in outs:
        ke.assert_bits_equal(out.get(), poison, "a refused batch wrote")


# ----------------------------------------------------------------------------- 3. run_chains against the per-event loop
SR = 16000
CLIP_LENS = (3201, 4507, 5333, 6100, 7019, 7999)     # 0.2 .. 0.5 s at 16 kHz


def chains(sr=SR):
    return [
        [aug.Phaser(sr, rate_hz=1.5, depth=0.7, centre_frequency_hz=900.0, feedback=0.6, mix=0.5)],
        [aug.HighShelfFilter(sr, gain_db=6.0, cutoff_frequency_hz=3000.0, q=0.7),
         aug.Phaser(sr, rate_hz=3.0, depth=0.9, centre_frequency_hz=2100.0, feedback=0.0, mix=0.35)],
        [aug.TimeWarpReverse(sr, fps=10.0, prob=0.5),
         aug.Chorus(sr, rate_hz=2.0, depth=0.5, centre_delay_ms=6.0, feedback=0.5, mix=0.4),
         aug.TimeWarpSilence(sr, fps=7.0, prob=0.5)],
        [aug.TimeWarpDuplicate(sr, fps=5.0, prob=0.5)],
        [aug.Gain(sr, gain_db=-3.5),
         aug.MultibandEqualizer(sr, n_bands=3, gain_db=[6.0, -12.0, 9.0], cutoff_frequency_hz=[500.0, 1800.0, 3500.0], q=[0.7, 0.3, 1.0]),
         aug.Deemphasis(sr, coef=0.9)],
        [aug.Chorus(sr, rate_hz=3.3, depth=0.7, centre_delay_ms=12.5, feedback=0.0, mix=0.4),
         aug.LowpassFilter(sr, cutoff_frequency_hz=0)],
    ]


# what the chains above imply: wave 1 holds e1's shelf and e4's equaliser, e2's chorus, e0's phaser; wave 2 e1's phaser and e4's
# de-emphasis.  One launch per (wave, kind), written as {(kind, jobs in the launch): launches}
EXPECTED_LAUNCHES = {(_hip.FXB_SOS, 2): 1, (_hip.FXB_CHORUS, 1): 1, (_hip.FXB_PHASER, 1): 2, (_hip.FXB_DEEMPH, 1): 1}


def raw_clips():
    return [ffc.noise(n, 40 + i) * np.float32(0.5) for i, n in enumerate(CLIP_LENS)]


def seed_all(seed=1234):
    random.seed(seed)
    np.random.seed(seed)


def per_event_loop(clips, chain_list, normalize=False):
    return [aug.run_chain(clip, chain, normalize) for clip, chain in zip(clips, chain_list)]


def count_calls(r, monkeypatch):
    calls = []
    real = r.lib.call

    def counting(name, *args):
        calls.append((name, args))
        return real(name, *args)

    monkeypatch.setattr(r.lib, "call", counting)
    return calls


def run_chains_equal_the_loop(r, monkeypatch):
    fxs, raws = chains(), raw_clips()
    seed_all()
    want = [clip.host() for clip in per_event_loop([aug.DeviceClip(r, raw) for raw in raws], fxs)]
    after_loop = random.random()
    calls = count_calls(r, monkeypatch)
    seed_all()
    clips = [aug.DeviceClip(r, raw) for raw in raws]
    done = aug.run_chains(clips, fxs)
    ran = list(calls)
    assert [c is d for c, d in zip(clips, done)] == [True] * 6
    assert random.random() == after_loop        # the same number of draws, from the same state
    for i, (clip, w) in enumerate(zip(done, want)):
        assert clip.n == CLIP_LENS[i]
        assert np.array_equal(ke.bits(clip.host()), ke.bits(w)), i
        assert clip.uploads == 1
    names = collections.Counter(name for name, _ in ran)
    launches = collections.Counter((args[0], args[2]) for name, args in ran if name == "al_fx_batch_launch")
    assert launches == EXPECTED_LAUNCHES, launches
    assert names["al_fx_batch_pack"] == names["al_fx_batch_launch"] == 5
    assert names["al_fx_phaser"] == 0 and names["al_fx_sos"] == 0
    assert names["al_fx_chorus"] == 1                                     # feedback 0: its grid-wide launch
    chorus_args, = [args for name, args in ran if name == "al_fx_chorus"]
    assert chorus_args[7] == 0.0
    ops = [args[0] for name, args in ran if name == "al_fx_apply"]
    assert sorted(ops) == [_hip.FX_GAIN, _hip.FX_GAIN]                    # Gain, and the low-pass at cutoff 0 as its one pointwise launch
    assert names["al_fx_frame_shuffle"] == 3


# ----------------------------------------------------------------------------- 4. a scene through stage_event_chains
def render_scene(r):
    rng = np.random.default_rng(9)
    C, L = 3, 500
    fxs, raws = chains(), raw_clips()
    irs = (rng.standard_normal((C, len(raws), L)) * np.exp(-np.arange(L) / 100.0)).astype(np.float32)
    scene = core.Scene(1.5, core.StaticIRState({"mic000": irs}), sample_rate=SR, ref_db=-65)
    for i, (x, c) in enumerate(zip(raws, fxs)):
        scene.add_event(core.Event(f"e{i}", x, SR, snr=8.0 + i, scene_start=0.15 * i, augmentations=c))
    seed_all()
    out = scene.generate()
    return scene, np.array(out["mic000"])


def run_scene_equals_the_loop(r, monkeypatch):
    calls = count_calls(r, monkeypatch)
    scene, got = render_scene(r)
    launches = collections.Counter((args[0], args[2]) for name, args in calls if name == "al_fx_batch_launch")
    assert launches == EXPECTED_LAUNCHES, launches
    for ev in scene.events.values():
        clip = ev._last_chain
        assert clip is not None and clip.uploads == 1 and clip.downloads == 0
    monkeypatch.setattr(aug, "run_chains", per_event_loop)
    del calls[:]
    _, want = render_scene(r)
    assert not [name for name, _ in calls if name.startswith("al_fx_batch")]
    assert got.shape == want.shape and np.array_equal(ke.bits(got), ke.bits(want))
