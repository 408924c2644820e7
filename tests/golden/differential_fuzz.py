#!/usr/bin/env python
"""Differential fuzz against the REAL reference (build container only: /root/reference does not exist on the GPU box).

Random small scenes -- static, moving and zero-emitter events, snr drawn from {0, negative, U(5, 30)}, some clips and IRs all
zeros, events running past the scene end or not reaching it, an optional coloured-noise ambience -- are rendered twice from the
same duck-typed objects: by the reference's own ``render_audio_for_all_scene_events`` + ``generate_scene_audio_from_events``
(numpy / scipy, imported from /root/reference exactly as tests/golden/make_golden.py does) and by this package's functions of
the same names over the host-emulated kernels (the unmodified kernel sources compiled for the CPU; the gfx950 build runs the
same scenes in the GPU suite through the oracle).  Every event's ``spatial_audio`` and every ``scene.audio`` must agree within
the contract's bound (1e-4 relative RMS and max-abs / max|ref|) AND carry the reference's dtype (a float32 clip tiled over the
capsules stays float32, synthesize.py:572-599); silent results must be silent on both sides.

    python tests/golden/differential_fuzz.py [FIRST LAST]        (default 0 200; prints the worst case, exit code 1 on a failure)

The reference's side can be stored and replayed without the reference (what tests/test_dropin_reference.py does):

    python tests/golden/differential_fuzz.py --record tests/golden/reference_fuzz_vectors.npz 0 25   (needs the reference)
    python tests/golden/differential_fuzz.py --replay tests/golden/reference_fuzz_vectors.npz 0 25   (this package alone)

``--record`` keeps, for every array the reference returned, a compact record under ``"<seed>|<scene or fx>|<what>"``: shape, dtype,
rms and max|x|, fixed samples and random-sign projections of the whole array (see ``summarize``; an array of at most SAMPLES
values is kept whole).  ``--replay`` builds the same seeded inputs, renders them with this package only (ambiences drawn by its
own ``Ambience``, which takes the reference's seeded host draws) and checks them against those records under the same bound and
dtype rule; a case missing on either side fails.
"""
import copy
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (the reference import machinery and the duck-typed FakeEvent)


def random_scene(seed, amb_mod):
    rng = np.random.default_rng(70_000 + seed)
    sr = int(rng.choice([8000, 16000]))
    n_caps = int(rng.integers(1, 5))
    dur = float(rng.uniform(0.6, 1.6))
    lir = int(rng.integers(40, 1500))
    events, irs = {}, []
    for i in range(int(rng.integers(1, 6))):
        kind = rng.choice(["static", "static", "static", "moving", "tiled"])
        n = int(rng.integers(700 if kind == "moving" else 30, 7000))
        ne = {"static": 1, "tiled": 0, "moving": int(rng.integers(2, 6))}[kind]
        a = mg.make_clip(rng, n)
        if rng.random() < 0.12:
            a = np.zeros_like(a)                                    # a silent clip
        h = mg.make_irs(rng, n_caps, ne, lir) if ne else np.zeros((n_caps, 0, lir))
        if ne and rng.random() < 0.12:
            h[:, int(rng.integers(0, ne)), :] = 0.0                  # an all-zero IR (one emitter of a moving event, or the static one)
        snr = float(rng.choice([0.0, -float(rng.uniform(1, 10)), float(rng.uniform(5, 30)), float(rng.uniform(5, 30))]))
        start = float(rng.uniform(-0.05, dur * 1.02))               # some start before 0, some at or beyond the scene's end
        if seed >= 100_000:     # the adversarial range: clips that are not peak-normalised, IRs far from unit scale, slots on half samples
            a = (a * float(rng.choice([1.0, 1.0, 1e-6, 1e-20, 3e5]))).astype(np.float32)
            h = h * float(rng.choice([1.0, 1.0, 1e-8, 1e4]))
            h = h.astype(np.float32).astype(np.float64)
            if rng.random() < 0.5:
                start = (int(rng.integers(0, int(dur * sr))) + 0.5) / sr     # round-half-even on both slot ends (synthesize.py:361-362)
        # (no dry render for snr = 0: the reference scales it by db_to_multiplier(., mean|0|) = 10^(dB/20) / tiny, i.e. to 1e305 in
        # float64 -- its own output is overflow-scale garbage there, and nothing a float32 path could or should reproduce)
        dry = ne == 1 and snr != 0.0 and rng.random() < 0.25
        events[f"ev{i}"] = mg.FakeEvent(f"ev{i}", a, ne, snr, sr, scene_start=start, is_moving=ne > 1,
                                        ref_ir_channel=int(rng.integers(0, n_caps)) if dry else None,
                                        direct_path_time_ms=[2, 25] if dry else None)
        irs.append(h)
    mic_ir = np.concatenate(irs, axis=1)
    if mic_ir.shape[1] == 0:                                        # the reference refuses a WorldState without emitters
        return None
    # dtypes the reference's arithmetic keeps or widens (a generator of its own: the scenes of earlier records stay the same):
    # float32 IRs (static renders and dry renders stay float32), the odd float64 clip (a tiled clip stays float64)
    drng = np.random.default_rng(90_000 + seed)
    if drng.random() < 0.3:
        mic_ir = mic_ir.astype(np.float32)
    for ev in events.values():
        if drng.random() < 0.15:
            ev._audio = ev._audio.astype(np.float64)
    noise = rng.choice([None, None, "white", "pink", 1.5])
    ambience = {}
    if noise is not None:
        ambience["a0"] = amb_mod.Ambience(channels=n_caps, duration=dur, alias="a0", noise=noise if isinstance(noise, str) else float(noise),
                                          ref_db=float(-rng.uniform(40, 70)), sample_rate=sr)
    state = types.SimpleNamespace(irs={"mic000": mic_ir}, get_irs=lambda: {"mic000": mic_ir}, simulate=lambda: None,
                                  microphones={"mic000": object()}, num_emitters=mic_ir.shape[1], name="fake")
    return types.SimpleNamespace(state=state, events=events, ambience=ambience, audio={}, ref_db=float(-rng.uniform(50, 70)), duration=dur,
                                 sample_rate=sr)


def fx_and_noise_outputs(seed, aug, amb):
    """[(label, output)] for one seed, computed by ONE side (``aug`` / ``amb``: the reference's modules or this package's): the
    sample-wise FX the reference implements itself in numpy (Fade with random shapes and lengths incl. fades longer than the clip,
    Invert, Reverse, the four TimeWarp classes under the same Python random seed) and powerlaw_psd_gaussian for a random exponent /
    length / fmin / seed (augmentation.py:1403-1790, ambience.py:271-375)."""
    import random

    rng = np.random.default_rng(80_000 + seed)
    sr = int(rng.choice([8000, 16000, 22050]))
    x = mg.make_clip(rng, int(rng.integers(300, 9000)))
    out = []
    shapes = list(aug.Fade.FADE_SHAPES)
    a, b = rng.choice(shapes), rng.choice(shapes)
    la, lb = float(rng.choice([0.0, rng.uniform(0.01, 0.4), 3.0])), float(rng.choice([0.0, rng.uniform(0.01, 0.4), 3.0]))
    kw = dict(sample_rate=sr, fade_in_len=la, fade_out_len=lb, fade_in_shape=str(a), fade_out_shape=str(b))
    out.append((f"Fade{a, b, round(la, 3), round(lb, 3)}", aug.Fade(**kw)(x)))
    out.append(("Invert", aug.Invert(sample_rate=sr)(x)))
    out.append(("Reverse", aug.Reverse(sample_rate=sr)(x)))
    name = str(rng.choice(["TimeWarpSilence", "TimeWarpDuplicate", "TimeWarpRemove", "TimeWarpReverse"]))
    fps, prob = float(rng.uniform(1.5, 12.0)), float(rng.uniform(0.05, 1.0))
    random.seed(seed)
    out.append((f"{name}(fps={fps:.2f}, prob={prob:.2f})", getattr(aug, name)(sample_rate=sr, fps=fps, prob=prob)(x)))
    beta = float(rng.choice([0.0, 1.0, 2.0, -1.0, rng.uniform(-2, 3)]))
    n = int(rng.choice([rng.integers(8, 5000), 4096, 1000, 2 * 3 * 5 * 7 * 11, 4001]))
    fmin = float(rng.choice([0.0, 0.0, rng.uniform(0.0, 0.5)]))
    shape = (int(rng.integers(1, 4)), n)
    sd = int(rng.integers(0, 10_000))
    out.append((f"powerlaw(beta={beta:.2f}, n={n}, fmin={fmin:.3f})", amb.powerlaw_psd_gaussian(beta, shape, fmin=fmin, seed=sd)))
    return out


def fx_and_noise_cases(seed, ref_aug, ref_amb, our_aug, our_amb):
    """[(label, ours, reference's)] for one seed: fx_and_noise_outputs of both sides on the same draws."""
    theirs = fx_and_noise_outputs(seed, ref_aug, ref_amb)
    mine = fx_and_noise_outputs(seed, our_aug, our_amb)
    return [(what, got, ref) for (what, got), (_, ref) in zip(mine, theirs)]


SMOOTH = sorted({2 ** a * 3 ** b * 5 ** c * 7 ** d for a in range(11) for b in range(4) for c in range(3) for d in range(2)
                 if 32 <= 2 ** a * 3 ** b * 5 ** c * 7 ** d <= 1024})


def geometry_output(seed, syn):
    """One moving event under a random STFT geometry the reference accepts (win >= hop, fft <= 2*hop + win; ANY fft size -- half the
    seeds draw a product of 2, 3, 5, 7, the other half any integer, primes included: Bluestein), rendered by ``syn``'s
    render_event_audio, the reference's or ours (synthesize.py:507-608,277-310): (label, spatial audio)."""
    rng = np.random.default_rng(85_000 + seed)
    hop = int(rng.integers(16, 200))
    win = int(rng.integers(hop, 3 * hop + 1))
    ok = [f for f in SMOOTH if f <= 2 * hop + win]
    fft = int(rng.choice(ok[-10:])) if rng.random() < 0.7 else int(rng.choice(ok))
    if seed % 2:                                                    # any size at all (a generator of its own: the other draws stay)
        fft = int(np.random.default_rng(86_000 + seed).integers(max(32, (2 * hop + win) // 3), min(1024, 2 * hop + win) + 1))
    n_irs, n_caps, sr = int(rng.integers(2, 6)), int(rng.integers(1, 4)), 8000
    a, h = mg.make_clip(rng, int(rng.integers(1500, 6000))), mg.make_irs(rng, n_caps, n_irs, int(rng.integers(100, 1200)))
    snr = float(rng.uniform(5, 30))
    ev = mg.FakeEvent("g", a, n_irs, snr, sr, is_moving=True)
    syn.render_event_audio(ev, h, "mic000", ref_db=-60, fft_size=fft, win_size=win, hop_size=hop)
    return f"moving event, fft/win/hop = {fft}/{win}/{hop}", ev.spatial_audio["mic000"]


def geometry_case(seed, ref_syn, ours):
    """(label, ours, reference's): geometry_output of both sides on the same draws."""
    what, ref = geometry_output(seed, ref_syn)
    return what, geometry_output(seed, ours)[1], ref


def errors(got, ref):
    if np.asarray(got).dtype != np.asarray(ref).dtype:      # a drop-in hands back the reference's dtype, not only its values
        return float("inf"), float("inf")
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if got.shape != ref.shape:
        return float("inf"), float("inf")
    if not np.isfinite(got).all():
        return float("inf"), float("inf")
    peak, rms = np.abs(ref).max() if ref.size else 0.0, np.sqrt(np.mean(ref ** 2)) if ref.size else 0.0
    if peak == 0:
        worst = float(np.abs(got).max()) if got.size else 0.0
        return worst, worst
    return float(np.sqrt(np.mean((got - ref) ** 2)) / rms), float(np.abs(got - ref).max() / peak)


# ----------------------------------------------------------------------------- the reference's arrays, stored compactly
# --record keeps, per array, its shape and dtype, float64 [rms, max|x|], SAMPLES values at fixed stratified positions (all of
# them for a small array) and SKETCH_ROWS random-sign projections of the whole array.  For signs r, E[(r . d)^2] = |d|^2: the
# projections of (ours - reference's) estimate the relative RMS error over EVERY sample, 32 rows to within a small factor -- the
# contract's bound is 1e-4, observed errors are below 1e-6.  The max-abs half is checked on the samples and on max|x| itself.
# Positions and signs come from an integer hash (splitmix64), not from a numpy generator, so they are the same on any numpy.
SAMPLES, SKETCH_ROWS = 256, 32


def _mix64(x):
    x = x.astype(np.uint64)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def sample_positions(n):
    """SAMPLES flat positions, one drawn in each of SAMPLES equal strata of [0, n) (every position when n <= SAMPLES)."""
    if n <= SAMPLES:
        return np.arange(n, dtype=np.int64)
    k = np.arange(SAMPLES, dtype=np.int64)
    lo, hi = k * n // SAMPLES, (k + 1) * n // SAMPLES
    return lo + (_mix64(k + 0x5EED) % (hi - lo).astype(np.uint64)).astype(np.int64)


def sketch(x):
    """SKETCH_ROWS projections of the flattened array on pseudo-random +-1 vectors (float64)."""
    flat = np.asarray(x, dtype=np.float64).ravel()
    idx = np.arange(flat.size, dtype=np.uint64)
    return np.array([np.dot(1.0 - 2.0 * (_mix64(idx + np.uint64((j + 1) << 40)) >> np.uint64(63)).astype(np.float64), flat)
                     for j in range(SKETCH_ROWS)])


def summarize(arr):
    """{field: array} kept for one of the reference's arrays (see above)."""
    arr = np.asarray(arr)
    x = arr.astype(np.float64).ravel()
    stats = [float(np.sqrt(np.mean(x ** 2))), float(np.abs(x).max())] if x.size else [0.0, 0.0]
    out = {"shape": np.array(arr.shape, dtype=np.int64), "stats": np.array(stats), "values": arr.ravel()[sample_positions(arr.size)]}
    if arr.size > SAMPLES:
        out["sketch"] = sketch(arr)
    return out


def stored_errors(got, ref):
    """errors() against a summarize() record: exact where the whole array is stored, else the sketch's relative RMS estimate and
    the largest deviation over the samples and of max|x|, relative to the reference's max|x|."""
    got = np.asarray(got)
    if got.dtype != ref["values"].dtype or got.shape != tuple(int(v) for v in ref["shape"]) or not np.isfinite(got).all():
        return float("inf"), float("inf")
    if "sketch" not in ref:
        return errors(got, ref["values"].reshape(got.shape))
    rms, peak = (float(v) for v in ref["stats"])
    g = got.astype(np.float64).ravel()
    if peak == 0:
        worst = float(np.abs(g).max())
        return worst, worst
    est = float(np.sqrt(np.mean((sketch(g) - ref["sketch"]) ** 2) / g.size)) / rms
    dev = max(float(np.abs(g[sample_positions(g.size)] - ref["values"].astype(np.float64)).max()), abs(float(np.abs(g).max()) - peak))
    return est, dev / peak


def ref_peak(ref):
    if isinstance(ref, dict):
        return float(ref["stats"][1])
    ref = np.asarray(ref)
    return float(np.abs(ref).max()) if ref.size else 0.0


def scene_arrays(scene):
    """[(what, array)]: everything a rendered scene hands back -- the scene, every event's spatial audio, its dry render where it has
    one and its full-scene padded copy where it keeps one."""
    out = [("scene", scene.audio["mic000"])]
    for k, ev in scene.events.items():
        out.append((k, ev.spatial_audio["mic000"]))
        if ev.ref_ir_channel is not None:
            out.append((k + ".dry", ev._spatial_audio_dry["mic000"]))
        if "mic000" in ev._spatial_audio_padded:
            out.append((k + ".padded", ev._spatial_audio_padded["mic000"]))
    return out


def main():
    argv = sys.argv[1:]
    mode, path = "live", None
    if argv and argv[0] in ("--record", "--replay"):
        mode, path, argv = argv[0][2:], argv[1], argv[2:]
    first, last = (int(argv[0]), int(argv[1])) if len(argv) > 1 else (0, 200)
    from audiblelight_amd import _hip, ambience as our_amb, augmentation as our_aug, engine, synthesize as ours
    from tests import hostemu                       # this repo's tests package, before the reference tree goes onto sys.path

    if mode == "replay":
        stored = {}                                 # "<seed>|<scene or fx>|<what>" -> summarize() record
        with np.load(path) as z:
            for k in z.files:
                case, _, field = k.rpartition("#")
                if case:
                    stored.setdefault(case, {})[field] = z[k]
    else:
        ref_syn, ref_amb = mg._import_reference()
        import audiblelight.augmentation as ref_aug

        sys.path.insert(0, HERE)
        from make_fx_golden import _frame

        ref_aug.librosa.util.frame = _frame           # librosa is absent: its documented framing, as in make_fx_golden.py
    if mode == "record":
        rec = {}
        for seed in range(first, last):
            a = random_scene(seed, ref_amb)
            if a is not None:
                with np.errstate(all="ignore"):
                    ref_syn.render_audio_for_all_scene_events(a)
                    ref_syn.generate_scene_audio_from_events(a)
                for what, arr in scene_arrays(a):
                    rec.update({f"{seed}|scene|{what}#{k}": v for k, v in summarize(arr).items()})
            for what, arr in fx_and_noise_outputs(seed, ref_aug, ref_amb) + [geometry_output(seed, ref_syn)]:
                rec.update({f"{seed}|fx|{what}#{k}": v for k, v in summarize(arr).items()})
        # the drop-in test's known answers: the reference's scalar helpers and the names its synthesize module defines
        x = np.linspace(-0.5, 0.7, 101)
        rec["dropin|apply_snr(x, 7.0)"] = np.asarray(ref_syn.apply_snr(x, 7.0))
        rec["dropin|db_to_multiplier(-40.0, 0.3)"] = np.asarray(ref_syn.db_to_multiplier(-40.0, 0.3))
        rec["dropin|synthesize_names"] = np.array(sorted(n for n, v in vars(ref_syn).items()
                                                         if isinstance(v, types.FunctionType) and v.__module__ == ref_syn.__name__))
        np.savez_compressed(path, **rec)
        print(f"seeds {first}..{last - 1}: {len({k.split('#')[0] for k in rec})} arrays of the reference summarised in {path} "
              f"({os.path.getsize(path) // 1024} KiB)")
        return 0

    ours.set_renderer(engine.Renderer(lib=_hip.Library(hostemu.build()), memory=hostemu.NumpyMemory()))
    pairs = []                    # (seed, what, ours, reference's, FX / noise / geometry case?); None where a side lacks the case
    for seed in range(first, last):
        if mode == "replay":
            a = random_scene(seed, our_amb)
            want = {k.split("|", 2)[2]: v for k, v in stored.items() if k.startswith(f"{seed}|scene|")}
            got = {}
            if a is not None:
                ours.render_audio_for_all_scene_events(a)
                ours.generate_scene_audio_from_events(a)
                got = dict(scene_arrays(a))
            pairs += [(seed, what, got.get(what), want.get(what), False) for what in sorted(set(want) | set(got))]
            fx = fx_and_noise_outputs(seed, our_aug, our_amb) + [geometry_output(seed, ours)]
            fx_cases = [(what, arr, stored.get(f"{seed}|fx|{what}")) for what, arr in fx]
            fx_cases += [(k.split("|", 2)[2], None, v) for k, v in stored.items()
                         if k.startswith(f"{seed}|fx|") and k.split("|", 2)[2] not in {w for w, _ in fx}]
        else:
            a = random_scene(seed, ref_amb)
            if a is not None:
                b = copy.deepcopy(a)
                b.state.get_irs = lambda irs=b.state.irs: irs
                with np.errstate(all="ignore"):
                    ref_syn.render_audio_for_all_scene_events(a)
                    ref_syn.generate_scene_audio_from_events(a)
                ours.render_audio_for_all_scene_events(b)
                ours.generate_scene_audio_from_events(b)
                mine = dict(scene_arrays(b))
                pairs += [(seed, what, mine[what], ref, False) for what, ref in scene_arrays(a)]
            fx_cases = fx_and_noise_cases(seed, ref_aug, ref_amb, our_aug, our_amb) + [geometry_case(seed, ref_syn, ours)]
        pairs += [(seed, what, got, ref, True) for what, got, ref in fx_cases]
    ours.set_renderer(None)

    worst, bad, n_cmp, n_silent, n_fx = (0.0, None), [], 0, 0, 0
    for seed, what, got, ref, is_fx in pairs:
        n_cmp += 1
        n_fx += is_fx
        if got is None or ref is None:
            rms = mx = float("inf")
        else:
            rms, mx = stored_errors(got, ref) if isinstance(ref, dict) else errors(got, ref)
            n_silent += (not is_fx) and ref_peak(ref) == 0.0
        if max(rms, mx) > worst[0]:
            worst = (max(rms, mx), (seed, what))
        if rms > 1e-4 or mx > 1e-4:
            bad.append((seed, what, rms, mx, None if got is None else str(np.asarray(got).dtype),
                        None if ref is None else str((ref["values"] if isinstance(ref, dict) else np.asarray(ref)).dtype)))
    against = "the reference's own" if mode == "live" else f"the reference's stored in {os.path.basename(path)}"
    print(f"{n_fx} of the arrays are FX / coloured-noise outputs (Fade, Invert, Reverse, TimeWarp*, powerlaw_psd_gaussian) and moving events "
          f"under random STFT geometries")
    print(f"seeds {first}..{last - 1}: {n_cmp} arrays compared with {against} ({n_silent} of them silent), {len(bad)} outside 1e-4; "
          f"worst error {worst[0]:.2e} at {worst[1]}")
    for item in bad[:20]:
        print("FAILED", item)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
