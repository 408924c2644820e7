"""Timing of al_ism_shoebox_src / al_ism_shoebox_bands_src beside the entries they stand for, on the same tensor (DESIGN.md "Shoebox
IRs: directional sources and air", the measured table).  The cfg2-shaped tensor: 32 rows x 64 sources x 96 000 samples at 48 kHz
(786 MB), a 6 x 5 x 3 m room with beta = 0.877; the rows as 32 omnidirectional capsules, as 8 FOA listeners (P = 8, K = 4) and, for
six octave bands with half = 512 (absorption 0.10 .. 0.40 rising with frequency), as 32 capsules.  Each through the old entry and
through the new one with a cardioid of its own on every source and the air of 20 degrees and 50 % (at 4 kHz for the broadband
cases, at the band centres for the bands), with the tail's default mix and fade and, without a tail, at max_order 10.  HIP events
around each call, every case warmed up once, then REPS rounds that go through the cases in turn; the median per case and the spread
(max - min) / median are printed.  The host time of the knot tables of the 64 distinct source patterns is printed too: the quadrature
of tail_envelope runs once per pair of patterns (64 for the omni capsules, 4 x 64 for FOA, 64 x 6 for the bands).

    python profiles/tools/shoebox_source_timing.py [--small]        (--small: 8 rows x 8 sources, to try the script)
"""
import ctypes as ct
import os
import sys
import time

import numpy as np

REPS = 5
ROOM, BETA, FS, IR_LEN, ORDER, HALF = (6.0, 5.0, 3.0), 0.877, 48000.0, 96000, 10, 512
ALPHAS = (0.10, 0.14, 0.18, 0.23, 0.30, 0.40)


def main(small=False):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from audiblelight_amd import engine, shoebox

    n_rows, n_src = (8, 8) if small else (32, 64)
    r = engine.Renderer()
    lib, mem, torch = r.lib, r.mem, r.mem.torch
    rng = np.random.default_rng(0)
    room, betas = np.array(ROOM), np.full(6, BETA)
    band_betas = np.ascontiguousarray(np.repeat(shoebox.betas_from_absorption(ALPHAS)[None, :], 6, axis=0))
    n_bands = band_betas.shape[1]
    sources = rng.uniform(0.15, 0.85, (n_src, 3)) * room
    capsules = rng.uniform(0.15, 0.85, (n_rows, 3)) * room
    foa = np.tile(shoebox.foa_patterns(), (n_rows // 4, 1, 1))
    spats = np.stack([shoebox.cardioid(v) for v in rng.standard_normal((n_src, 3))])
    air = float(shoebox.air_absorption(4000.0))
    band_air = np.ascontiguousarray(shoebox.air_absorption(shoebox.OCTAVE_CENTRES))
    shoebox.check_arguments(room, betas, sources, capsules, IR_LEN, FS, patterns=np.tile(shoebox.omni(), (n_rows, 1, 1)), source_patterns=spats,
                            air=air)
    pitch = shoebox.pitch_of(IR_LEN)
    total = n_rows * n_src * pitch
    mix, fade = shoebox.tail_samples(shoebox.ShoeboxTail(seed=1), room, FS)
    # the knot tables: one per distinct pattern (old entries), one per distinct pair of patterns (new entries)
    omni_env = shoebox.tail_envelope(room, betas, IR_LEN, FS, mix)
    n_knots = len(omni_env)
    foa_env = np.stack([shoebox.tail_envelope(room, betas, IR_LEN, FS, mix, pattern=p) for p in foa[0]])
    band_env = np.stack([shoebox.tail_envelope(room, band_betas[:, b], IR_LEN, FS, mix) for b in range(n_bands)])
    t0 = time.perf_counter()
    omni_src_env = np.stack([shoebox.tail_envelope(room, betas, IR_LEN, FS, mix, source_pattern=sp, air=air) for sp in spats])
    t1 = time.perf_counter()
    foa_src_env = np.stack([[shoebox.tail_envelope(room, betas, IR_LEN, FS, mix, pattern=p, source_pattern=sp, air=air) for sp in spats]
                            for p in foa[0]])
    t2 = time.perf_counter()
    band_src_env = np.stack([[shoebox.tail_envelope(room, band_betas[:, b], IR_LEN, FS, mix, source_pattern=sp, air=band_air[b])
                              for b in range(n_bands)] for sp in spats])
    t3 = time.perf_counter()
    print(f"host time of the knot tables ({n_knots} knots each) for {n_src} distinct source patterns: omni capsules {n_src} tables "
          f"{t1 - t0:.2f} s, FOA {4 * n_src} tables {t2 - t1:.2f} s, {n_bands} bands {n_bands * n_src} tables {t3 - t2:.2f} s", flush=True)
    up = lambda a: mem.upload(np.ascontiguousarray(a, dtype=np.float64).reshape(-1))      # noqa: E731
    src_dev, cap_dev, spat_dev, foa_dev = up(sources), up(capsules), up(spats), up(foa)
    env = dict(omni=up(omni_env), foa=up(np.tile(foa_env, (n_rows // 4, 1))), band=up(band_env),
               omni_src=up(np.broadcast_to(omni_src_env[None], (n_rows, n_src, n_knots))),
               foa_src=up(np.tile(foa_src_env, (n_rows // 4, 1, 1))), band_src=up(band_src_env))
    phi_dev = up(shoebox.band_filters(shoebox.OCTAVE_CENTRES, FS, HALF))
    out = mem.empty(total)
    L, B = room.ctypes.data_as(ct.POINTER(ct.c_double)), betas.ctypes.data_as(ct.POINTER(ct.c_double))
    BB, AA = band_betas.ctypes.data_as(ct.POINTER(ct.c_double)), band_air.ctypes.data_as(ct.POINTER(ct.c_double))
    P, S, C, O, X = mem.ptr(src_dev), mem.ptr(spat_dev), mem.ptr(cap_dev), mem.ptr(out), mem.stream()
    pairs = n_rows * n_src

    def workspace(mix_arg, fade_arg):
        per_pair = lib.call("al_ism_shoebox_bands_workspace_bytes", n_bands, HALF, IR_LEN, mix_arg, fade_arg)
        n = max(1, min(pairs, shoebox.BAND_WORKSPACE_CAP // per_pair))
        return mem.empty(n * per_pair // 8, dtype=np.float64), n * per_pair

    ws_tail, ws_tail_bytes = workspace(mix, fade)
    ws_plain, ws_plain_bytes = workspace(-1, 0)

    def old(kind, tail):
        order, t = (-1, (mix, fade, 1, 0, 0)) if tail else (ORDER, ())
        if kind == "omni":
            return lambda: lib.call("al_ism_shoebox" + "_tail" * tail, P, n_src, C, n_rows, L, B, 343.0, FS, order, IR_LEN, pitch, *t,
                                    *((mem.ptr(env["omni"]), n_knots) if tail else ()), O, X)
        if kind == "foa":
            return lambda: lib.call("al_ism_shoebox_dir" + "_tail" * tail, P, n_src, C, n_rows // 4, mem.ptr(foa_dev), 4, L, B, 343.0, FS, order,
                                    IR_LEN, pitch, *t, *((mem.ptr(env["foa"]), n_knots) if tail else ()), O, X)
        ws, ws_bytes = (ws_tail, ws_tail_bytes) if tail else (ws_plain, ws_plain_bytes)
        return lambda: lib.call("al_ism_shoebox_bands" + "_tail" * tail, P, n_src, C, n_rows, L, BB, n_bands, mem.ptr(phi_dev), HALF, 343.0, FS,
                                order, IR_LEN, pitch, *t, *((mem.ptr(env["band"]), n_knots) if tail else ()), mem.ptr(ws), ws_bytes, O, X)

    def new(kind, tail):
        order, t = (-1, (mix, fade, 1, 0, 0)) if tail else (ORDER, (-1, 0, 0, 0, 0))
        table = (mem.ptr(env[kind + "_src"]), n_knots) if tail else (None, 0)
        if kind == "omni":
            return lambda: lib.call("al_ism_shoebox_src", P, n_src, S, C, n_rows, None, 1, L, B, air, 343.0, FS, order, IR_LEN, pitch, *t, *table,
                                    O, X)
        if kind == "foa":
            return lambda: lib.call("al_ism_shoebox_src", P, n_src, S, C, n_rows // 4, mem.ptr(foa_dev), 4, L, B, air, 343.0, FS, order, IR_LEN,
                                    pitch, *t, *table, O, X)
        ws, ws_bytes = (ws_tail, ws_tail_bytes) if tail else (ws_plain, ws_plain_bytes)
        return lambda: lib.call("al_ism_shoebox_bands_src", P, n_src, S, C, n_rows, L, BB, n_bands, mem.ptr(phi_dev), HALF, AA, 343.0, FS, order,
                                IR_LEN, pitch, *t, *table, mem.ptr(ws), ws_bytes, O, X)

    names = {"omni": f"{n_rows} omni capsules", "foa": f"{n_rows // 4} FOA listeners (K = 4)", "band": f"{n_rows} capsules, {n_bands} bands"}
    cases = []
    for tail, what in ((True, f"tail, mix {mix} fade {fade}"), (False, f"no tail, max_order {ORDER}")):
        for kind in ("omni", "foa", "band"):
            cases += [(f"{names[kind]:26s} old entry  {what}", old(kind, tail)), (f"{names[kind]:26s} new entry  {what}", new(kind, tail))]
    times = {label: [] for label, _ in cases}
    for rep in range(REPS + 1):
        for label, call in cases:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            mem.synchronize()
            a.record(torch.cuda.current_stream(mem.device))
            call()
            b.record(torch.cuda.current_stream(mem.device))
            mem.synchronize()
            if rep > 0:      # the first round warms every case up
                times[label].append(a.elapsed_time(b))
    print(f"tensor {n_rows} x {n_src} x {IR_LEN}, pitch {pitch}: {4 * total / 1e6:.1f} MB; median of {REPS}")
    medians = []
    for label, _ in cases:
        t = np.array(times[label])
        medians.append(float(np.median(t)))
        print(f"{label:72s} {medians[-1]:9.3f} ms   spread {(t.max() - t.min()) / medians[-1] * 100:5.1f} %", flush=True)
    print("new / old: " + ", ".join(f"{cases[i][0].split('  ')[0].strip()} {'tail' if i < 6 else 'order ' + str(ORDER)} "
                                    f"{medians[i + 1] / medians[i]:.3f}" for i in range(0, len(cases), 2)))


if __name__ == "__main__":
    main(small="--small" in sys.argv[1:])
