"""Timing of al_ism_shoebox_sphere beside what a user had before it, on the same tensor (DESIGN.md "Shoebox IRs: rigid-sphere
receivers", the measured table).  The cfg2-shaped tensor: 32 capsules x 64 sources x 96 000 samples at 48 kHz (786 MB), a 6 x 5 x 3 m
room with beta = 0.877.  The 32 capsules sit on a rigid sphere of 4.2 cm (directions drawn from a seed; 28 Legendre orders, filters of
half = 64): with the tail's default mix and fade, and without a tail at max_order 10.  Beside them: 32 omnidirectional capsules at the
same points in free air (al_ism_shoebox_tail, al_ism_shoebox at max_order 10), and Renderer.upload_irs of a host tensor of that
shape.  HIP events around each call (a host clock around the upload, which ends in a synchronise), every case warmed up once, then
REPS rounds that go through the cases in turn; the median per case and the spread (max - min) / median are printed.

    python profiles/tools/shoebox_sphere_timing.py [--small]        (--small: 8 capsules x 8 sources, to try the script)
"""
import ctypes as ct
import os
import sys
import time

import numpy as np

REPS = 5
ROOM, BETA, FS, IR_LEN, ORDER, RADIUS = (6.0, 5.0, 3.0), 0.877, 48000.0, 96000, 10, 0.042


def main(small=False):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from audiblelight_amd import engine, shoebox

    n_cap, n_src = (8, 8) if small else (32, 64)
    r = engine.Renderer()
    lib, mem, torch = r.lib, r.mem, r.mem.torch
    rng = np.random.default_rng(0)
    room, betas = np.array(ROOM), np.full(6, BETA)
    centre = np.array([3.1, 2.4, 1.5])
    directions = shoebox.check_directions(rng.standard_normal((n_cap, 3)))
    capsules = centre + RADIUS * directions
    sources = rng.uniform(0.15, 0.85, (n_src, 3)) * room
    shoebox.check_arguments(room, betas, sources, capsules, IR_LEN, FS)
    shoebox.check_sphere(room, centre, RADIUS, sources)
    table, psi = shoebox.sphere_filters(RADIUS, FS), shoebox.sphere_diffuse_filter(RADIUS, FS)
    n_orders, half = table.shape[0], (table.shape[1] - 1) // 2
    pitch = shoebox.pitch_of(IR_LEN)
    total = n_cap * n_src * pitch
    mix, fade = shoebox.tail_samples(shoebox.ShoeboxTail(seed=1), room, FS)
    ln_env = shoebox.tail_envelope(room, betas, IR_LEN, FS, mix)
    n_knots = len(ln_env)
    up = lambda a: mem.upload(np.ascontiguousarray(a, dtype=np.float64).reshape(-1))      # noqa: E731
    src_dev, cap_dev, dir_dev, table_dev, psi_dev = up(sources), up(capsules), up(directions), up(table), up(psi)
    env_dev, env_src_dev = up(ln_env), up(np.tile(ln_env, (n_src, 1)))
    out = mem.empty(total)
    L, B = room.ctypes.data_as(ct.POINTER(ct.c_double)), betas.ctypes.data_as(ct.POINTER(ct.c_double))
    O_ = centre.ctypes.data_as(ct.POINTER(ct.c_double))
    P, C, D, O, X = mem.ptr(src_dev), mem.ptr(cap_dev), mem.ptr(dir_dev), mem.ptr(out), mem.stream()
    pairs = n_cap * n_src

    def workspace(mix_arg, fade_arg):
        per_pair = lib.call("al_ism_shoebox_sphere_workspace_bytes", n_orders, half, IR_LEN, mix_arg, fade_arg)
        n = max(1, min(pairs, shoebox.BAND_WORKSPACE_CAP // per_pair))
        return mem.empty(n * per_pair // 8, dtype=np.float64), n * per_pair, n

    ws_tail, ws_tail_bytes, per_pass_tail = workspace(mix, fade)
    ws_plain, ws_plain_bytes, per_pass_plain = workspace(-1, 0)
    print(f"sphere of {RADIUS} m: {n_orders} orders, half {half}; workspace {ws_tail_bytes / 1e6:.1f} MB with the tail ({per_pass_tail} pairs per "
          f"pass), {ws_plain_bytes / 1e6:.1f} MB without ({per_pass_plain} pairs per pass)", flush=True)

    def sphere(tail):
        order, t, ws, ws_bytes = (-1, (mix, fade, 1, 0, 0, mem.ptr(env_src_dev), n_knots), ws_tail, ws_tail_bytes) if tail else (
            ORDER, (-1, 0, 0, 0, 0, None, 0), ws_plain, ws_plain_bytes)
        return lambda: lib.call("al_ism_shoebox_sphere", P, n_src, None, O_, D, n_cap, L, B, 0.0, mem.ptr(table_dev), n_orders, half,
                                mem.ptr(psi_dev), 343.0, FS, order, IR_LEN, pitch, *t, mem.ptr(ws), ws_bytes, O, X)

    def omni(tail):
        if tail:
            return lambda: lib.call("al_ism_shoebox_tail", P, n_src, C, n_cap, L, B, 343.0, FS, -1, IR_LEN, pitch, mix, fade, 1, 0, 0,
                                    mem.ptr(env_dev), n_knots, O, X)
        return lambda: lib.call("al_ism_shoebox", P, n_src, C, n_cap, L, B, 343.0, FS, ORDER, IR_LEN, pitch, O, X)

    host = rng.standard_normal((n_cap, n_src, IR_LEN)).astype(np.float32)
    cases = [(f"{n_cap} capsules on the sphere  tail, mix {mix} fade {fade}", sphere(True)),
             (f"{n_cap} omni capsules, free air  al_ism_shoebox_tail, mix {mix} fade {fade}", omni(True)),
             (f"{n_cap} capsules on the sphere  no tail, max_order {ORDER}", sphere(False)),
             (f"{n_cap} omni capsules, free air  al_ism_shoebox, max_order {ORDER}", omni(False))]
    times = {label: [] for label, _ in cases}
    uploads = []
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
        mem.synchronize()
        t0 = time.perf_counter()
        r.upload_irs(host)
        mem.synchronize()
        if rep > 0:
            uploads.append(1e3 * (time.perf_counter() - t0))
    print(f"tensor {n_cap} x {n_src} x {IR_LEN}, pitch {pitch}: {4 * total / 1e6:.1f} MB; median of {REPS}")
    for label, _ in cases:
        t = np.array(times[label])
        print(f"{label:78s} {np.median(t):9.3f} ms   spread {(t.max() - t.min()) / np.median(t) * 100:5.1f} %", flush=True)
    t = np.array(uploads)
    print(f"{'Renderer.upload_irs of a host tensor of that shape (host clock)':78s} {np.median(t):9.3f} ms   spread "
          f"{(t.max() - t.min()) / np.median(t) * 100:5.1f} %", flush=True)


if __name__ == "__main__":
    main(small="--small" in sys.argv[1:])
