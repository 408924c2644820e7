"""Timing of al_ism_shoebox_dir / al_ism_shoebox_dir_tail beside the omnidirectional entries on the same tensor (DESIGN.md "Shoebox
IRs: directional receivers", the measured table).  The cfg2-shaped tensor: 32 rows x 64 sources x 96 000 samples at 48 kHz (786 MB),
a 6 x 5 x 3 m room with beta = 0.877.  The 32 rows are made three ways: 32 omnidirectional capsules (the entries as they were), 8 FOA
listeners (P = 8, K = 4: a quarter of the image searches) and 32 cardioids (P = 32, K = 1: the price of the gain alone); each with
the tail's default mix and fade, and without a tail at max_order 10.  HIP events around each call, every case warmed up once, then
REPS rounds that go through the cases in turn; the median per case and the spread (max - min) / median are printed.

    python profiles/tools/shoebox_directional_timing.py [--small]        (--small: 8 rows x 8 sources, to try the script)
"""
import ctypes as ct
import os
import sys

import numpy as np

REPS = 5
ROOM, BETA, FS, IR_LEN, ORDER = (6.0, 5.0, 3.0), 0.877, 48000.0, 96000, 10


def main(small=False):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from audiblelight_amd import engine, shoebox

    n_rows, n_src = (8, 8) if small else (32, 64)
    r = engine.Renderer()
    lib, mem, torch = r.lib, r.mem, r.mem.torch
    rng = np.random.default_rng(0)
    room, betas = np.array(ROOM), np.full(6, BETA)
    sources = rng.uniform(0.15, 0.85, (n_src, 3)) * room
    capsules = rng.uniform(0.15, 0.85, (n_rows, 3)) * room
    foa = np.tile(shoebox.foa_patterns(), (n_rows // 4, 1, 1))
    cardioids = np.stack([shoebox.cardioid(v)[None] for v in rng.standard_normal((n_rows, 3))])
    shoebox.check_arguments(room, betas, sources, capsules, IR_LEN, FS, patterns=cardioids)
    pitch = shoebox.pitch_of(IR_LEN)
    total = n_rows * n_src * pitch
    mix, fade = shoebox.tail_samples(shoebox.ShoeboxTail(seed=1), room, FS)
    omni_env = shoebox.tail_envelope(room, betas, IR_LEN, FS, mix)
    n_knots = len(omni_env)
    foa_env = np.stack([shoebox.tail_envelope(room, betas, IR_LEN, FS, mix, pattern=p) for p in foa.reshape(-1, 4)])
    card_env = np.stack([shoebox.tail_envelope(room, betas, IR_LEN, FS, mix, pattern=p) for p in cardioids.reshape(-1, 4)])
    up = lambda a: mem.upload(np.ascontiguousarray(a, dtype=np.float64).reshape(-1))      # noqa: E731
    src_dev, cap_dev = up(sources), up(capsules)
    dev = dict(omni_env=up(omni_env), foa=up(foa), foa_env=up(foa_env), card=up(cardioids), card_env=up(card_env))
    out = mem.empty(total)
    L, B = room.ctypes.data_as(ct.POINTER(ct.c_double)), betas.ctypes.data_as(ct.POINTER(ct.c_double))

    def omni(tail):
        if tail:
            return lambda: lib.call("al_ism_shoebox_tail", mem.ptr(src_dev), n_src, mem.ptr(cap_dev), n_rows, L, B, 343.0, FS, -1, IR_LEN,
                                    pitch, mix, fade, 1, 0, 0, mem.ptr(dev["omni_env"]), n_knots, mem.ptr(out), mem.stream())
        return lambda: lib.call("al_ism_shoebox", mem.ptr(src_dev), n_src, mem.ptr(cap_dev), n_rows, L, B, 343.0, FS, ORDER, IR_LEN, pitch,
                                mem.ptr(out), mem.stream())

    def directional(tail, pat, env, n_pos, k):
        if tail:
            return lambda: lib.call("al_ism_shoebox_dir_tail", mem.ptr(src_dev), n_src, mem.ptr(cap_dev), n_pos, mem.ptr(dev[pat]), k, L, B,
                                    343.0, FS, -1, IR_LEN, pitch, mix, fade, 1, 0, 0, mem.ptr(dev[env]), n_knots, mem.ptr(out), mem.stream())
        return lambda: lib.call("al_ism_shoebox_dir", mem.ptr(src_dev), n_src, mem.ptr(cap_dev), n_pos, mem.ptr(dev[pat]), k, L, B, 343.0,
                                FS, ORDER, IR_LEN, pitch, mem.ptr(out), mem.stream())

    cases = []
    for tail, what in ((True, f"tail, mix {mix} fade {fade}"), (False, f"no tail, max_order {ORDER}")):
        cases += [(f"{n_rows} omni capsules          {what}", omni(tail)),
                  (f"{n_rows // 4} FOA listeners (K = 4)    {what}", directional(tail, "foa", "foa_env", n_rows // 4, 4)),
                  (f"{n_rows} cardioids (K = 1)       {what}", directional(tail, "card", "card_env", n_rows, 1))]
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
        print(f"{label:62s} {medians[-1]:9.3f} ms   spread {(t.max() - t.min()) / medians[-1] * 100:5.1f} %", flush=True)
    for base, what in ((0, "tail"), (3, f"max_order {ORDER}")):
        print(f"{what}: FOA / omni = {medians[base + 1] / medians[base]:.3f}, cardioids / omni = {medians[base + 2] / medians[base]:.3f}")


if __name__ == "__main__":
    main(small="--small" in sys.argv[1:])
