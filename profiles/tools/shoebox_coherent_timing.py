"""Timing of al_ism_shoebox_coherent beside the independent tail and a fill of the same tensor (DESIGN.md "Shoebox IRs: the coherent
tail", the measured table).  The cfg2-shaped tensor: 32 rows x 64 sources x 96 000 samples at 48 kHz (786 MB), a 6 x 5 x 3 m room with
beta = 0.877, the tail's default mix and fade, 64 plane waves of 8 taps.  The 32 rows are once 32 omni capsules of one array (one
group, one call) and once eight FOA points (eight groups, eight calls into the one tensor).  HIP events around each case, every case
warmed up once, then REPS rounds that go through the cases in turn; the median per case and the spread (max - min) / median are
printed, and for the coherent cases the float64 multiply-add rate of the samples past the split.  "below the split only" is the
same call on rows that end at the split: the image kernels with the direct evaluator in their epilogue, no k_ism_ctail.

    python profiles/tools/shoebox_coherent_timing.py [--small]        (--small: 8 rows x 8 sources x 96 000, to try the script)
"""
import ctypes as ct
import os
import sys

import numpy as np

REPS = 5
ROOM, BETA, FS, IR_LEN = (6.0, 5.0, 3.0), 0.877, 48000.0, 96000
N_WAVES, HALF_TAPS = 64, 4
TAG_GAUSSIAN = 3
PEAK_F64 = 78.6e12     # the chip's float64 vector peak, flop/s


def main(small=False):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from audiblelight_amd import engine, shoebox

    n_rows, n_src = (8, 8) if small else (32, 64)
    r = engine.Renderer()
    lib, mem, torch = r.lib, r.mem, r.mem.torch
    rng = np.random.default_rng(0)
    room, betas = np.array(ROOM), np.full(6, BETA)
    sources = rng.uniform(0.15, 0.85, (n_src, 3)) * room
    array = np.array([3.1, 2.4, 1.5]) + rng.uniform(-0.1, 0.1, (n_rows, 3))      # an array 20 cm across
    points = rng.uniform(0.3, 0.7, (n_rows // 4, 3)) * room                        # FOA listeners about the room
    shoebox.check_arguments(room, betas, sources, np.concatenate([array, points]), IR_LEN, FS)
    pitch = shoebox.pitch_of(IR_LEN)
    total = n_rows * n_src * pitch
    mix, fade = shoebox.tail_samples(shoebox.ShoeboxTail(seed=1), room, FS)
    n_knots = shoebox.n_knots_of(IR_LEN)
    ln_env = shoebox.tail_envelope(room, betas, IR_LEN, FS, mix)
    foa = shoebox.foa_patterns()
    env_foa = np.stack([shoebox.tail_envelope(room, betas, IR_LEN, FS, mix, pattern=p) for p in foa])      # (4, n_knots)
    up = lambda a: mem.upload(np.ascontiguousarray(a).reshape(-1))      # noqa: E731
    src_dev, arr_dev, env_dev = up(sources), up(array), up(ln_env)
    env_rows_dev = up(np.broadcast_to(ln_env, (n_rows, n_src, n_knots)))
    env_foa_dev = up(np.broadcast_to(env_foa[:, None, :], (4, n_src, n_knots)))
    taps, delays = shoebox.coherent_tail_tables(array, None, None, FS, 343.0, N_WAVES, HALF_TAPS)
    taps_dev, delays_dev = up(taps), up(delays)
    foa_taps, foa_delays = shoebox.coherent_tail_tables(np.zeros((4, 3)), foa, None, FS, 343.0, N_WAVES, HALF_TAPS)
    foa_taps_dev, foa_delays_dev, foa_dev = up(foa_taps), up(foa_delays), up(foa)
    point_dev = [up(p) for p in points]
    out = mem.empty(total)
    L, B = room.ctypes.data_as(ct.POINTER(ct.c_double)), betas.ctypes.data_as(ct.POINTER(ct.c_double))
    J = 2 * HALF_TAPS

    split = (mix + fade + 255) // 256 * 256
    short_knots = shoebox.n_knots_of(split)      # rows that end at the split read the first knots of the same tables
    env_rows_short = up(np.broadcast_to(ln_env[:short_knots], (n_rows, n_src, short_knots)))
    env_foa_short = up(np.broadcast_to(env_foa[:, None, :short_knots], (4, n_src, short_knots)))

    def array_call(length=IR_LEN, row_pitch=pitch, env=env_rows_dev, knots=n_knots):
        lib.call("al_ism_shoebox_coherent", mem.ptr(src_dev), n_src, None, mem.ptr(arr_dev), n_rows, None, 1, L, B, 0.0, 343.0, FS, -1, length,
                 row_pitch, mix, fade, 1, 0, 0, mem.ptr(env), knots, mem.ptr(taps_dev), mem.ptr(delays_dev), N_WAVES, J, 0,
                 mem.ptr(out), mem.stream())

    def foa_call(length=IR_LEN, row_pitch=pitch, env=env_foa_dev, knots=n_knots):
        for i, p in enumerate(point_dev):
            lib.call("al_ism_shoebox_coherent", mem.ptr(src_dev), n_src, None, mem.ptr(p), 1, mem.ptr(foa_dev), 4, L, B, 0.0, 343.0, FS, -1,
                     length, row_pitch, mix, fade, 1, 0, 4 * i, mem.ptr(env), knots, mem.ptr(foa_taps_dev), mem.ptr(foa_delays_dev),
                     N_WAVES, J, 4 * i, mem.ptr(out) + 4 * (4 * i * n_src * row_pitch), mem.stream())

    def tail_call():
        lib.call("al_ism_shoebox_tail", mem.ptr(src_dev), n_src, mem.ptr(arr_dev), n_rows, L, B, 343.0, FS, -1, IR_LEN, pitch, mix, fade,
                 1, 0, 0, mem.ptr(env_dev), n_knots, mem.ptr(out), mem.stream())

    def fill_call():
        lib.call("al_normal_fill", mem.ptr(out), total, ct.c_uint64(1), TAG_GAUSSIAN, ct.c_float(1.0), mem.stream())

    cases = [(f"coherent, {n_rows} omnis as one group", array_call), (f"coherent, {n_rows // 4} FOA points as {n_rows // 4} groups", foa_call),
             (f"  below the split only ({split} samples), omnis", lambda: array_call(split, split, env_rows_short, short_knots)),
             (f"  below the split only ({split} samples), FOA", lambda: foa_call(split, split, env_foa_short, short_knots)),
             (f"al_ism_shoebox_tail, mix {mix} fade {fade}", tail_call), ("al_normal_fill, same bytes", fill_call)]
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
    flop = 2.0 * n_rows * n_src * (IR_LEN - split) * N_WAVES * J
    print(f"tensor {n_rows} x {n_src} x {IR_LEN}, pitch {pitch}: {4 * total / 1e6:.1f} MB; {N_WAVES} plane waves x {J} taps; median of {REPS}")
    for label, _ in cases:
        t = np.array(times[label])
        med = float(np.median(t))
        rate = f"   {flop / med / 1e9:7.2f} TFLOP/s float64 ({flop / med / 1e-3 / PEAK_F64 * 100:4.1f} % of peak)" if label.startswith("coherent") else ""
        print(f"{label:44s} {med:9.3f} ms   spread {(t.max() - t.min()) / med * 100:5.1f} %   {4 * total / med / 1e9:7.3f} TB/s{rate}", flush=True)


if __name__ == "__main__":
    main(small="--small" in sys.argv[1:])
