"""Timing of al_ism_shoebox_tail beside a fill, an upload and the plain generator of the same tensor (DESIGN.md "Shoebox IRs: the
diffuse tail", the measured table).  The cfg2-shaped tensor: 32 capsules x 64 sources x 96 000 samples at 48 kHz (786 MB), a 6 x 5 x
3 m room with beta = 0.877, the tail's default mix and fade.  HIP events around each call, every case warmed up once, then REPS
rounds that go through the cases in turn; the median per case and the spread (max - min) / median are printed.

    python profiles/tools/shoebox_tail_timing.py [--small]        (--small: 4 x 8 x 96 000, to try the script)
"""
import ctypes as ct
import os
import sys

import numpy as np

REPS = 5
ROOM, BETA, FS, IR_LEN = (6.0, 5.0, 3.0), 0.877, 48000.0, 96000
TAG_GAUSSIAN = 3


def main(small=False):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from audiblelight_amd import engine, shoebox

    n_cap, n_src = (4, 8) if small else (32, 64)
    r = engine.Renderer()
    lib, mem, torch = r.lib, r.mem, r.mem.torch
    rng = np.random.default_rng(0)
    room, betas = np.array(ROOM), np.full(6, BETA)
    sources = rng.uniform(0.15, 0.85, (n_src, 3)) * room
    capsules = rng.uniform(0.15, 0.85, (n_cap, 3)) * room
    shoebox.check_arguments(room, betas, sources, capsules, IR_LEN, FS)
    pitch = shoebox.pitch_of(IR_LEN)
    total = n_cap * n_src * pitch
    tail = shoebox.ShoeboxTail(seed=1)
    mix, fade = shoebox.tail_samples(tail, room, FS)
    ln_env = shoebox.tail_envelope(room, betas, IR_LEN, FS, mix)
    src_dev, cap_dev, env_dev = mem.upload(sources.reshape(-1)), mem.upload(capsules.reshape(-1)), mem.upload(ln_env)
    out = mem.empty(total)
    host = np.ones((n_cap, n_src, IR_LEN), dtype=np.float32)
    L, B = room.ctypes.data_as(ct.POINTER(ct.c_double)), betas.ctypes.data_as(ct.POINTER(ct.c_double))

    def tail_call():
        lib.call("al_ism_shoebox_tail", mem.ptr(src_dev), n_src, mem.ptr(cap_dev), n_cap, L, B, 343.0, FS, -1, IR_LEN, pitch, mix, fade,
                 1, 0, 0, mem.ptr(env_dev), len(ln_env), mem.ptr(out), mem.stream())

    def fill_call():
        lib.call("al_normal_fill", mem.ptr(out), total, ct.c_uint64(1), TAG_GAUSSIAN, ct.c_float(1.0), mem.stream())

    def order10_call():
        lib.call("al_ism_shoebox", mem.ptr(src_dev), n_src, mem.ptr(cap_dev), n_cap, L, B, 343.0, FS, 10, IR_LEN, pitch, mem.ptr(out),
                 mem.stream())

    def upload_call():
        r.upload_irs(host)

    cases = [(f"al_ism_shoebox_tail, mix {mix} fade {fade}", tail_call), ("al_normal_fill, same bytes", fill_call),
             ("al_ism_shoebox, max_order 10", order10_call), ("Renderer.upload_irs", upload_call)]
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
    print(f"tensor {n_cap} x {n_src} x {IR_LEN}, pitch {pitch}: {4 * total / 1e6:.1f} MB; median of {REPS}")
    for label, _ in cases:
        t = np.array(times[label])
        med = float(np.median(t))
        print(f"{label:44s} {med:9.3f} ms   spread {(t.max() - t.min()) / med * 100:5.1f} %   {4 * total / med / 1e9:7.3f} TB/s", flush=True)


if __name__ == "__main__":
    main(small="--small" in sys.argv[1:])
