"""Timing of al_ism_shoebox_bands_tail beside the broadband tail, an upload and the band entry without a tail (DESIGN.md "Shoebox IRs:
frequency-dependent walls", the measured table).  The cfg2-shaped tensor: 32 capsules x 64 sources x 96 000 samples at 48 kHz
(786 MB), a 6 x 5 x 3 m room, six octave bands with half = 512 and absorption 0.10 .. 0.40 rising with frequency on every wall, the
tail's default mix and fade; the broadband cases with beta = 0.877.  HIP events around each call, every case warmed up once, then
REPS rounds that go through the cases in turn; the median per case and the spread (max - min) / median are printed.  The band
workspace is what shoebox_irs_device would allocate (1 GiB cap).  "image part only" is the same call on rows that end at the split
(ir_len = 2560): what is left of the full call's time is k_ism_band_tail's.

    python profiles/tools/shoebox_bands_timing.py [--small]        (--small: 4 x 8 x 96 000, to try the script)
"""
import ctypes as ct
import os
import sys

import numpy as np

REPS = 5
ROOM, BETA, FS, IR_LEN, HALF = (6.0, 5.0, 3.0), 0.877, 48000.0, 96000, 512
ALPHAS = (0.10, 0.14, 0.18, 0.23, 0.30, 0.40)


def main(small=False):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from audiblelight_amd import engine, shoebox

    n_cap, n_src = (4, 8) if small else (32, 64)
    r = engine.Renderer()
    lib, mem, torch = r.lib, r.mem, r.mem.torch
    rng = np.random.default_rng(0)
    room, betas = np.array(ROOM), np.full(6, BETA)
    band_betas = np.ascontiguousarray(np.repeat(shoebox.betas_from_absorption(ALPHAS)[None, :], 6, axis=0))
    n_bands = band_betas.shape[1]
    sources = rng.uniform(0.15, 0.85, (n_src, 3)) * room
    capsules = rng.uniform(0.15, 0.85, (n_cap, 3)) * room
    bands = shoebox.ShoeboxBands(shoebox.OCTAVE_CENTRES, HALF)
    tail = shoebox.ShoeboxTail(seed=1)
    shoebox.check_arguments(room, band_betas, sources, capsules, IR_LEN, FS, tail=tail, bands=bands)
    pitch = shoebox.pitch_of(IR_LEN)
    total = n_cap * n_src * pitch
    mix, fade = shoebox.tail_samples(tail, room, FS)
    split = (mix + fade + 255) // 256 * 256
    ln_env = shoebox.tail_envelope(room, betas, IR_LEN, FS, mix)
    band_env = np.stack([shoebox.tail_envelope(room, band_betas[:, b], IR_LEN, FS, mix) for b in range(n_bands)])
    cut_env = np.ascontiguousarray(band_env[:, : shoebox.n_knots_of(split)])
    src_dev, cap_dev, env_dev = mem.upload(sources.reshape(-1)), mem.upload(capsules.reshape(-1)), mem.upload(ln_env)
    band_env_dev, cut_env_dev = mem.upload(band_env.reshape(-1)), mem.upload(cut_env.reshape(-1))
    phi_dev = mem.upload(shoebox.band_filters(bands.centres, FS, HALF).reshape(-1))
    out = mem.empty(total)
    host = np.ones((n_cap, n_src, IR_LEN), dtype=np.float32)
    L, B = room.ctypes.data_as(ct.POINTER(ct.c_double)), betas.ctypes.data_as(ct.POINTER(ct.c_double))
    BB = band_betas.ctypes.data_as(ct.POINTER(ct.c_double))
    pairs = n_cap * n_src

    def workspace(mix_arg, fade_arg, ir_len):
        per_pair = lib.call("al_ism_shoebox_bands_workspace_bytes", n_bands, HALF, ir_len, mix_arg, fade_arg)
        n = max(1, min(pairs, shoebox.BAND_WORKSPACE_CAP // per_pair))
        return mem.empty(n * per_pair // 8, dtype=np.float64), n * per_pair, n

    ws_tail, ws_tail_bytes, tail_pairs = workspace(mix, fade, IR_LEN)
    ws_plain, ws_plain_bytes, plain_pairs = workspace(-1, 0, IR_LEN)

    def bands_tail_call():
        lib.call("al_ism_shoebox_bands_tail", mem.ptr(src_dev), n_src, mem.ptr(cap_dev), n_cap, L, BB, n_bands, mem.ptr(phi_dev), HALF, 343.0,
                 FS, -1, IR_LEN, pitch, mix, fade, 1, 0, 0, mem.ptr(band_env_dev), band_env.shape[1], mem.ptr(ws_tail), ws_tail_bytes,
                 mem.ptr(out), mem.stream())

    def bands_image_part_call():
        lib.call("al_ism_shoebox_bands_tail", mem.ptr(src_dev), n_src, mem.ptr(cap_dev), n_cap, L, BB, n_bands, mem.ptr(phi_dev), HALF, 343.0,
                 FS, -1, split, split, mix, fade, 1, 0, 0, mem.ptr(cut_env_dev), cut_env.shape[1], mem.ptr(ws_tail), ws_tail_bytes,
                 mem.ptr(out), mem.stream())

    def bands_order10_call():
        lib.call("al_ism_shoebox_bands", mem.ptr(src_dev), n_src, mem.ptr(cap_dev), n_cap, L, BB, n_bands, mem.ptr(phi_dev), HALF, 343.0, FS,
                 10, IR_LEN, pitch, mem.ptr(ws_plain), ws_plain_bytes, mem.ptr(out), mem.stream())

    def tail_call():
        lib.call("al_ism_shoebox_tail", mem.ptr(src_dev), n_src, mem.ptr(cap_dev), n_cap, L, B, 343.0, FS, -1, IR_LEN, pitch, mix, fade,
                 1, 0, 0, mem.ptr(env_dev), len(ln_env), mem.ptr(out), mem.stream())

    def upload_call():
        r.upload_irs(host)

    cases = [(f"al_ism_shoebox_bands_tail, 6 bands, half {HALF}", bands_tail_call),
             (f"  the same, image part only (ir_len {split})", bands_image_part_call),
             ("al_ism_shoebox_tail (broadband)", tail_call), ("Renderer.upload_irs", upload_call),
             ("al_ism_shoebox_bands, max_order 10, no tail", bands_order10_call)]
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
    print(f"tensor {n_cap} x {n_src} x {IR_LEN}, pitch {pitch}: {4 * total / 1e6:.1f} MB; mix {mix} fade {fade} split {split}; median of {REPS}")
    print(f"band workspace: with a tail {ws_tail_bytes / 2**20:.1f} MiB ({tail_pairs} pairs per pass), without {ws_plain_bytes / 2**20:.1f} MiB "
          f"({plain_pairs} pairs per pass)")
    for label, _ in cases:
        t = np.array(times[label])
        med = float(np.median(t))
        print(f"{label:52s} {med:10.3f} ms   spread {(t.max() - t.min()) / med * 100:5.1f} %", flush=True)


if __name__ == "__main__":
    main(small="--small" in sys.argv[1:])
