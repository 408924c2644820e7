"""Timing of the octave-band split and of the band metrics behind it (DESIGN.md "IR metrics: octave bands", the measured table).  The
cfg2-shaped tensor of ir_metrics_timing.py: 32 capsules x 64 sources x 96 000 samples at 48 kHz (786 MB), a 6 x 5 x 3 m room with beta =
0.877 and the default tail, generated on the device.  Timed: al_ir_band_split alone (six octave bands into a tensor six times the
size) and al_ir_band_metrics (the split in passes over a workspace of at most 1 GiB, and the five metric kernels over each pass), each at
half = 64 and half = 512, beside al_ir_metrics on the same tensor.  The count of float64 multiply-adds, rows x L x B x (2 half + 1), over
the chip's float64 vector peak (78.6 TFLOPS: 39.3e12 multiply-adds per second) is the ceiling printed beside each.  HIP events around
each call, every case warmed up once, then REPS rounds that go through the cases in turn; the median per case and the spread
(max - min) / median are printed.

    python profiles/tools/ir_band_metrics_timing.py [--small]        (--small: 8 capsules x 8 sources, to try the script)
"""
import os
import sys

import numpy as np

REPS = 5
ROOM, BETA, FS, IR_LEN = (6.0, 5.0, 3.0), 0.877, 48000.0, 96000
FMA_PER_SECOND = 39.3e12
WORKSPACE_CAP = 1 << 30


def main(small=False):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from audiblelight_amd import acoustics, engine, shoebox

    n_cap, n_src = (8, 8) if small else (32, 64)
    r = engine.Renderer()
    lib, mem, torch = r.lib, r.mem, r.mem.torch
    rng = np.random.default_rng(0)
    room, betas = np.array(ROOM), np.full(6, BETA)
    capsules = np.array([3.1, 2.4, 1.5]) + 0.042 * shoebox.check_directions(rng.standard_normal((n_cap, 3)))
    sources = rng.uniform(0.15, 0.85, (n_src, 3)) * room
    buf, (stride_c, pitch), _ = shoebox.shoebox_irs_device(r, room, betas, sources, capsules, IR_LEN, FS, tail=shoebox.ShoeboxTail(seed=1))
    rows, B = n_cap * n_src, len(shoebox.OCTAVE_CENTRES)
    out_pitch = (IR_LEN + 3) // 4 * 4
    band_rows = mem.empty(rows * B * out_pitch)
    per_row = lib.call("al_ir_band_metrics_workspace_bytes", B, IR_LEN)
    ws_bytes = max(1, min(rows, WORKSPACE_CAP // per_row)) * per_row
    ws = mem.empty(ws_bytes // 8, np.float64)
    table = mem.empty(rows * B * 16, np.float64)
    wide_bytes = lib.call("al_ir_metrics_workspace_bytes", n_cap, n_src, IR_LEN)
    wide_ws = mem.empty(wide_bytes // 8 + 1, np.float64)
    wide = mem.empty(rows * 16, np.float64)
    P, X = mem.ptr(buf), mem.stream()
    filters = {half: mem.upload(shoebox.band_filters(shoebox.OCTAVE_CENTRES, FS, half).reshape(-1)) for half in (64, 512)}

    def split(half):
        return lambda: lib.call("al_ir_band_split", P, n_cap, n_src, stride_c, pitch, IR_LEN, mem.ptr(filters[half]), B, half,
                                mem.ptr(band_rows), out_pitch, X)

    def metrics(half):
        return lambda: lib.call("al_ir_band_metrics", P, n_cap, n_src, stride_c, pitch, IR_LEN, FS, mem.ptr(filters[half]), B, half,
                                mem.ptr(ws), ws_bytes, mem.ptr(table), None, X)

    cases = [(f"al_ir_band_split, half {half}", split(half), half) for half in (64, 512)]
    cases += [(f"al_ir_band_metrics, half {half}", metrics(half), half) for half in (64, 512)]
    cases.append(("al_ir_metrics (broadband), table only",
                  lambda: lib.call("al_ir_metrics", P, n_cap, n_src, stride_c, pitch, IR_LEN, FS, mem.ptr(wide_ws), wide_bytes, mem.ptr(wide),
                                   None, X), None))
    times = {label: [] for label, _, _ in cases}
    for rep in range(REPS + 1):
        for label, call, _ in cases:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            mem.synchronize()
            a.record(torch.cuda.current_stream(mem.device))
            call()
            b.record(torch.cuda.current_stream(mem.device))
            mem.synchronize()
            if rep > 0:      # the first round warms every case up
                times[label].append(a.elapsed_time(b))
    print(f"tensor {n_cap} x {n_src} x {IR_LEN}, pitch {pitch}: {4 * rows * pitch / 1e6:.1f} MB; {B} bands: band rows {4 * rows * B * out_pitch / 1e6:.1f} MB; "
          f"band metrics workspace {ws_bytes / 1e6:.1f} MB ({ws_bytes // per_row} rows per pass); median of {REPS}")
    for label, _, half in cases:
        t = np.array(times[label])
        line = f"{label:44s} {np.median(t):9.3f} ms   spread {(t.max() - t.min()) / np.median(t) * 100:5.1f} %"
        if half is not None:
            ceiling = 1e3 * rows * IR_LEN * B * (2 * half + 1) / FMA_PER_SECOND
            line += f"   {rows * IR_LEN * B * (2 * half + 1):.3g} multiply-adds: ceiling {ceiling:7.3f} ms, reached {100 * ceiling / np.median(t):5.1f} %"
        print(line, flush=True)
    got = np.asarray(mem.download(table)).reshape(rows, B, 16)
    t30 = got[:, :, acoustics.COLUMNS.index("t30")]
    print(f"the band rows (half 512): bad {int(got[:, :, 0].sum())}; median T30 per band " + " ".join(f"{v:.3f}" for v in np.nanmedian(t30, axis=0)) +
          f" s; Sabine {acoustics.sabine_rt60(room, betas):.3f} s")


if __name__ == "__main__":
    main(small="--small" in sys.argv[1:])
