"""Timing of al_ir_metrics beside one plain read pass over the same bytes and beside the download it replaces (DESIGN.md "IR
metrics", the measured table).  The cfg2-shaped tensor: 32 capsules x 64 sources x 96 000 samples at 48 kHz (786 MB), a 6 x 5 x 3 m
room with beta = 0.877 and the default tail, generated on the device.  Timed: al_ir_metrics without and with the knots of the curve,
al_row_stats over the same rows (one read pass: sum |x|, max |x|, the non-finite count and sum x^2 in float32), and
DeviceIRTensor.host(), the download a numpy Schroeder integral would start from.  HIP events around each call (a host clock around
the download, which ends in a synchronise), every case warmed up once, then REPS rounds that go through the cases in turn; the median
per case and the spread (max - min) / median are printed.

    python profiles/tools/ir_metrics_timing.py [--small]        (--small: 8 capsules x 8 sources, to try the script)
"""
import os
import sys
import time

import numpy as np

REPS = 5
ROOM, BETA, FS, IR_LEN = (6.0, 5.0, 3.0), 0.877, 48000.0, 96000


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
    tensor = shoebox.DeviceIRTensor(r, buf, (stride_c, pitch), (n_cap, n_src, IR_LEN))
    assert pitch == IR_LEN and stride_c == n_src * pitch          # al_row_stats reads (rows, cols) without a pitch
    rows = n_cap * n_src
    nbytes = lib.call("al_ir_metrics_workspace_bytes", n_cap, n_src, IR_LEN)
    ws = mem.empty(nbytes // 8 + 1, np.float64)
    out = mem.empty(rows * 16, np.float64)
    knots = mem.empty(rows * acoustics.n_knots_of(IR_LEN), np.float64)
    partials = mem.empty(lib.call("al_row_stats_partials", rows, IR_LEN))
    stats = mem.empty(rows * 4, np.float64)
    P, X = mem.ptr(buf), mem.stream()

    def metrics(with_knots):
        return lambda: lib.call("al_ir_metrics", P, n_cap, n_src, stride_c, pitch, IR_LEN, FS, mem.ptr(ws), nbytes, mem.ptr(out),
                                mem.ptr(knots) if with_knots else None, X)

    cases = [("al_ir_metrics, table only", metrics(False)), ("al_ir_metrics, table and knots", metrics(True)),
             ("al_row_stats over the same rows (one read pass)", lambda: lib.call("al_row_stats", P, rows, IR_LEN, mem.ptr(partials),
                                                                                  mem.ptr(stats), X))]
    times = {label: [] for label, _ in cases}
    downloads = []
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
        tensor._host = None
        mem.synchronize()
        t0 = time.perf_counter()
        tensor.host()
        if rep > 0:
            downloads.append(1e3 * (time.perf_counter() - t0))
    table = np.asarray(mem.download(out)).reshape(rows, 16)
    print(f"tensor {n_cap} x {n_src} x {IR_LEN}, pitch {pitch}: {4 * rows * pitch / 1e6:.1f} MB; workspace {nbytes / 1e6:.1f} MB; median of {REPS}")
    for label, _ in cases:
        t = np.array(times[label])
        gbs = 4e-6 * rows * IR_LEN / np.median(t)
        print(f"{label:60s} {np.median(t):9.3f} ms   spread {(t.max() - t.min()) / np.median(t) * 100:5.1f} %   {gbs:7.0f} GB/s per tensor pass", flush=True)
    t = np.array(downloads)
    print(f"{'DeviceIRTensor.host(): the download (host clock)':60s} {np.median(t):9.3f} ms   spread {(t.max() - t.min()) / np.median(t) * 100:5.1f} %",
          flush=True)
    col = {name: table[:, i] for i, name in enumerate(acoustics.COLUMNS)}
    print(f"the rows: bad {int(col['bad'].sum())}; median T30 {np.nanmedian(col['t30']):.3f} s, EDT {np.nanmedian(col['edt']):.3f} s, "
          f"DRR {np.nanmedian(col['drr_db']):.2f} dB, C50 {np.nanmedian(col['c50_db']):.2f} dB; Sabine {acoustics.sabine_rt60(room, betas):.3f} s, "
          f"Eyring {acoustics.eyring_rt60(room, betas):.3f} s")


if __name__ == "__main__":
    main(small="--small" in sys.argv[1:])
