"""Timing of the channel-pair IR metrics (DESIGN.md "IR metrics: channel pairs", the measured table).  The cfg2-shaped tensor of
ir_metrics_timing.py: 32 capsules x 64 sources x 96 000 samples at 48 kHz (786 MB), a 6 x 5 x 3 m room with beta = 0.877 and the default
tail, generated on the device.  Timed: al_ir_pair_metrics at max_lag 48 (ISO's +-1 ms) over the 16 consecutive pairs and over all 496
pairs -- the pair list walked in calls whose workspace stays under 1 GiB, as acoustics.pair_metrics_device walks it --, with and
without the curves, beside al_ir_metrics on the same tensor (the rows table every pair call needs, formed once) and beside
DeviceIRTensor.host(), the download a numpy route starts from (wall clock, one transfer).  The count of float64 multiply-adds the
definition asks for, lines x L x (2 J + 1 + 2), over the chip's float64 vector peak (78.6 TFLOPS: 39.3e12 multiply-adds per second) is
the ceiling printed beside each; the kernel issues lines x L x 64 ceil((2 J + 1) / 64) + 2 of them (lanes own lags in blocks of 64).
HIP events around each case, every case warmed up once, then REPS rounds that go through the cases in turn; the median per case and
the spread (max - min) / median are printed.

    python profiles/tools/ir_pair_metrics_timing.py [--small]        (--small: 8 capsules x 8 sources, to try the script)
"""
import os
import sys
import time

import numpy as np

REPS = 5
ROOM, BETA, FS, IR_LEN, MAX_LAG = (6.0, 5.0, 3.0), 0.877, 48000.0, 96000, 48
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
    rows, n_lags = n_cap * n_src, 2 * MAX_LAG + 1
    P, X = mem.ptr(buf), mem.stream()
    wide_bytes = lib.call("al_ir_metrics_workspace_bytes", n_cap, n_src, IR_LEN)
    wide_ws = mem.empty(wide_bytes // 8 + 1, np.float64)
    wide = mem.empty(rows * 16, np.float64)
    lists = {"consecutive": acoustics.check_pairs(None, n_cap), "all": acoustics.check_pairs("all", n_cap)}
    one = lib.call("al_ir_pair_metrics_workspace_bytes", 1, n_src, IR_LEN, MAX_LAG)
    most = max(len(v) for v in lists.values())
    per_call = max(1, min(most, WORKSPACE_CAP // one))
    ws = mem.empty(per_call * one // 8, np.float64)
    out = mem.empty(most * n_src * len(acoustics.PAIR_COLUMNS), np.float64)
    xc = mem.empty(most * n_src * 2 * n_lags, np.float64)
    tables = {k: mem.upload(v.reshape(-1)) for k, v in lists.items()}

    def broadband():
        lib.call("al_ir_metrics", P, n_cap, n_src, stride_c, pitch, IR_LEN, FS, mem.ptr(wide_ws), wide_bytes, mem.ptr(wide), None, X)

    def pairs(which, curves):
        def run():
            n_pairs = len(lists[which])
            for p0 in range(0, n_pairs, per_call):
                count = min(per_call, n_pairs - p0)
                lib.call("al_ir_pair_metrics", P, n_cap, n_src, stride_c, pitch, IR_LEN, FS, mem.ptr(wide), mem.ptr(tables[which]) + 8 * p0, count,
                         MAX_LAG, mem.ptr(ws), per_call * one, mem.ptr(out) + 8 * p0 * n_src * len(acoustics.PAIR_COLUMNS),
                         mem.ptr(xc) + 8 * p0 * n_src * 2 * n_lags if curves else None, X)
        return run

    cases = [("al_ir_metrics (the rows table)", broadband, None)]
    for which in lists:
        for curves in (False, True):
            cases.append((f"al_ir_pair_metrics, {len(lists[which])} pairs ({which})" + (", with curves" if curves else ""), pairs(which, curves),
                          len(lists[which])))
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
    print(f"tensor {n_cap} x {n_src} x {IR_LEN}, pitch {pitch}: {4 * rows * pitch / 1e6:.1f} MB; max_lag {MAX_LAG}; workspace {per_call * one / 1e6:.1f} MB "
          f"({per_call} pairs per call); median of {REPS}")
    for label, _, n_pairs in cases:
        t = np.array(times[label])
        line = f"{label:58s} {np.median(t):9.3f} ms   spread {(t.max() - t.min()) / np.median(t) * 100:5.1f} %"
        if n_pairs is not None:
            fma = n_pairs * n_src * IR_LEN * (n_lags + 2)
            issued = n_pairs * n_src * IR_LEN * (64 * -(-n_lags // 64) + 2)
            ceiling = 1e3 * fma / FMA_PER_SECOND
            line += (f"   {fma:.3g} multiply-adds ({issued:.3g} issued): ceiling {ceiling:7.3f} ms, reached {100 * ceiling / np.median(t):5.1f} % "
                     f"({100e3 * issued / FMA_PER_SECOND / np.median(t):5.1f} % of the issued)")
        print(line, flush=True)
    tensor = shoebox.DeviceIRTensor(r, buf, (stride_c, pitch), (n_cap, n_src, IR_LEN))
    mem.synchronize()
    start = time.perf_counter()
    host = tensor.host()
    print(f"{'DeviceIRTensor.host() (wall clock, once)':58s} {1e3 * (time.perf_counter() - start):9.3f} ms   {host.nbytes / 1e6:.1f} MB")
    got = np.asarray(mem.download(out))[: len(lists["all"]) * n_src * len(acoustics.PAIR_COLUMNS)].reshape(-1, n_src, len(acoustics.PAIR_COLUMNS))
    col = {name: got[..., i] for i, name in enumerate(acoustics.PAIR_COLUMNS)}
    print(f"all pairs: bad {int(np.nansum(col['bad']))}; median IACC early {np.nanmedian(np.abs(col['peak_e'])):.3f}, late "
          f"{np.nanmedian(np.abs(col['peak_l'])):.3f} (the tail draws independent noise per row); median |lag_e| {np.nanmedian(np.abs(col['lag_e'])):.1f} samples")


if __name__ == "__main__":
    main(small="--small" in sys.argv[1:])
