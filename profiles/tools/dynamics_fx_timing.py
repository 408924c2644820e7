"""Timing of k_fx_dynamics (al_fx_compressor, al_fx_limiter, and the batched launch of 64 clips of each) at 48 kHz for 4 s / 10 s /
60 s clips.  Run it twice: plainly for the wall time per call (a host clock around a synchronise), and under
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/tools/dynamics_fx_timing.py` for the kernel times, then
`python profiles/tools/dynamics_fx_timing.py --summarise DIR` prints one line per case from the trace (the cases launch the one
kernel, so the trace is cut into the cases by dispatch order: REPS dispatches each).

Input: uniform noise in (-0.5, 0.5), so the envelope is over the threshold from the first samples on and every sample pays the
gain's log and exp: the expensive side of the pointwise work."""
import csv
import ctypes as ct
import glob
import os
import sys
import time

import numpy as np

FS = 48000
LENGTHS = (4 * FS, 10 * FS, 60 * FS)
BATCH = 64
WARM, TIMED = 2, 10
REPS = WARM + TIMED
COMP = (-30.0, 4.0, 5.0, 120.0)
LIM = (-25.0, 300.0)


def cases():
    for n in LENGTHS:
        yield f"compressor n={n}", "compressor", n, 1
        yield f"limiter n={n}", "limiter", n, 1
        yield f"compressor n={n} x{BATCH} clips", "compressor", n, BATCH
        yield f"limiter n={n} x{BATCH} clips", "limiter", n, BATCH
    # the walk alone: a threshold the envelope never reaches, so no sample pays the gain's log and exp
    yield f"compressor n={LENGTHS[1]} under T", "quiet", LENGTHS[1], 1


def run():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from audiblelight_amd import _hip, engine

    r = engine.Renderer()
    lib, mem = r.lib, r.mem
    rng = np.random.default_rng(1)
    for label, kind, n, count in cases():
        srcs = [mem.upload(rng.uniform(-0.5, 0.5, n).astype(np.float32)) for _ in range(count)]
        dsts = [mem.empty(n) for _ in range(count)]
        args = (float(FS),) + {"compressor": COMP, "limiter": LIM, "quiet": (20.0,) + COMP[1:]}[kind]
        if count == 1:
            entry = "al_fx_limiter" if kind == "limiter" else "al_fx_compressor"

            def launch():
                lib.call(entry, mem.ptr(srcs[0]), mem.ptr(dsts[0]), n, *args, mem.stream())
        else:
            fxb = _hip.FXB_COMPRESSOR if kind == "compressor" else _hip.FXB_LIMITER
            arr = (_hip.FXB_JOBS[fxb] * count)()
            names = [f for f, _ in _hip.FXB_JOBS[fxb]._fields_[3:]]
            for job, s, d in zip(arr, srcs, dsts):
                job.src, job.dst, job.n = mem.ptr(s), mem.ptr(d), n
                for name, value in zip(names, args):
                    setattr(job, name, value)
            table = np.zeros(count * lib.call("al_fx_batch_desc_bytes", fxb), dtype=np.uint8)
            lib.call("al_fx_batch_pack", fxb, ct.cast(arr, ct.c_void_p), count, table.ctypes.data)
            device_table = mem.upload(table)

            def launch():
                lib.call("al_fx_batch_launch", fxb, mem.ptr(device_table), count, mem.stream())
        for _ in range(WARM):
            launch()
        mem.synchronize()
        t0 = time.perf_counter()
        for _ in range(TIMED):
            launch()
        mem.synchronize()
        print(f"wall  {label:38s} {(time.perf_counter() - t0) / TIMED * 1e3:9.3f} ms/call", flush=True)
        del srcs, dsts


def summarise(directory):
    paths = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    assert len(paths) == 1, paths
    rows = [row for row in csv.DictReader(open(paths[0])) if "k_fx_dynamics" in row["Kernel_Name"]]
    rows.sort(key=lambda row: int(row["Start_Timestamp"]))
    labels = [label for label, *_ in cases()]
    assert len(rows) == REPS * len(labels), (len(rows), len(labels))
    for i, label in enumerate(labels):
        us = [(int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3 for row in rows[i * REPS + WARM: (i + 1) * REPS]]
        print(f"k_fx_dynamics  {label:38s} dispatches {TIMED:3d}  avg {np.mean(us):10.1f} us  min {min(us):10.1f}  max {max(us):10.1f}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2])
    else:
        run()
