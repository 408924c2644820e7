"""What a shoebox room sounds like, measured on the device: the reverberation times Sabine and Eyring predict for the room beside the
T30, EDT, direct-to-reverberant ratio and C50 that the generated impulse responses actually have (acoustics.ir_metrics: Schroeder's
backward integral over the tensors where they lie; nothing but the table of results is downloaded).  Once for a room asked for by
``rt60=0.5`` with the default diffuse tail, once for a room of named materials in octave bands.
The second room -- five hard walls and a carpet -- measures several times what Sabine and Eyring say: the image field keeps the
paths that run between the hard walls and never meet the carpet, which a diffuse-field formula averages away.

    python examples/shoebox_metrics.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from audiblelight_amd import acoustics, core, shoebox  # noqa: E402

ROOM = (6.0, 5.0, 3.0)
FS = 16000
CAPSULES = [[2.0, 2.4, 1.5], [2.1, 2.4, 1.5], [4.4, 1.2, 1.1]]
EMITTERS = [[4.6, 3.9, 1.7], [1.1, 1.0, 1.2]]
# absorption coefficients at 125 Hz ... 4 kHz (textbook values, rounded)
MATERIALS = {"carpet": ([125, 250, 500, 1000, 2000, 4000], [0.08, 0.24, 0.57, 0.69, 0.71, 0.73]),
             "plaster": ([125, 250, 500, 1000, 2000, 4000], [0.14, 0.10, 0.06, 0.05, 0.04, 0.03]),
             "glass": ([125, 250, 500, 1000, 2000, 4000], [0.35, 0.25, 0.18, 0.12, 0.07, 0.04])}


def report(title, state, predicted):
    state.add_microphone("mic", CAPSULES)
    state.add_emitters(EMITTERS)
    state.simulate()
    m = state.metrics()["mic"]                      # {alias: IRMetrics}; every column is (capsules, emitters)
    print(title)
    for name, value in predicted:
        print(f"  {name:28s} {value:6.3f} s")
    print("  capsule   T30 [s]   EDT [s]   DRR [dB]   C50 [dB]   decay in the row [dB]     (mean over the emitters)")
    for c in range(len(CAPSULES)):
        print(f"  {c:7d} {np.nanmean(m.t30[c]):9.3f} {np.nanmean(m.edt[c]):9.3f} {np.mean(m.drr_db[c]):10.2f} {np.mean(m.c50_db[c]):10.2f} "
              f"{np.mean(m.dyn_db[c]):12.1f}")
    assert not m.bad.any()
    return m


def main():
    st = core.ShoeboxIRState(ROOM, rt60=0.5, ir_len=FS, sample_rate=FS, tail=shoebox.ShoeboxTail(seed=7))
    report("a room asked for by rt60 = 0.5 s (Sabine), default tail", st,
           [("Sabine", acoustics.sabine_rt60(ROOM, st.betas)), ("Eyring", acoustics.eyring_rt60(ROOM, st.betas))])
    table = {k: (np.array(f, dtype=np.float64), np.array(a)) for k, (f, a) in MATERIALS.items()}
    walls = ["plaster", "glass", "plaster", "plaster", "carpet", "plaster"]
    st = core.ShoeboxIRState(ROOM, materials=walls, material_table=table, ir_len=FS, sample_rate=FS, tail=shoebox.ShoeboxTail(seed=7))
    bands = st.bands.centres
    sab = [acoustics.sabine_rt60(ROOM, st.betas[:, b]) for b in range(len(bands))]
    eyr = [acoustics.eyring_rt60(ROOM, st.betas[:, b]) for b in range(len(bands))]
    report("a room of materials (x: plaster, glass; y: plaster; floor: carpet; ceiling: plaster)", st,
           [(f"Sabine, {min(bands):.0f} .. {max(bands):.0f} Hz: min", min(sab)), ("Sabine: max", max(sab)), ("Eyring: min", min(eyr)),
            ("Eyring: max", max(eyr))])


if __name__ == "__main__":
    main()
