"""A room of named materials measured per octave band, on the device: the T30 and EDT every band of the generated impulse responses
has (state.band_metrics(): acoustics.ir_band_metrics splits the tensors into the room's own bands where they lie and runs Schroeder's
backward integral over every band row; nothing but the tables is downloaded), beside what Sabine and Eyring predict for that band
(acoustics.sabine_rt60_bands, eyring_rt60_bands).  The room is the second one of examples/shoebox_metrics.py, whose one broadband
T30 follows whichever band rings longest.

    python examples/shoebox_band_metrics.py
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


def main():
    table = {k: (np.array(f, dtype=np.float64), np.array(a)) for k, (f, a) in MATERIALS.items()}
    walls = ["plaster", "glass", "plaster", "plaster", "carpet", "plaster"]
    st = core.ShoeboxIRState(ROOM, materials=walls, material_table=table, ir_len=FS, sample_rate=FS, tail=shoebox.ShoeboxTail(seed=7))
    st.add_microphone("mic", CAPSULES)
    st.add_emitters(EMITTERS)
    st.simulate()
    m = st.band_metrics()["mic"]                    # {alias: IRBandMetrics}; every column is (capsules, emitters, bands)
    wide = st.metrics()["mic"]
    sabine, eyring = acoustics.sabine_rt60_bands(ROOM, st.betas), acoustics.eyring_rt60_bands(ROOM, st.betas)
    print("a room of materials (x: plaster, glass; y: plaster; floor: carpet; ceiling: plaster), measured in its own bands")
    print("  band [Hz]   Sabine [s]   Eyring [s]   T30 [s]   EDT [s]   decay in the row [dB]     (mean over capsules and emitters)")
    for b, centre in enumerate(m.centres):
        print(f"  {centre:9.0f} {sabine[b]:12.3f} {eyring[b]:12.3f} {np.nanmean(m.t30[:, :, b]):9.3f} {np.nanmean(m.edt[:, :, b]):9.3f} "
              f"{np.mean(m.dyn_db[:, :, b]):12.1f}")
    print(f"  broadband {'':25s} {np.nanmean(wide.t30):9.3f} {np.nanmean(wide.edt):9.3f} {np.mean(wide.dyn_db):12.1f}")
    assert not m.bad.any()


if __name__ == "__main__":
    main()
