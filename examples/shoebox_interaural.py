#!/usr/bin/env python
"""The interaural measures of a binaural listener in a rectangular room, on the device: a listener with a rigid spherical head faces +x
and a source stands 1.5 m away at azimuths of 0, 45 and 90 degrees to the left.  state.pair_metrics() (acoustics.ir_pair_metrics)
correlates the two ear rows of every emitter where the tensor lies and downloads one small table: the ITD (the lag of the
correlation peak) beside Woodworth's (a / c)(theta + sin theta) for a rigid sphere, the ILD, and the inter-aural cross-correlation
coefficient (ISO 3382-1 Annex B) of the early 80 ms and of what follows.  The same head is measured twice: with the direct path
alone (no reflections, no tail), which is what Woodworth's formula describes, and in the room.

    python examples/shoebox_interaural.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from audiblelight_amd import core, shoebox  # noqa: E402

ROOM = (6.0, 5.0, 3.0)
FS = 48000
HEAD = np.array([2.5, 2.0, 1.5])
AZIMUTHS = (0.0, 45.0, 90.0)
DISTANCE = 1.5


def listener(**room):
    st = core.ShoeboxIRState(ROOM, rt60=0.4, sample_rate=FS, **room)
    mic = st.add_binaural_listener("head", HEAD, forward=(1.0, 0.0, 0.0), up=(0.0, 0.0, 1.0))      # left ear first, towards +y
    st.add_emitters([HEAD + DISTANCE * np.array([np.cos(np.deg2rad(az)), np.sin(np.deg2rad(az)), 0.0]) for az in AZIMUTHS])
    st.simulate()
    return st, mic.metadata["sphere"]["radius"]


def main():
    direct, radius = listener(ir_len=FS // 20, max_order=0)                  # the direct path alone
    room, _ = listener(ir_len=FS // 2, tail=shoebox.ShoeboxTail(seed=7))     # reflections and the default diffuse tail
    free = direct.pair_metrics()["head"]            # {alias: IRPairMetrics}; every column is (pairs, emitters): here (1, 3)
    m = room.pair_metrics()["head"]
    print(f"a spherical head of {radius} m, ears at +-100 degrees; lags of +-{m.max_lag} samples at {FS} Hz; a positive ITD: the left ear first")
    print("  azimuth [deg]   Woodworth [us]   direct path: ITD [us]  ILD [dB]   in the room: ITD [us]  ILD [dB]  IACC early  IACC late")
    for n, az in enumerate(AZIMUTHS):
        theta = np.deg2rad(az)
        woodworth = radius / room.c * (theta + np.sin(theta))
        print(f"  {az:13.0f} {1e6 * woodworth:16.1f} {1e6 * free.itd_a[0, n]:23.1f} {free.ild_db_a[0, n]:9.2f} {1e6 * m.itd_e[0, n]:23.1f} "
              f"{m.ild_db_e[0, n]:9.2f} {m.iacc_e[0, n]:11.3f} {m.iacc_l[0, n]:10.3f}")
    print("Woodworth's formula has the ears at +-90 degrees and one arrival.  In the room the early 80 ms hold the first reflections as well,")
    print("each with an ITD of its own: at 1.5 m, beyond the critical distance, the peak of their sum need not be the direct path's.")
    print("The late IACC reads about 0 because the diffuse tail draws independent noise for every row: a real room's does not.")
    assert not m.bad.any() and not free.bad.any()


if __name__ == "__main__":
    main()
