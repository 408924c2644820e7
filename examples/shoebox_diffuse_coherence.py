#!/usr/bin/env python
"""The coherence of the diffuse tail between two capsules, on the device: pairs of omnidirectional capsules 2, 5 and 17 cm apart in
a rectangular room, once with the independent tail and once with shoebox.ShoeboxTail(coherent=True), whose rows share 64 seeded plane
waves.  state.pair_metrics() correlates the two rows of every pair where the tensor lies: the late IACC (the peak over +-1 ms) and
the correlation at lag 0, beside what a diffuse field gives at that spacing, sin(kd) / (kd) averaged over the band up to the Nyquist
frequency.  The short interpolation kernel of the plane waves' fractional delays (half_taps = 4) rolls off below the Nyquist
frequency, where the coherence is lowest, so the generated figures lie somewhat above the band average.

    python examples/shoebox_diffuse_coherence.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from audiblelight_amd import core, shoebox  # noqa: E402

ROOM = (6.0, 5.0, 3.0)
FS = 16000
POINT = np.array([2.5, 2.0, 1.5])
SPACINGS = (0.02, 0.05, 0.17)


def pair_state(coherent):
    st = core.ShoeboxIRState(ROOM, rt60=0.5, ir_len=FS, sample_rate=FS, tail=shoebox.ShoeboxTail(seed=7, coherent=coherent))
    for d in SPACINGS:      # a microphone is a group: its rows share their plane waves, two microphones share nothing
        st.add_microphone(f"pair {100 * d:.0f} cm", np.stack([POINT, POINT + [d, 0.0, 0.0]]))
    st.add_emitters([[4.5, 3.5, 1.2]])
    st.simulate()
    return st


def main():
    states = {flag: pair_state(flag) for flag in (False, True)}
    f = np.linspace(0.0, 0.5 * FS, 4001)
    print(f"two omnis in a {ROOM} m room at {FS} Hz, one second of response; late window: from 80 ms past the direct sound")
    print("  spacing [cm]   band mean of sin(kd)/(kd)   independent: IACC late  lag 0   coherent: IACC late  lag 0")
    for d in SPACINGS:
        alias = f"pair {100 * d:.0f} cm"
        model = float(np.mean(np.sinc(2.0 * f * d / states[True].c)))
        row = []
        for flag in (False, True):
            peak = states[flag].pair_metrics(alias)[alias]
            lag0 = states[flag].pair_metrics(alias, max_lag=0)[alias]
            row += [float(peak.iacc_l[0, 0]), float(lag0.peak_l[0, 0])]
        print(f"  {100 * d:12.0f} {model:26.3f} {row[0]:24.3f} {row[1]:6.3f} {row[2]:21.3f} {row[3]:6.3f}")
    print("The independent tail reads about 0 at every spacing; the coherent one follows the diffuse-field law as far as one second of")
    print("noise can show it (a correlation estimate from N_eff samples scatters by about 1 / sqrt(N_eff)).")


if __name__ == "__main__":
    main()
