#!/usr/bin/env python
"""Recording of the accumulate dispatch: al_spectral_mac_variant over tests/mac_regimes.py::SWEEP_AXES (every descriptor field plan_mac
reads, both sides of every threshold), from the host build of the library (plan_mac is host code).

Run at commit 6db8681, the last one whose al_spectral_mac spelled the choice of instantiation as if / switch chains over template
arguments; the table-driven dispatch that replaced them must reproduce every pair (tests/test_host_logic.py).  Re-run it only for a
change that is MEANT to alter the dispatch, and say so in that change.

    python tests/golden/make_mac_dispatch_sweep.py      ->  tests/golden/mac_dispatch_sweep.npz
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from audiblelight_amd import _hip  # noqa: E402
from tests import hostemu, mac_regimes as mr  # noqa: E402


def main():
    static, moving = mr.dispatch_sweep(_hip.Library(hostemu.build()))
    # the moving code depends on neither the flag word's low bits nor the clip length: int16 holds it (0, 612, 624)
    np.savez_compressed(mr.SWEEP_FIXTURE, static_code=static, moving_code=moving.astype(np.int16),
                        **{name: np.asarray(values, np.int32) for name, values in mr.SWEEP_AXES})
    print(f"{static.size} descriptors, {len(np.unique(static))} static codes, {len(np.unique(moving))} moving codes, "
          f"{os.path.getsize(mr.SWEEP_FIXTURE)} bytes")


if __name__ == "__main__":
    main()
