#!/usr/bin/env python
"""Render a scene in a rectangular room whose impulse responses are generated on the MI355X (image-source method): no IR array is
ever made on the host or sent over PCIe.

    python examples/shoebox_room.py [--tail] [output_dir]

--tail: two seconds of IR instead of half a second, exact images up to the mixing time (42 ms) and a diffuse tail of seeded noise
past it (shoebox.ShoeboxTail), with no order limit: the long rows cost a write of their bytes.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from audiblelight_amd import core, shoebox  # noqa: E402


def main(out_dir="shoebox_out", tail=False):
    rng = np.random.default_rng(0)
    sr = 24000
    if tail:
        # the same room, two seconds of IR: every image of the first 53 ms, then the diffuse tail
        state = core.ShoeboxIRState((6.0, 5.0, 3.0), rt60=0.4, ir_len=2 * sr, sample_rate=sr, tail=shoebox.ShoeboxTail(seed=2024))
    else:
        # a 6 x 5 x 3 m room with a reverberation time of 0.4 s (Sabine), half a second of IR, images up to order 20
        state = core.ShoeboxIRState((6.0, 5.0, 3.0), rt60=0.4, ir_len=sr // 2, sample_rate=sr, max_order=20)
    centre, radius = np.array([3.1, 2.4, 1.5]), 0.042
    tetra = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]) / np.sqrt(3.0)
    state.add_microphone("mic000", centre + radius * tetra)            # four omnidirectional point capsules
    # the same tetrahedron as four cardioids that look outwards, and a first-order ambisonic listener at its centre (AmbiX: W Y Z X)
    state.add_microphone("mic001", centre + radius * tetra, patterns=[shoebox.cardioid(v) for v in tetra])
    state.add_foa_listener("foa000", centre, order="wyzx")
    state.add_emitters([[1.2, 3.9, 1.6]], alias="static")              # one IR column
    state.add_emitters(np.linspace([4.8, 0.8, 1.2], [4.9, 4.2, 1.7], 4), alias="moving")   # a trajectory of four points
    scene = core.Scene(duration=8.0, state=state, sample_rate=sr)
    scene.add_event(core.Event("static", rng.standard_normal(2 * sr).astype(np.float32), sr, snr=15, scene_start=0.5))
    scene.add_event(core.Event("moving", rng.standard_normal(4 * sr).astype(np.float32), sr, snr=20, scene_start=3.0, n_emitters=4))
    audio = scene.generate(output_dir=out_dir, metadata_dcase=False)
    for mic, buf in audio.items():
        print(f"{mic}: {buf.shape} float32, peak {np.abs(buf).max():.3e} -> {out_dir}/audio_out_{mic}.wav")
    # the metadata carries the room: the scene renders again from its JSON and the clips alone
    again = core.Scene.from_json(os.path.join(out_dir, "metadata_out.json"), clips={a: e._raw for a, e in scene.events.items()})
    audio_again = again.generate()
    assert all(np.array_equal(audio_again[mic], audio[mic]) for mic in audio)
    print("re-rendered from metadata_out.json bit-identically, IRs generated again on the device")


if __name__ == "__main__":
    main(*[a for a in sys.argv[1:] if a != "--tail"], tail="--tail" in sys.argv[1:])
