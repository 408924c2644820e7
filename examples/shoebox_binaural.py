#!/usr/bin/env python
"""Render a BINAURAL scene in a rectangular room: a listener with a rigid spherical head faces +x and a talker stands 1.2 m to the
left.  The impulse responses are generated on the MI355X with the scattering of every image off the head (level and time differences
between the ears, no pinna and no torso) and a diffuse tail; the scene is written as a two-channel WAV, left first.

    python examples/shoebox_binaural.py [output_dir]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from audiblelight_amd import core, shoebox  # noqa: E402


def main(out_dir="shoebox_binaural_out"):
    rng = np.random.default_rng(0)
    sr = 48000
    state = core.ShoeboxIRState((4.1, 3.3, 2.6), rt60=0.35, ir_len=sr // 2, sample_rate=sr, tail=shoebox.ShoeboxTail(seed=2024))
    head, talker = np.array([2.0, 1.4, 1.3]), np.array([2.0, 2.6, 1.3])
    mic = state.add_binaural_listener("head", head, forward=(1.0, 0.0, 0.0), up=(0.0, 0.0, 1.0))
    sphere = mic.metadata["sphere"]
    print(f"head: radius {sphere['radius']} m, {sphere['n_orders']} Legendre orders, filters of {2 * sphere['half'] + 1} taps; ears at "
          f"{np.round(mic.metadata['coordinates_absolute'], 3).tolist()}")
    state.add_emitters([talker], alias="talker")
    scene = core.Scene(duration=3.0, state=state, sample_rate=sr)
    speech = rng.standard_normal(2 * sr).astype(np.float32)
    scene.add_event(core.Event("talker", speech, sr, snr=15, scene_start=0.5))
    audio = scene.generate(output_dir=out_dir, metadata_dcase=False)["head"]
    print(f"head: {audio.shape} float32 (left, right), peak {np.abs(audio).max():.3e} -> {out_dir}/audio_out_head.wav")
    # the interaural differences of the direct path, read off the two IRs
    ir = np.asarray(state.irs["head"])[:, 0].astype(np.float64)
    arrival = int(np.linalg.norm(talker - head) * sr / state.c)
    win = ir[:, arrival - 90: arrival + 100]          # the first reflection comes 196 samples after the direct path
    energy = (win * win).sum(axis=1)
    centroid = (win * win) @ np.arange(win.shape[1]) / energy
    geometric = sphere["radius"] * sr / state.c * (np.cos(np.deg2rad(10.0)) + np.deg2rad(80.0))
    print(f"direct path: left ear {10.0 * np.log10(energy[0] / energy[1]):.1f} dB above the right, right ear {centroid[1] - centroid[0]:.1f} "
          f"samples later (the path round a sphere: {geometric:.1f})")
    # the metadata carries the head: the scene renders again from its JSON
    again = core.Scene.from_json(os.path.join(out_dir, "metadata_out.json"), clips={"talker": speech})
    assert np.array_equal(again.generate()["head"], audio)
    print("re-rendered from metadata_out.json bit-identically")


if __name__ == "__main__":
    main(*sys.argv[1:2])
