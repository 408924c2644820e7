#!/usr/bin/env python
"""Render a talker -- a cardioid source -- in a rectangular room, once turned TOWARDS a first-order ambisonic listener and once
turned AWAY from it, through air that absorbs: the impulse responses are generated on the MI355X with the source's pattern and
exp(-m d) on every image, and a diffuse tail whose level and decay follow both.

    python examples/shoebox_talker.py [output_dir]

What turns with the talker is the direct sound and the first reflections, not the reverberation: the early-to-late ratio printed
at the end (the first 5 ms from the direct arrival against everything after) is the distance cue a listener hears move.  Turned
away, the cardioid sends nothing along the direct path at all: what is left of the early part are the first reflections.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from audiblelight_amd import core, shoebox  # noqa: E402


def main(out_dir="shoebox_talker_out"):
    rng = np.random.default_rng(0)
    sr = 24000
    room, listener, talker = (6.0, 5.0, 3.0), np.array([3.1, 2.4, 1.5]), np.array([1.4, 3.6, 1.6])
    towards = (listener - talker) / np.linalg.norm(listener - talker)
    air = float(shoebox.air_absorption(4000.0))          # one broadband coefficient: the air at 4 kHz, 20 degrees, 50 %
    speech = rng.standard_normal(2 * sr).astype(np.float32) * np.repeat(rng.uniform(0.0, 1.0, 16), sr // 8).astype(np.float32)
    ratios = {}
    for name, direction in (("towards", towards), ("away", -towards)):
        state = core.ShoeboxIRState(room, rt60=0.5, ir_len=sr, sample_rate=sr, tail=shoebox.ShoeboxTail(seed=7), air=air)
        state.add_foa_listener("foa", listener)                                       # AmbiX: W, Y, Z, X
        state.add_emitters([talker], alias="talker", patterns=shoebox.cardioid(direction))
        scene = core.Scene(duration=4.0, state=state, sample_rate=sr)
        scene.add_event(core.Event("talker", speech, sr, snr=15, scene_start=0.5))
        audio = scene.generate(output_dir=os.path.join(out_dir, name), metadata_dcase=False)
        w = np.asarray(state.irs["foa"])[0, 0].astype(np.float64)                    # the W channel's impulse response
        t0 = int(np.linalg.norm(listener - talker) / state.c * sr)
        early, late = (w[: t0 + sr // 200] ** 2).sum(), (w[t0 + sr // 200:] ** 2).sum()      # 5 ms from the direct arrival, and the rest
        ratios[name] = 10.0 * np.log10(early / late)
        print(f"{name:8s}: scene {audio['foa'].shape}, peak {np.abs(audio['foa']).max():.3e}; early-to-late ratio of W "
              f"{ratios[name]:6.1f} dB -> {out_dir}/{name}/audio_out_foa.wav")
        # the metadata carries the emitter's pattern and the air: the scene renders again from its JSON
        again = core.Scene.from_json(os.path.join(out_dir, name, "metadata_out.json"), clips={a: e._raw for a, e in scene.events.items()})
        assert all(np.array_equal(again.generate()[mic], audio[mic]) for mic in audio)
    print(f"turning the talker away moves the early-to-late ratio by {ratios['towards'] - ratios['away']:.1f} dB")


if __name__ == "__main__":
    main(*sys.argv[1:2])
