#!/usr/bin/env python
"""Render a scene in a rectangular room whose walls are MATERIALS with octave-band absorption (carpet on the floor, acoustic tile
on the ceiling, brick, glass and plaster around): the impulse responses are generated on the MI355X with a reflection coefficient
per wall and band, and a diffuse tail that decays at each band's own rate.

    python examples/shoebox_materials.py MATERIALS_JSON [output_dir]

MATERIALS_JSON: a material file in the layout {"materials": [{"name": ..., "absorption": [f0, a0, f1, a1, ...]}, ...]}; under the
drop-in package that is audiblelight.worldstate.MATERIALS_JSON.  The package ships none.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from audiblelight_amd import core, shoebox  # noqa: E402

# (x0, x1, y0, y1, z0, z1): two brick walls, a glass front, plaster opposite, carpet below, acoustic tile above
WALLS = ("Brick", "Brick", "Glass", "Plaster on Brick", "Carpet, Heavy", "Acoustic Tile")


def main(materials_json, out_dir="shoebox_materials_out"):
    rng = np.random.default_rng(0)
    sr = 24000
    table = shoebox.load_materials(materials_json)
    bands = shoebox.ShoeboxBands(shoebox.OCTAVE_CENTRES, half=512)
    betas = shoebox.material_betas(table, WALLS, bands.centres)
    for name, row in zip(WALLS, betas):
        print(f"{name:18s} absorption at {[int(f) for f in bands.centres]} Hz: {np.round(1.0 - row * row, 2).tolist()}")
    state = core.ShoeboxIRState((6.0, 5.0, 3.0), materials=WALLS, material_table=table, bands=bands, ir_len=sr, sample_rate=sr,
                                tail=shoebox.ShoeboxTail(seed=2024))
    centre, radius = np.array([3.1, 2.4, 1.5]), 0.042
    tetra = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]) / np.sqrt(3.0)
    state.add_microphone("mic000", centre + radius * tetra)
    state.add_emitters([[1.2, 3.9, 1.6]], alias="static")
    state.add_emitters(np.linspace([4.8, 0.8, 1.2], [4.9, 4.2, 1.7], 4), alias="moving")
    scene = core.Scene(duration=8.0, state=state, sample_rate=sr)
    scene.add_event(core.Event("static", rng.standard_normal(2 * sr).astype(np.float32), sr, snr=15, scene_start=0.5))
    scene.add_event(core.Event("moving", rng.standard_normal(4 * sr).astype(np.float32), sr, snr=20, scene_start=3.0, n_emitters=4))
    audio = scene.generate(output_dir=out_dir, metadata_dcase=False)
    for mic, buf in audio.items():
        print(f"{mic}: {buf.shape} float32, peak {np.abs(buf).max():.3e} -> {out_dir}/audio_out_{mic}.wav")
    # the decay per octave of one IR: the energy of the second quarter second over that of the first, in dB
    ir = np.asarray(state.irs["mic000"])[0, 0].astype(np.float64)
    freqs = np.fft.rfftfreq(sr // 4, 1.0 / sr)
    first, second = (np.abs(np.fft.rfft(ir[i * sr // 4: (i + 1) * sr // 4])) ** 2 for i in (0, 1))
    for f in bands.centres:
        octave = (freqs >= f / np.sqrt(2.0)) & (freqs < f * np.sqrt(2.0))
        print(f"{int(f):5d} Hz: {10.0 * np.log10(second[octave].sum() / first[octave].sum()):6.1f} dB from the first quarter second to the second")
    # the metadata carries betas, bands and material names: the scene renders again from its JSON without the material file
    again = core.Scene.from_json(os.path.join(out_dir, "metadata_out.json"), clips={a: e._raw for a, e in scene.events.items()})
    audio_again = again.generate()
    assert all(np.array_equal(audio_again[mic], audio[mic]) for mic in audio)
    print("re-rendered from metadata_out.json bit-identically, without the material file")


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    main(*sys.argv[1:3])
