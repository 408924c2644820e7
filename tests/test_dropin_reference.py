"""The drop-in claim, checked against what the reference package defines and returns, stored under tests/golden/
(reference_fuzz_vectors.npz, written by ``tests/golden/differential_fuzz.py --record`` where the reference is installed):
``dropin.install()`` rebinds the functions ``audiblelight.core.Scene.generate`` resolves by lazy import (reference
core.py:1828-1831) on a module named ``audiblelight.synthesize`` that defines the reference's functions, and the entry points
of that module then render the golden scene through the (host-emulated) kernels.  No test here needs the reference itself."""
import os
import sys
import types

import numpy as np
import pytest

from audiblelight_amd import _hip, dropin, engine, synthesize as ours
from tests import hostemu
from tests.conftest import assert_parity

FUZZ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_fuzz_vectors.npz")


@pytest.fixture(scope="module")
def fuzz_golden():
    with np.load(FUZZ) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture()
def reference_synthesize(fuzz_golden):
    """A stand-in for the reference's ``audiblelight.synthesize``, importable under that name: one function for every function the
    real module defines (their names are stored with the goldens), each failing the test if it is ever called.  The stand-in
    and its package are removed from sys.modules afterwards."""
    module = types.ModuleType("audiblelight.synthesize")

    def not_rebound(name):
        def call(*args, **kwargs):
            raise AssertionError(f"the reference's {name} was called: dropin.install() did not rebind it")
        return call

    for name in fuzz_golden["dropin|synthesize_names"]:
        setattr(module, str(name), not_rebound(str(name)))
    package = types.ModuleType("audiblelight")
    package.__path__ = []
    package.synthesize = module
    saved = {k: sys.modules.get(k) for k in ("audiblelight", "audiblelight.synthesize")}
    sys.modules.update({"audiblelight": package, "audiblelight.synthesize": module})
    try:
        yield module
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_install_rebinds_what_scene_generate_imports(reference_synthesize, golden, fuzz_golden):
    from tests.test_hostemu_api import build_g8_scene

    ref_syn = reference_synthesize
    assert set(dropin.REPLACED) <= set(vars(ref_syn)), "install() rebinds a name the reference's module does not define"
    originals = {n: getattr(ref_syn, n) for n in dropin.REPLACED}
    ours.set_renderer(engine.Renderer(lib=_hip.Library(hostemu.build()), memory=hostemu.NumpyMemory()))
    dropin.install()            # no argument: imports audiblelight.synthesize by name, as the reference's Scene.generate does
    try:
        # the two names Scene.generate imports at call time now resolve to the MI355X path
        from audiblelight.synthesize import generate_scene_audio_from_events, render_audio_for_all_scene_events
        assert render_audio_for_all_scene_events is ours.render_audio_for_all_scene_events
        assert generate_scene_audio_from_events is ours.generate_scene_audio_from_events
        scene = build_g8_scene(golden)
        ref_syn.render_audio_for_all_scene_events(scene)
        ref_syn.generate_scene_audio_from_events(scene)
        assert scene.audio["mic000"].dtype == np.float32
        assert_parity(scene.audio["mic000"], golden["g8_scene"], 1e-4)
        # scalar helpers keep the reference's results (its own outputs on these inputs are the check here)
        x = np.linspace(-0.5, 0.7, 101)
        np.testing.assert_allclose(ref_syn.apply_snr(x, 7.0), fuzz_golden["dropin|apply_snr(x, 7.0)"], rtol=1e-6)
        assert ref_syn.db_to_multiplier(-40.0, 0.3) == pytest.approx(float(fuzz_golden["dropin|db_to_multiplier(-40.0, 0.3)"]), rel=1e-6)
    finally:
        dropin.uninstall()
        ours.set_renderer(None)
    for n in dropin.REPLACED:
        assert getattr(ref_syn, n) is originals[n]


def test_differential_fuzz_against_the_reference():
    """tests/golden/differential_fuzz.py on a handful of seeds: random scenes (static / moving / tiled events, snr 0 and negative,
    silent clips, all-zero IRs, events off the scene's ends, coloured ambiences, dry renders) rendered by this package's functions
    over the host-emulated kernels and compared, every array, values and dtypes, with what the REFERENCE's own functions returned
    for the same seeded inputs (stored in tests/golden/reference_fuzz_vectors.npz).  In a process of its own, as the live run
    against the reference is.  (600+ seeds against the reference itself: profiles/r05l_differential_fuzz.txt.)"""
    import subprocess

    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "differential_fuzz.py")
    res = subprocess.run([sys.executable, script, "--replay", FUZZ, "0", "25"], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "317 arrays compared" in res.stdout, res.stdout[-2000:]
    assert "0 outside 1e-4" in res.stdout
