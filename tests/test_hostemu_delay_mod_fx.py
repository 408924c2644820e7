"""The device delay and modulation FX (tests/delay_mod_fx_cases.py) on the host-emulated kernels: every class at four sample
rates against the float64 oracle (fixed parameters and drawn defaults), Delay line lengths around the run and wave sizes,
Chorus with and without feedback at integer delays and at the 110 ms clamp, Phaser centre frequencies, edge lengths into
guarded buffers, the C ABI's refusals, the classes' reference API, a chain on an Event and in a scene, a reference scene
JSON.  The gfx950 build runs the same scenarios, plus 10 s and 60 s clips, in tests/test_gpu_delay_mod_fx.py."""
import pytest

from audiblelight_amd import _hip, engine, synthesize as syn
from tests import delay_mod_fx_cases as cases
from tests import hostemu


@pytest.fixture(scope="module", autouse=True)
def emu():
    r = engine.Renderer(lib=_hip.Library(hostemu.build()), memory=hostemu.NumpyMemory())
    syn.set_renderer(r)
    yield r
    syn.set_renderer(None)


@pytest.mark.parametrize("fs", cases.FS)
def test_emu_every_class_matches_oracle(fs):
    cases.run_class_parity(fs)


@pytest.mark.parametrize("fs", cases.FS)
def test_emu_defaults_drawn(fs):
    cases.run_defaults_drawn(fs, seconds=0.5, seeds=range(2))


@pytest.mark.parametrize("n", [1000, 4099])
def test_emu_delay_lengths(emu, n):
    for D in cases.delay_lengths(n):
        cases.run_delay_edges(emu, n, D, shift=D % 2)


def test_emu_delay_identity_and_clamp():
    cases.run_delay_special()


def test_emu_chorus_regimes():
    cases.run_chorus_regimes()


@pytest.mark.parametrize("fs", cases.FS)
def test_emu_phaser_centres(fs):
    cases.run_phaser_centres(fs)


@pytest.mark.parametrize("n", cases.EDGE_N)
def test_emu_edge_lengths(emu, n):
    cases.run_edge_lengths(emu, n, shift=n % 2)


def test_emu_abi_refusals(emu):
    cases.run_abi_refusals(emu)


def test_emu_class_api():
    cases.run_class_api()


def test_emu_event_chain_stays_on_device(emu, monkeypatch):
    cases.run_event_chain(emu, monkeypatch)


def test_emu_reference_scene_json_with_delay_mod_fx(tmp_path):
    cases.run_scene_json(tmp_path)
