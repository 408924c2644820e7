"""The device time-stretch FX (tests/time_stretch_fx_cases.py) on the host-emulated kernels: SpeedUp and PitchShift against the
float64 oracle of the definition (fixed parameters, drawn defaults), edge lengths and tile edges through ``al_fx_time_stretch``
into guarded buffers with a guarded workspace, more frames than one launch group, the resampler alone, where a tone lands,
silence and the identity parameters, the refusals of the C ABI, the classes' reference API, chains on an Event and in a scene, a
reference scene JSON.  The gfx950 build runs the same scenarios, plus one 10 s clip, in tests/test_gpu_time_stretch_fx.py."""
import pytest

from audiblelight_amd import _hip, engine, synthesize as syn
from tests import hostemu
from tests import time_stretch_fx_cases as cases


@pytest.fixture(scope="module", autouse=True)
def emu():
    r = engine.Renderer(lib=_hip.Library(hostemu.build()), memory=hostemu.NumpyMemory())
    syn.set_renderer(r)
    yield r
    syn.set_renderer(None)


@pytest.mark.parametrize("case", range(6))
@pytest.mark.parametrize("fs", cases.FS)
def test_emu_every_class_matches_oracle(fs, case):
    cases.run_class_parity(fs, case)


@pytest.mark.parametrize("fs", cases.FS)
def test_emu_defaults_drawn(fs):
    cases.run_defaults_drawn(fs)


@pytest.mark.parametrize("n", cases.EDGE_N)
def test_emu_edge_lengths(emu, n):
    cases.run_edge_lengths(emu, n)


def test_emu_tile_edges(emu):
    cases.run_tile_edges(emu)


def test_emu_past_one_launch_group(emu):
    cases.run_past_one_group(emu)


@pytest.mark.parametrize("m,n", cases.RESAMPLE_CASES)
def test_emu_resampler_alone(emu, m, n):
    cases.run_resampler(emu, m, n)


def test_emu_tone_lands_where_it_should():
    cases.run_structure()


def test_emu_silence_and_identity(emu, monkeypatch):
    cases.run_silence_and_identity(emu, monkeypatch)


def test_emu_abi_refusals(emu):
    cases.run_abi_refusals(emu)


def test_emu_class_api():
    cases.run_class_api()


def test_emu_event_chain_stays_on_device(emu, monkeypatch):
    cases.run_event_chain(emu, monkeypatch)


def test_emu_reference_scene_json_with_time_stretch_fx(tmp_path):
    cases.run_scene_json(tmp_path)
