"""tests/time_stretch_fx_cases.py on the real MI355X (gfx950 build): the scenarios of tests/test_hostemu_time_stretch_fx.py,
plus one 10 s clip at 48 kHz through ``al_fx_time_stretch`` (the length the kernels' profile is reported at)."""
import pytest

from tests import time_stretch_fx_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    from audiblelight_amd import engine, synthesize as syn

    r = engine.Renderer()
    assert r.lib.path.endswith("libaudiblelight_hip.so")
    syn.set_renderer(r)
    yield r
    syn.set_renderer(None)


@pytest.mark.parametrize("case", range(6))
@pytest.mark.parametrize("fs", cases.FS)
def test_every_class_matches_oracle(fs, case):
    cases.run_class_parity(fs, case)


@pytest.mark.parametrize("fs", cases.FS)
def test_defaults_drawn(fs):
    cases.run_defaults_drawn(fs)


@pytest.mark.parametrize("n", cases.EDGE_N)
def test_edge_lengths(gpu, n):
    cases.run_edge_lengths(gpu, n)


def test_tile_edges(gpu):
    cases.run_tile_edges(gpu)


def test_past_one_launch_group(gpu):
    cases.run_past_one_group(gpu)


@pytest.mark.parametrize("m,n", cases.RESAMPLE_CASES)
def test_resampler_alone(gpu, m, n):
    cases.run_resampler(gpu, m, n)


def test_tone_lands_where_it_should():
    cases.run_structure()


def test_silence_and_identity(gpu, monkeypatch):
    cases.run_silence_and_identity(gpu, monkeypatch)


def test_abi_refusals(gpu):
    cases.run_abi_refusals(gpu)


def test_class_api():
    cases.run_class_api()


def test_event_chain_stays_on_device(gpu, monkeypatch):
    cases.run_event_chain(gpu, monkeypatch)


def test_reference_scene_json_with_time_stretch_fx(tmp_path):
    cases.run_scene_json(tmp_path)


def test_long_clip(gpu):
    cases.run_long(gpu)
