"""tests/dynamics_fx_cases.py on the real MI355X (gfx950 build): the scenarios of tests/test_hostemu_dynamics_fx.py, plus one
10 s clip at 48 kHz through each entry point (a length the kernel's profile is reported at)."""
import pytest

from tests import dynamics_fx_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    from audiblelight_amd import engine, synthesize as syn

    r = engine.Renderer()
    assert r.lib.path.endswith("libaudiblelight_hip.so")
    syn.set_renderer(r)
    yield r
    syn.set_renderer(None)


@pytest.mark.parametrize("fs", cases.FS)
def test_every_class_matches_oracle(fs):
    cases.run_class_parity(fs)


@pytest.mark.parametrize("fs", cases.FS)
def test_defaults_drawn(fs):
    cases.run_defaults_drawn(fs)


@pytest.mark.parametrize("n", cases.EDGE_N)
def test_edge_lengths(gpu, n):
    cases.run_edge_lengths(gpu, n, shift=n % 2)


def test_limiter_structure():
    cases.run_limiter_structure()


def test_silence_and_tiny_input():
    cases.run_silence_and_tiny()


@pytest.mark.parametrize("kind", sorted(cases.KINDS))
def test_batch_equals_single_launches(gpu, kind):
    cases.run_batch_equals_singles(gpu, kind)


def test_batch_refusals(gpu):
    cases.run_batch_refusals(gpu)


def test_abi_refusals(gpu):
    cases.run_abi_refusals(gpu)


def test_class_api():
    cases.run_class_api()


def test_event_chain_stays_on_device(gpu, monkeypatch):
    cases.run_event_chain(gpu, monkeypatch)


def test_scene_jobs_batch_by_kind(gpu, monkeypatch):
    cases.run_scene_batches_by_kind(gpu, monkeypatch)


def test_reference_scene_json_with_dynamics_fx(tmp_path):
    cases.run_scene_json(tmp_path)


@pytest.mark.parametrize("kind", sorted(cases.KINDS))
def test_long_clip(gpu, kind):
    cases.run_long(gpu, kind)
