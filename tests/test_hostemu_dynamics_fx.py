"""The device dynamics FX (tests/dynamics_fx_cases.py) on the host-emulated kernel: Compressor and Limiter at four sample rates
against the float64 oracle (fixed parameters, both coefficient orders, the two cutoffs of the time constants, drawn defaults),
edge lengths around the wave and the tile into guarded buffers, the Limiter's structure, silence, a batch against the single-clip
launches, the refusals of the C ABI and of the pack, the classes' reference API, chains on an Event and in a scene, a reference
scene JSON.  The gfx950 build runs the same scenarios, plus one 10 s clip per entry, in tests/test_gpu_dynamics_fx.py."""
import pytest

from audiblelight_amd import _hip, engine, synthesize as syn
from tests import dynamics_fx_cases as cases
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
    cases.run_defaults_drawn(fs)


@pytest.mark.parametrize("n", cases.EDGE_N)
def test_emu_edge_lengths(emu, n):
    cases.run_edge_lengths(emu, n, shift=n % 2)


def test_emu_limiter_structure():
    cases.run_limiter_structure()


def test_emu_silence_and_tiny_input():
    cases.run_silence_and_tiny()


@pytest.mark.parametrize("kind", sorted(cases.KINDS))
def test_emu_batch_equals_single_launches(emu, kind):
    cases.run_batch_equals_singles(emu, kind)


def test_emu_batch_refusals(emu):
    cases.run_batch_refusals(emu)


def test_emu_abi_refusals(emu):
    cases.run_abi_refusals(emu)


def test_emu_class_api():
    cases.run_class_api()


def test_emu_event_chain_stays_on_device(emu, monkeypatch):
    cases.run_event_chain(emu, monkeypatch)


def test_emu_scene_jobs_batch_by_kind(emu, monkeypatch):
    cases.run_scene_batches_by_kind(emu, monkeypatch)


def test_emu_reference_scene_json_with_dynamics_fx(tmp_path):
    cases.run_scene_json(tmp_path)
