"""The device filter FX (tests/filter_fx_cases.py) on the host-emulated kernels: every class at four sample rates against the
float64 sosfilt oracle, the two cases float32 state cannot meet, edge lengths into guarded buffers, degenerate cutoffs, the C
ABI's refusals, the classes' reference API, a chain on an Event and in a scene, a reference scene JSON.  The gfx950 build runs
the same scenarios, plus 10 s and 60 s clips, in tests/test_gpu_filter_fx.py."""
import pytest

from audiblelight_amd import _hip, engine, synthesize as syn
from tests import filter_fx_cases as cases
from tests import hostemu, kernel_edges as ke


@pytest.fixture(scope="module", autouse=True)
def emu():
    r = engine.Renderer(lib=_hip.Library(hostemu.build()), memory=hostemu.NumpyMemory())
    syn.set_renderer(r)
    yield r
    syn.set_renderer(None)


@pytest.mark.parametrize("fs", cases.FS)
def test_emu_every_class_matches_oracle(fs):
    cases.run_class_parity(fs)


@pytest.mark.parametrize("label", [label for label, _ in cases.HARD])
def test_emu_float64_state_cases(label):
    cases.run_hard_case(label)


def test_emu_sinusoid_gains():
    cases.run_sinusoid_gains()


@pytest.mark.parametrize("k", [1, 8, 20])
@pytest.mark.parametrize("n", cases.EDGE_SOS_N)
def test_emu_sos_edge_lengths(emu, n, k):
    cases.run_sos_edges(emu, n, k, shift=n % 2)


@pytest.mark.parametrize("n", [1, 65, 1025, 16385])
def test_emu_sos_in_place(emu, n):
    cases.run_sos_edges(emu, n, 8, shift=1, in_place=True)


def test_emu_degenerate_cutoffs():
    cases.run_degenerate_cutoffs()


def test_emu_argument_errors():
    cases.run_argument_errors()


def test_emu_abi_refusals(emu):
    cases.run_abi_refusals(emu)


def test_emu_class_api():
    cases.run_class_api()


def test_emu_event_chain_stays_on_device(emu):
    cases.run_event_chain(emu)


def test_emu_reference_scene_json_with_filters(tmp_path):
    cases.run_scene_json(tmp_path)
