"""tests/filter_fx_cases.py on the real MI355X (gfx950 build): the scenarios of tests/test_hostemu_filter_fx.py, plus 10 s and
60 s clips at 48 kHz through 1 and 8 sections (the lengths the kernel's profile is reported at)."""
import pytest

from tests import filter_fx_cases as cases

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
    cases.run_class_parity(fs, seconds=4.0)


@pytest.mark.parametrize("label", [label for label, _ in cases.HARD])
def test_float64_state_cases(label):
    cases.run_hard_case(label, seconds=4.0)


def test_sinusoid_gains():
    cases.run_sinusoid_gains()


@pytest.mark.parametrize("k", [1, 8, 20])
@pytest.mark.parametrize("n", cases.EDGE_SOS_N)
def test_sos_edge_lengths(gpu, n, k):
    cases.run_sos_edges(gpu, n, k, shift=n % 2)


@pytest.mark.parametrize("n", [1, 65, 1025, 16385, 2 ** 20 + 7])
def test_sos_in_place(gpu, n):
    cases.run_sos_edges(gpu, n, 8, shift=1, in_place=True)


@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("n", [cases.CLIP_10S, cases.CLIP_60S])
def test_sos_long_clips(gpu, n, k):
    cases.run_sos_long(gpu, n, k)


@pytest.mark.parametrize("n", [cases.CLIP_10S, cases.CLIP_60S])
def test_sos_long_clips_guarded(gpu, n):
    cases.run_sos_edges(gpu, n, 8)


def test_degenerate_cutoffs():
    cases.run_degenerate_cutoffs()


def test_argument_errors():
    cases.run_argument_errors()


def test_abi_refusals(gpu):
    cases.run_abi_refusals(gpu)


def test_class_api():
    cases.run_class_api()


def test_event_chain_stays_on_device(gpu):
    cases.run_event_chain(gpu)


def test_reference_scene_json_with_filters(tmp_path):
    cases.run_scene_json(tmp_path)
