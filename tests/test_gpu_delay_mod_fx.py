"""tests/delay_mod_fx_cases.py on the real MI355X (gfx950 build): the scenarios of tests/test_hostemu_delay_mod_fx.py, plus
10 s and 60 s clips at 48 kHz through every entry point (the lengths the kernels' profile is reported at)."""
import pytest

from tests import delay_mod_fx_cases as cases

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
    cases.run_class_parity(fs, seconds=2.0)


@pytest.mark.parametrize("fs", cases.FS)
def test_defaults_drawn(fs):
    cases.run_defaults_drawn(fs, seconds=1.0, seeds=range(4))


@pytest.mark.parametrize("n", [1000, 4099, 100003])
def test_delay_lengths(gpu, n):
    for D in cases.delay_lengths(n):
        cases.run_delay_edges(gpu, n, D, shift=D % 2)


def test_delay_identity_and_clamp():
    cases.run_delay_special()


def test_chorus_regimes():
    cases.run_chorus_regimes(seconds=1.0)


@pytest.mark.parametrize("fs", cases.FS)
def test_phaser_centres(fs):
    cases.run_phaser_centres(fs)


@pytest.mark.parametrize("n", cases.EDGE_N)
def test_edge_lengths(gpu, n):
    cases.run_edge_lengths(gpu, n, shift=n % 2)


@pytest.mark.parametrize("n", [cases.CLIP_10S, cases.CLIP_60S])
@pytest.mark.parametrize("kind,kw", [("delay", dict(D=1, fb=0.9, mix=0.5)), ("delay", dict(D=480, fb=0.5, mix=0.4)),
                                     ("delay", dict(D=48000, fb=0.3, mix=0.5)), ("chorus", dict(fb=0.0)),
                                     ("chorus", dict(fb=0.5)), ("phaser", dict())])
def test_long_clips(gpu, kind, kw, n):
    cases.run_long(gpu, kind, n, **kw)


def test_abi_refusals(gpu):
    cases.run_abi_refusals(gpu)


def test_class_api():
    cases.run_class_api()


def test_event_chain_stays_on_device(gpu, monkeypatch):
    cases.run_event_chain(gpu, monkeypatch)


def test_reference_scene_json_with_delay_mod_fx(tmp_path):
    cases.run_scene_json(tmp_path)
