"""tests/ir_band_metrics_cases.py on the real MI355X (gfx950 build): the scenarios of tests/test_hostemu_ir_band_metrics.py, and the
schedule independence of k_ir_band_split and of the passes behind it: one call with half = 300 (more than one tap chunk), five bands
and two passes gives bit-identical band rows, tables and knots through the product library and the `s1` and `s3w` builds of
tests/shake.py (held to the split's bound first)."""
import numpy as np
import pytest

from tests import ir_band_metrics_cases as cases
from tests import shake

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    from audiblelight_amd import engine, synthesize as syn

    r = engine.Renderer()
    assert r.lib.path.endswith("libaudiblelight_hip.so")
    syn.set_renderer(r)
    yield r
    syn.set_renderer(None)
    for name, frac in sorted(cases.WORST.items()):
        print(f"\n[gfx950] ir band metrics, {name}: worst error / bound {frac:.3g}")


@pytest.mark.parametrize("ir_len,half,n_bands,pair", cases.SPLIT_SHAPES)
def test_split_against_the_restatement(gpu, ir_len, half, n_bands, pair):
    cases.run_split_shape(gpu, ir_len, half, n_bands, pair)


def test_split_layouts(gpu):
    cases.run_split_layouts(gpu)


def test_exact_ties(gpu):
    cases.run_exact(gpu)


def test_composition(gpu):
    cases.run_composition(gpu)


def test_non_finite_sample(gpu):
    cases.run_non_finite(gpu)


def test_two_rate_rows(gpu):
    cases.run_meaning(gpu)


def test_abi_refusals(gpu):
    cases.run_abi_refusals(gpu)


def test_python_errors(gpu):
    cases.run_python_errors(gpu)


def test_python_layer(gpu):
    cases.run_python_layer(gpu)


def test_states(gpu, monkeypatch):
    cases.run_state(gpu, cases.FIXTURE, monkeypatch)


def test_schedule_independence(gpu):
    """cases.run_shake_rows through the product library and the two schedule-perturbed builds: bit-identical band rows, tables and
    knots."""
    from audiblelight_amd import _hip, engine

    ref = cases.run_shake_rows(gpu)
    for name, path in shake.existing_or_built(["s1", "s3w"]).items():
        got = cases.run_shake_rows(engine.Renderer(lib=_hip.Library(path)))
        for key in ref:
            assert np.array_equal(cases.bits(got[key]), cases.bits(ref[key])), f"{key}: the {name} build differs from the product library"
