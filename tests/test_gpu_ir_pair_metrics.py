"""tests/ir_pair_metrics_cases.py on the real MI355X (gfx950 build): the scenarios of tests/test_hostemu_ir_pair_metrics.py, and the
schedule independence of k_irp_tiles and k_irp_columns: one call (3 pairs x 5 sources, ir_len 2100, max_lag 300, with curves) gives
bit-identical tables and curves through the product library and the `s1` and `s3w` builds of tests/shake.py (held to the restatement
first)."""
import numpy as np
import pytest

from tests import ir_pair_metrics_cases as cases
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
        print(f"\n[gfx950] ir pair metrics, {name}: worst error / bound {frac:.3g}")


@pytest.mark.parametrize("ir_len", cases.LENGTHS)
def test_against_the_restatement(gpu, ir_len):
    cases.run_length(gpu, ir_len)


def test_pair_and_source_counts(gpu):
    cases.run_sizes(gpu)


def test_window_edges(gpu):
    cases.run_windows(gpu)


def test_layouts_and_identity(gpu):
    cases.run_layouts(gpu)


def test_exact_ties(gpu):
    cases.run_exact(gpu)


def test_coherent_early_independent_late(gpu):
    cases.run_meaning(gpu)


def test_states(gpu):
    cases.run_states(gpu)


def test_abi_refusals(gpu):
    cases.run_abi_refusals(gpu)


def test_python_errors(gpu, monkeypatch):
    cases.run_python_errors(gpu, monkeypatch)


def test_python_layer(gpu):
    cases.run_python_layer(gpu)


def test_shoebox_and_static_states(gpu, monkeypatch):
    cases.run_state(gpu, monkeypatch)


def test_band_composition(gpu):
    cases.run_band_composition(gpu)


def test_schedule_independence(gpu):
    """cases.run_shake_rows through the product library and the two schedule-perturbed builds: bit-identical tables and curves."""
    from audiblelight_amd import _hip, engine

    ref = cases.run_shake_rows(gpu)
    for name, path in shake.existing_or_built(["s1", "s3w"]).items():
        got = cases.run_shake_rows(engine.Renderer(lib=_hip.Library(path)))
        for key in ref:
            assert np.array_equal(cases.bits(got[key]), cases.bits(ref[key])), f"{key}: the {name} build differs from the product library"
