"""tests/ir_metrics_cases.py on the real MI355X (gfx950 build): the scenarios of tests/test_hostemu_ir_metrics.py, the second
capsule's rows past element 2^31 and past byte 2^32 (untouched buffers, skipped when memory is short), and the schedule independence
of the four kernels (whose LDS hand-overs the perturbed builds surround with sleeps): the product library and the `s1` and `s3w`
builds of tests/shake.py give bit-identical tables and knots."""
import numpy as np
import pytest

from tests import ir_metrics_cases as cases
from tests import shake
from tests.wide_offset_cases import need, release, reserve

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
        print(f"\n[gfx950] ir metrics, {name}: worst error / bound {frac:.3g}")


@pytest.mark.parametrize("ir_len", cases.LENGTHS)
def test_parity_and_layouts(gpu, ir_len):
    cases.run_length(gpu, ir_len)


def test_nine_tiles(gpu):
    cases.run_tiled(gpu)


def test_short_row_features(gpu):
    cases.run_features(gpu)


def test_silent_and_non_finite_rows(gpu):
    cases.run_special(gpu)


def test_identity(gpu):
    cases.run_identity(gpu)


@pytest.mark.parametrize("position", ["i31", "b32"])
def test_second_capsule_at_a_wide_stride(gpu, position):
    try:
        cases.run_wide(gpu, position, reserve, need)
    finally:
        release(gpu)


def test_abi_refusals(gpu):
    cases.run_abi_refusals(gpu)


def test_python_errors(gpu):
    cases.run_python_errors(gpu)


def test_state_and_host_arrays(gpu):
    cases.run_state(gpu)


def test_dictionary_round_trip(gpu):
    cases.run_round_trip(gpu)


def test_schedule_independence(gpu):
    """cases.run_shake_rows (each within its bound first) through the product library and the two schedule-perturbed builds:
    bit-identical tables and knots."""
    from audiblelight_amd import _hip, engine

    ref = cases.run_shake_rows(gpu)
    for name, path in shake.existing_or_built(["s1", "s3w"]).items():
        got = cases.run_shake_rows(engine.Renderer(lib=_hip.Library(path)))
        for key in ref:
            assert np.array_equal(cases.bits(got[key]), cases.bits(ref[key])), f"{key}: the {name} build differs from the product library"
