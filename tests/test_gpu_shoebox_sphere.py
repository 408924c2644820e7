"""tests/shoebox_sphere_cases.py on the real MI355X (gfx950 build): the scenarios of tests/test_hostemu_shoebox_sphere.py, plus the
schedule independence of the sphere's gather and combine kernels (one-wave workgroups, whose LDS hand-overs the perturbed builds
surround with sleeps; the workspace hand-over from one launch and pass to the next is ordered by the stream): the product library
and the `s1` and `s3w` builds of tests/shake.py give bit-identical rows."""
import numpy as np
import pytest

from tests import shake
from tests import shoebox_sphere_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    from audiblelight_amd import engine, synthesize as syn

    r = engine.Renderer()
    assert r.lib.path.endswith("libaudiblelight_hip.so")
    syn.set_renderer(r)
    yield r
    syn.set_renderer(None)


@pytest.mark.parametrize("room,order,n_orders,half,pairs,ir_len,table", cases.PARITY)
def test_parity_with_restatement(gpu, room, order, n_orders, half, pairs, ir_len, table):
    cases.run_parity(gpu, room, order, n_orders, half, pairs, ir_len, table)


@pytest.mark.parametrize("ir_len", cases.EDGE_LEN)
def test_edge_lengths(gpu, ir_len):
    cases.run_edge_length(gpu, ir_len)


def test_source_on_a_capsule_axis_at_two_radii(gpu):
    cases.run_on_axis(gpu)


def test_source_patterns_and_air(gpu):
    cases.run_source_and_air(gpu)


def test_one_order_is_the_omni_entry(gpu):
    cases.run_omni_tie(gpu)


def test_two_orders_are_the_first_order_entry(gpu):
    cases.run_first_order_tie(gpu)


def test_null_arguments(gpu):
    cases.run_null_arguments(gpu)


def test_tail_past_the_row_is_the_entry_without_a_tail(gpu):
    cases.run_no_tail(gpu)


def test_past_the_split_is_the_one_band_tail(gpu):
    cases.run_past_the_split(gpu)


@pytest.mark.parametrize("M,F,ir_len,table,pairs,order,pitch,sid0,cid0,per_pass", cases.TAIL_PARITY)
def test_tail_parity_with_restatement(gpu, M, F, ir_len, table, pairs, order, pitch, sid0, cid0, per_pass):
    cases.run_tail_parity(gpu, M, F, ir_len, table, pairs, order, pitch, sid0, cid0, per_pass)


def test_identity_and_workspace(gpu):
    cases.run_identity(gpu)


def test_binaural_scene(gpu, monkeypatch, tmp_path):
    cases.run_binaural_scene(gpu, monkeypatch, tmp_path)


def test_state_and_json_round_trip(gpu):
    cases.run_state(gpu)


def test_round_trip_keeps_the_directions_bits(gpu):
    cases.run_round_trip_directions(gpu)


def test_abi_refusals(gpu):
    cases.run_abi_refusals(gpu)


def test_python_errors(gpu):
    cases.run_python_errors(gpu)


def test_schedule_independence(gpu):
    """cases.run_shake_rows (the entry without a tail and with one, each within its bound first) through the product library and
    the two schedule-perturbed builds: bit-identical rows."""
    from audiblelight_amd import _hip, engine

    ref = cases.run_shake_rows(gpu)
    for name, path in shake.existing_or_built(["s1", "s3w"]).items():
        got = cases.run_shake_rows(engine.Renderer(lib=_hip.Library(path)))
        for key in ref:
            assert np.array_equal(cases.bits(got[key]), cases.bits(ref[key])), f"{key}: the {name} build differs from the product library"
