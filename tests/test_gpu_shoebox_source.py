"""tests/shoebox_source_cases.py on the real MI355X (gfx950 build): the scenarios of tests/test_hostemu_shoebox_source.py, and the rows
of the new entries through the schedule-perturbed builds."""
import numpy as np
import pytest

from tests import shake
from tests import shoebox_source_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    from audiblelight_amd import engine, synthesize as syn

    r = engine.Renderer()
    assert r.lib.path.endswith("libaudiblelight_hip.so")
    syn.set_renderer(r)
    yield r
    syn.set_renderer(None)


@pytest.mark.parametrize("room,order,kind,air", cases.PARITY)
def test_parity_with_restatement(gpu, room, order, kind, air):
    cases.run_parity(gpu, room, order, kind, air)


@pytest.mark.parametrize("ir_len", cases.EDGE_LEN)
def test_edge_row_lengths(gpu, ir_len):
    cases.run_edge_length(gpu, ir_len)


def test_capsule_one_centimetre_from_its_source(gpu):
    cases.run_close_capsule(gpu)


def test_omni_sources_without_air_are_the_old_entries(gpu):
    cases.run_omni_ties(gpu)


def test_order_zero_in_closed_form(gpu):
    cases.run_order_zero(gpu)


def test_reciprocity_against_the_receiver_kernel(gpu):
    cases.run_reciprocity(gpu)


def test_equal_bands_are_the_broadband_entry(gpu):
    cases.run_equal_bands(gpu)


@pytest.mark.parametrize("M,F,ir_len,kind,order,pitch,sid0,cid0", cases.TAIL_PARITY)
def test_tail_parity_with_restatement(gpu, M, F, ir_len, kind, order, pitch, sid0, cid0):
    cases.run_tail_parity(gpu, M, F, ir_len, kind, order, pitch, sid0, cid0)


def test_tail_identity_and_workspace(gpu):
    cases.run_tail_identity(gpu)


def test_abi_refusals(gpu):
    cases.run_abi_refusals(gpu)


def test_python_errors(gpu):
    cases.run_python_errors(gpu)


def test_state_and_json_round_trip(gpu):
    cases.run_state(gpu)


def test_talker_facing_and_away(gpu):
    cases.run_talker_irs(gpu)
    cases.run_talker_scene(gpu)


def test_air_in_a_hard_room(gpu):
    cases.run_air_scene(gpu)


def test_schedule_independence(gpu):
    """cases.run_shake_rows (the new entries without a tail and with one, each within its bound first) through the product library
    and the two schedule-perturbed builds: bit-identical rows."""
    from audiblelight_amd import _hip, engine

    ref = cases.run_shake_rows(gpu)
    for name, path in shake.existing_or_built(["s1", "s3w"]).items():
        got = cases.run_shake_rows(engine.Renderer(lib=_hip.Library(path)))
        for key in ref:
            assert np.array_equal(cases.bits(got[key]), cases.bits(ref[key])), f"{key}: the {name} build differs from the product library"
