"""tests/shoebox_coherent_cases.py on the real MI355X (gfx950 build): the scenarios of tests/test_hostemu_shoebox_coherent.py, and the
rows of the new entry through the schedule-perturbed builds."""
import numpy as np
import pytest

from tests import shake
from tests import shoebox_coherent_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    from audiblelight_amd import engine, synthesize as syn

    r = engine.Renderer()
    assert r.lib.path.endswith("libaudiblelight_hip.so")
    syn.set_renderer(r)
    yield r
    syn.set_renderer(None)


@pytest.mark.parametrize("P,J,M,F,ir_len,kind,pitch,sid0,cid0,gid,source,order,tables", cases.PARITY)
def test_parity_with_restatement(gpu, P, J, M, F, ir_len, kind, pitch, sid0, cid0, gid, source, order, tables):
    cases.run_parity(gpu, P, J, M, F, ir_len, kind, pitch, sid0, cid0, gid, source, order, tables)


def test_direct_evaluator_against_ctail(gpu):
    cases.run_direct_against_ctail(gpu)


def test_one_plane_wave_is_shared_by_the_rows(gpu):
    cases.run_one_wave_is_shared(gpu)


def test_no_tail_is_the_source_entry(gpu):
    cases.run_no_tail_is_the_source_entry(gpu)


def test_one_row_through_python_is_todays_tail(gpu):
    cases.run_one_row_is_todays_tail(gpu)


def test_row_identity(gpu):
    cases.run_row_identity(gpu)


def test_pair_cross_correlation(gpu):
    cases.run_pair_xcorr(gpu)


def test_state_pair_metrics_late_iacc(gpu):
    cases.run_state_pair_metrics(gpu)


def test_foa_channels_at_lag_zero(gpu):
    cases.run_foa_lag0(gpu)


def test_abi_refusals(gpu):
    cases.run_abi_refusals(gpu)


def test_python_errors(gpu, monkeypatch):
    cases.run_python_errors(gpu, monkeypatch)


def test_state_and_json_round_trip(gpu):
    cases.run_state(gpu)


def test_scene_end_to_end(gpu, monkeypatch, tmp_path):
    cases.run_end_to_end(gpu, monkeypatch, tmp_path)


def test_schedule_independence(gpu):
    """cases.run_shake_rows through the product library and the two schedule-perturbed builds: bit-identical rows."""
    from audiblelight_amd import _hip, engine

    ref = cases.run_shake_rows(gpu)
    for name, path in shake.existing_or_built(["s1", "s3w"]).items():
        got = cases.run_shake_rows(engine.Renderer(lib=_hip.Library(path)))
        for key in ref:
            assert np.array_equal(cases.bits(got[key]), cases.bits(ref[key])), f"{key}: the {name} build differs from the product library"
