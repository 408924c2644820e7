"""tests/shoebox_bands_cases.py on the real MI355X (gfx950 build): the scenarios of tests/test_hostemu_shoebox_bands.py, plus the
schedule independence of the combine and tail kernels (one-wave workgroups, whose LDS hand-overs the perturbed builds surround with
sleeps; the workspace hand-over from one launch and pass to the next is ordered by the stream): the product library and the `s1`
and `s3w` builds of tests/shake.py give bit-identical rows."""
import numpy as np
import pytest

from tests import shake
from tests import shoebox_bands_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    from audiblelight_amd import engine, synthesize as syn

    r = engine.Renderer()
    assert r.lib.path.endswith("libaudiblelight_hip.so")
    syn.set_renderer(r)
    yield r
    syn.set_renderer(None)


@pytest.mark.parametrize("room,order,n_bands,half,pairs,fs,ir_len", cases.PARITY)
def test_parity_with_restatement(gpu, room, order, n_bands, half, pairs, fs, ir_len):
    cases.run_parity(gpu, room, order, n_bands, half, pairs, fs, ir_len)


@pytest.mark.parametrize("ir_len,half", cases.EDGES)
def test_edge_lengths(gpu, ir_len, half):
    cases.run_edge_length(gpu, ir_len, half)


def test_close_capsule(gpu):
    cases.run_close_capsule(gpu)


def test_crowded_tile(gpu):
    cases.run_crowded_tile(gpu)


def test_equal_columns_are_the_broadband_oracle(gpu):
    cases.run_equal_columns(gpu)


def test_one_band_is_the_broadband_entry(gpu):
    cases.run_one_band_is_the_broadband_entry(gpu)


def test_one_reflecting_wall(gpu):
    cases.run_one_wall(gpu)


def test_identity_and_workspace(gpu):
    cases.run_identity(gpu)


@pytest.mark.parametrize("M,F,ir_len,n_bands,half,pairs,order,pitch,sid0,cid0,per_pass", cases.TAIL_PARITY)
def test_tail_parity_with_restatement(gpu, M, F, ir_len, n_bands, half, pairs, order, pitch, sid0, cid0, per_pass):
    cases.run_tail_parity(gpu, M, F, ir_len, n_bands, half, pairs, order, pitch, sid0, cid0, per_pass)


def test_tail_knot_tables(gpu):
    cases.run_tail_tables(gpu)


def test_tail_equal_bands_are_the_broadband_tail(gpu):
    cases.run_tail_equal_bands(gpu)


def test_tail_past_the_row_is_the_entry_without_a_tail(gpu):
    cases.run_tail_no_tail_bits(gpu)


def test_tail_identity_and_workspace(gpu):
    cases.run_tail_identity(gpu)


def test_tail_abi_refusals(gpu):
    cases.run_tail_abi_refusals(gpu)


def test_abi_refusals(gpu):
    cases.run_abi_refusals(gpu)


def test_python_errors(gpu):
    cases.run_python_errors(gpu)


def test_state_and_json_round_trip(gpu):
    cases.run_state(gpu)


def test_scene_end_to_end(gpu, monkeypatch, tmp_path):
    cases.run_end_to_end(gpu, monkeypatch, tmp_path)


def test_schedule_independence(gpu):
    """cases.run_shake_rows (the entry without a tail and with one, each within its bound first) through the product library and
    the two schedule-perturbed builds: bit-identical rows."""
    from audiblelight_amd import _hip, engine

    ref = cases.run_shake_rows(gpu)
    for name, path in shake.existing_or_built(["s1", "s3w"]).items():
        got = cases.run_shake_rows(engine.Renderer(lib=_hip.Library(path)))
        for key in ref:
            assert np.array_equal(cases.bits(got[key][0]), cases.bits(ref[key][0])), f"{key}: the {name} build differs from the product library"
