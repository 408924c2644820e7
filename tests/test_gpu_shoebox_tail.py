"""tests/shoebox_tail_cases.py on the real MI355X (gfx950 build): the scenarios of tests/test_hostemu_shoebox_tail.py, plus the
pipelined batch driver staging a device-resident IR tensor with a tail (no copy, no H2D bytes counted)."""
import pytest

from tests import shoebox_tail_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    from audiblelight_amd import engine, synthesize as syn

    r = engine.Renderer()
    assert r.lib.path.endswith("libaudiblelight_hip.so")
    syn.set_renderer(r)
    yield r
    syn.set_renderer(None)


@pytest.mark.parametrize("M,F,ir_len,pairs,order,pitch,sid0,cid0", cases.PARITY)
def test_parity_with_restatement(gpu, M, F, ir_len, pairs, order, pitch, sid0, cid0):
    cases.run_parity(gpu, M, F, ir_len, pairs, order, pitch, sid0, cid0)


def test_no_tail_is_todays_bits(gpu):
    cases.run_no_tail_is_todays_bits(gpu)


def test_row_identity(gpu):
    cases.run_row_identity(gpu)


def test_envelope_tables(gpu):
    cases.run_envelope_tables(gpu)


def test_abi_refusals(gpu):
    cases.run_abi_refusals(gpu)


def test_python_errors(gpu):
    cases.run_python_errors(gpu)


def test_state_and_json_round_trip(gpu):
    cases.run_state(gpu)


def test_scene_end_to_end(gpu, monkeypatch, tmp_path):
    cases.run_end_to_end(gpu, monkeypatch, tmp_path)


def test_batch_driver_takes_the_device_tensor(gpu, monkeypatch):
    cases.run_batch_driver(gpu, monkeypatch)
