"""tests/shoebox_directional_cases.py on the real MI355X (gfx950 build): the scenarios of tests/test_hostemu_shoebox_directional.py."""
import pytest

from tests import shoebox_cases as sc
from tests import shoebox_directional_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    from audiblelight_amd import engine, synthesize as syn

    r = engine.Renderer()
    assert r.lib.path.endswith("libaudiblelight_hip.so")
    syn.set_renderer(r)
    yield r
    syn.set_renderer(None)


def test_anechoic_gains(gpu):
    cases.run_anechoic(gpu)


@pytest.mark.parametrize("room,order,kind,n,fs", cases.PARITY)
def test_parity_with_oracle(gpu, room, order, kind, n, fs):
    cases.run_parity(gpu, room, order, kind, n, fs)


@pytest.mark.parametrize("ir_len", sc.EDGE_LEN)
def test_edge_row_lengths(gpu, ir_len):
    cases.run_edge_length(gpu, ir_len)


def test_receiver_one_centimetre_from_the_source(gpu):
    cases.run_close_receiver(gpu)


def test_crowded_tile(gpu):
    cases.run_crowded_tile(gpu)


def test_determinism(gpu):
    cases.run_determinism(gpu)


@pytest.mark.parametrize("M,F,ir_len,kind,order,pitch,sid0,cid0", cases.TAIL_PARITY)
def test_tail_parity_with_restatement(gpu, M, F, ir_len, kind, order, pitch, sid0, cid0):
    cases.run_tail_parity(gpu, M, F, ir_len, kind, order, pitch, sid0, cid0)


def test_no_tail_is_the_plain_entry(gpu):
    cases.run_no_tail_is_the_plain_entry(gpu)


def test_tail_identity(gpu):
    cases.run_tail_identity(gpu)


def test_abi_refusals(gpu):
    cases.run_abi_refusals(gpu)


def test_python_errors(gpu):
    cases.run_python_errors(gpu)


def test_state_and_json_round_trip(gpu):
    cases.run_state(gpu)


def test_scene_end_to_end(gpu, monkeypatch, tmp_path):
    cases.run_end_to_end(gpu, monkeypatch, tmp_path)


def test_direction_end_to_end(gpu):
    cases.run_direction_end_to_end(gpu)
