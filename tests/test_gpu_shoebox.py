"""tests/shoebox_cases.py on the real MI355X (gfx950 build): the scenarios of tests/test_hostemu_shoebox.py, plus the pipelined
batch driver staging a device-resident IR tensor (no copy, no H2D bytes counted)."""
import pytest

from tests import shoebox_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    from audiblelight_amd import engine, synthesize as syn

    r = engine.Renderer()
    assert r.lib.path.endswith("libaudiblelight_hip.so")
    syn.set_renderer(r)
    yield r
    syn.set_renderer(None)


def test_anechoic_room_is_one_image(gpu):
    cases.run_anechoic(gpu)


@pytest.mark.parametrize("room,order,pairs,fs", cases.PARITY)
def test_parity_with_oracle(gpu, room, order, pairs, fs):
    cases.run_parity(gpu, room, order, pairs, fs)


@pytest.mark.parametrize("ir_len", cases.EDGE_LEN)
def test_edge_lengths(gpu, ir_len):
    cases.run_edge_length(gpu, ir_len)


def test_capsule_one_centimetre_from_source(gpu):
    cases.run_close_capsule(gpu)


def test_more_images_than_a_chunk_or_a_list(gpu):
    cases.run_crowded_tile(gpu)


def test_determinism(gpu):
    cases.run_determinism(gpu)


def test_abi_refusals(gpu):
    cases.run_abi_refusals(gpu)


def test_python_errors(gpu):
    cases.run_python_errors(gpu)


def test_rt60_round_trip():
    cases.run_rt60_round_trip()


def test_state_and_lazy_tensor(gpu):
    cases.run_state_and_tensor(gpu)


def test_scene_end_to_end(gpu, monkeypatch, tmp_path):
    cases.run_end_to_end(gpu, monkeypatch, tmp_path)


def test_batch_driver_takes_the_device_tensor(gpu, monkeypatch):
    cases.run_batch_driver(gpu, monkeypatch)
