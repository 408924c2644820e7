"""The directional receivers of the device shoebox IR generator (tests/shoebox_directional_cases.py) on the host-emulated kernels:
parity of every sample with the float64 oracle within the derived bound (anechoic gains, two rooms at four orders with FOA listeners
and one- and two-channel patterns, row lengths around the tile, a crowded tile, a receiver at 1 cm), bit-level determinism, the tail
with a knot table per channel, the weighted envelope law and its tables, the refusals of the C ABI and of the Python layer, the
state with its JSON round trip, scenes end to end.  The gfx950 build runs the same scenarios in
tests/test_gpu_shoebox_directional.py."""
import pytest

from audiblelight_amd import _hip, engine, synthesize as syn
from tests import hostemu
from tests import shoebox_cases as sc
from tests import shoebox_directional_cases as cases


@pytest.fixture(scope="module", autouse=True)
def emu():
    r = engine.Renderer(lib=_hip.Library(hostemu.build()), memory=hostemu.NumpyMemory())
    syn.set_renderer(r)
    yield r
    syn.set_renderer(None)


def test_emu_anechoic_gains(emu):
    cases.run_anechoic(emu)


@pytest.mark.parametrize("room,order,kind,n,fs", cases.PARITY)
def test_emu_parity_with_oracle(emu, room, order, kind, n, fs):
    cases.run_parity(emu, room, order, kind, n, fs)


@pytest.mark.parametrize("ir_len", sc.EDGE_LEN)
def test_emu_edge_row_lengths(emu, ir_len):
    cases.run_edge_length(emu, ir_len)


def test_emu_receiver_one_centimetre_from_the_source(emu):
    cases.run_close_receiver(emu)


def test_emu_crowded_tile(emu):
    cases.run_crowded_tile(emu)


def test_emu_determinism(emu):
    cases.run_determinism(emu)


@pytest.mark.parametrize("M,F,ir_len,kind,order,pitch,sid0,cid0", cases.TAIL_PARITY)
def test_emu_tail_parity_with_restatement(emu, M, F, ir_len, kind, order, pitch, sid0, cid0):
    cases.run_tail_parity(emu, M, F, ir_len, kind, order, pitch, sid0, cid0)


def test_emu_no_tail_is_the_plain_entry(emu):
    cases.run_no_tail_is_the_plain_entry(emu)


def test_emu_tail_identity(emu):
    cases.run_tail_identity(emu)


def test_envelope_tables():
    cases.run_envelope_tables()


def test_envelope_law_against_image_source_oracle():
    cases.run_envelope_law_against_images()


def test_emu_abi_refusals(emu):
    cases.run_abi_refusals(emu)


def test_emu_python_errors(emu):
    cases.run_python_errors(emu)


def test_emu_state_and_json_round_trip(emu):
    cases.run_state(emu)


def test_emu_scene_end_to_end(emu, monkeypatch, tmp_path):
    cases.run_end_to_end(emu, monkeypatch, tmp_path)


def test_emu_direction_end_to_end(emu):
    cases.run_direction_end_to_end(emu)
