"""The directional sources and the air absorption of the device shoebox IR generator (tests/shoebox_source_cases.py) on the
host-emulated kernels: parity of every sample with the float64 restatement within the derived bound (two rooms at four orders, omni,
cardioid and FOA receivers and walls in bands, a different pattern per source, three kinds of air, row lengths around the tile, a
capsule at 1 cm), the ties that need no restatement (the bits of the six old entries, order 0 in closed form, reciprocity against
the old receiver kernel, equal bands), the tail with a knot table per pair, the envelope law and ISO 9613-1, the refusals of the C ABI
and of the Python layer, the state with its JSON round trip, scenes end to end.  The gfx950 build runs the same scenarios in
tests/test_gpu_shoebox_source.py."""
import pytest

from audiblelight_amd import _hip, engine, synthesize as syn
from tests import hostemu
from tests import shoebox_source_cases as cases


@pytest.fixture(scope="module", autouse=True)
def emu():
    r = engine.Renderer(lib=_hip.Library(hostemu.build()), memory=hostemu.NumpyMemory())
    syn.set_renderer(r)
    yield r
    syn.set_renderer(None)


@pytest.mark.parametrize("room,order,kind,air", cases.PARITY)
def test_emu_parity_with_restatement(emu, room, order, kind, air):
    cases.run_parity(emu, room, order, kind, air)


@pytest.mark.parametrize("ir_len", cases.EDGE_LEN)
def test_emu_edge_row_lengths(emu, ir_len):
    cases.run_edge_length(emu, ir_len)


def test_emu_capsule_one_centimetre_from_its_source(emu):
    cases.run_close_capsule(emu)


def test_emu_omni_sources_without_air_are_the_old_entries(emu):
    cases.run_omni_ties(emu)


def test_emu_order_zero_in_closed_form(emu):
    cases.run_order_zero(emu)


def test_emu_reciprocity_against_the_receiver_kernel(emu):
    cases.run_reciprocity(emu)


def test_emu_equal_bands_are_the_broadband_entry(emu):
    cases.run_equal_bands(emu)


@pytest.mark.parametrize("M,F,ir_len,kind,order,pitch,sid0,cid0", cases.TAIL_PARITY)
def test_emu_tail_parity_with_restatement(emu, M, F, ir_len, kind, order, pitch, sid0, cid0):
    cases.run_tail_parity(emu, M, F, ir_len, kind, order, pitch, sid0, cid0)


def test_emu_tail_identity_and_workspace(emu):
    cases.run_tail_identity(emu)


def test_envelope_tables():
    cases.run_envelope_tables()


def test_envelope_law_against_image_source_restatement():
    cases.run_envelope_law_against_images()


def test_air_absorption_known_answers():
    cases.run_air_absorption()


def test_emu_abi_refusals(emu):
    cases.run_abi_refusals(emu)


def test_emu_python_errors(emu):
    cases.run_python_errors(emu)


def test_emu_state_and_json_round_trip(emu):
    cases.run_state(emu)


def test_emu_talker_facing_and_away(emu):
    cases.run_talker_irs(emu)
    cases.run_talker_scene(emu)


def test_emu_air_in_a_hard_room(emu):
    cases.run_air_scene(emu)
