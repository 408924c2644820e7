"""The diffuse tail of the device shoebox IR generator (tests/shoebox_tail_cases.py) on the host-emulated kernels: parity of every
sample with the float64 restatement within the derived bound (mixing samples and fades around the tile, the split on either side of
a tile edge, fades cut by the row end, rows just past the split, wide pitches, a row of two k_ism_tail workgroups), the bits of
al_ism_shoebox when nothing is mixed, the identity of a row, envelope tables, the envelope law against the image-source oracle, the
refusals of the C ABI and of the Python layer, the state with its JSON round trip, a scene end to end without the tensor touching
the host.  The gfx950 build runs the same scenarios in tests/test_gpu_shoebox_tail.py."""
import pytest

from audiblelight_amd import _hip, engine, synthesize as syn
from tests import hostemu
from tests import shoebox_tail_cases as cases


@pytest.fixture(scope="module", autouse=True)
def emu():
    r = engine.Renderer(lib=_hip.Library(hostemu.build()), memory=hostemu.NumpyMemory())
    syn.set_renderer(r)
    yield r
    syn.set_renderer(None)


@pytest.mark.parametrize("M,F,ir_len,pairs,order,pitch,sid0,cid0", cases.PARITY)
def test_emu_parity_with_restatement(emu, M, F, ir_len, pairs, order, pitch, sid0, cid0):
    cases.run_parity(emu, M, F, ir_len, pairs, order, pitch, sid0, cid0)


def test_emu_no_tail_is_todays_bits(emu):
    cases.run_no_tail_is_todays_bits(emu)


def test_emu_row_identity(emu):
    cases.run_row_identity(emu)


def test_emu_envelope_tables(emu):
    cases.run_envelope_tables(emu)


def test_envelope_law_properties():
    cases.run_envelope_law_properties()


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
