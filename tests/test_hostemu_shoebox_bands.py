"""Shoebox IRs with frequency-dependent walls (tests/shoebox_bands_cases.py) on the host-emulated kernels: the band filters'
properties, parity of every sample with the float64 restatement within the derived bound (rooms, orders, 1 to 8 bands with a band
group of one, filter half lengths from 1 to 300, row lengths around the tap count and the tile, a capsule 1 cm from its source), the
ties to the broadband oracle and entry, the identity of a row (alone, among many, at another pitch, with a workspace of one pair per
pass), materials, the refusals of the C ABI and of the Python layer, the state with its JSON round trip, a scene end to end.  The
gfx950 build runs the same scenarios in tests/test_gpu_shoebox_bands.py."""
import pytest

from audiblelight_amd import _hip, engine, synthesize as syn
from tests import hostemu
from tests import shoebox_bands_cases as cases


@pytest.fixture(scope="module", autouse=True)
def emu():
    r = engine.Renderer(lib=_hip.Library(hostemu.build()), memory=hostemu.NumpyMemory())
    syn.set_renderer(r)
    yield r
    syn.set_renderer(None)


def test_band_filters():
    cases.run_band_filters()


def test_materials():
    cases.run_materials()


@pytest.mark.parametrize("room,order,n_bands,half,pairs,fs,ir_len", cases.PARITY)
def test_emu_parity_with_restatement(emu, room, order, n_bands, half, pairs, fs, ir_len):
    cases.run_parity(emu, room, order, n_bands, half, pairs, fs, ir_len)


@pytest.mark.parametrize("ir_len,half", cases.EDGES)
def test_emu_edge_lengths(emu, ir_len, half):
    cases.run_edge_length(emu, ir_len, half)


def test_emu_close_capsule(emu):
    cases.run_close_capsule(emu)


def test_emu_crowded_tile(emu):
    cases.run_crowded_tile(emu)


def test_emu_equal_columns_are_the_broadband_oracle(emu):
    cases.run_equal_columns(emu)


def test_emu_one_band_is_the_broadband_entry(emu):
    cases.run_one_band_is_the_broadband_entry(emu)


def test_emu_one_reflecting_wall(emu):
    cases.run_one_wall(emu)


def test_emu_identity_and_workspace(emu):
    cases.run_identity(emu)


@pytest.mark.parametrize("M,F,ir_len,n_bands,half,pairs,order,pitch,sid0,cid0,per_pass", cases.TAIL_PARITY)
def test_emu_tail_parity_with_restatement(emu, M, F, ir_len, n_bands, half, pairs, order, pitch, sid0, cid0, per_pass):
    cases.run_tail_parity(emu, M, F, ir_len, n_bands, half, pairs, order, pitch, sid0, cid0, per_pass)


def test_emu_tail_knot_tables(emu):
    cases.run_tail_tables(emu)


def test_emu_tail_equal_bands_are_the_broadband_tail(emu):
    cases.run_tail_equal_bands(emu)


def test_emu_tail_past_the_row_is_the_entry_without_a_tail(emu):
    cases.run_tail_no_tail_bits(emu)


def test_emu_tail_identity_and_workspace(emu):
    cases.run_tail_identity(emu)


def test_emu_tail_abi_refusals(emu):
    cases.run_tail_abi_refusals(emu)


def test_emu_abi_refusals(emu):
    cases.run_abi_refusals(emu)


def test_emu_python_errors(emu):
    cases.run_python_errors(emu)


def test_emu_state_and_json_round_trip(emu):
    cases.run_state(emu)


def test_emu_scene_end_to_end(emu, monkeypatch, tmp_path):
    cases.run_end_to_end(emu, monkeypatch, tmp_path)
