"""Rigid-sphere receivers of the shoebox IR generator (tests/shoebox_sphere_cases.py) on the host-emulated kernels: the radial
filters against the exact series, parity of every sample with the float64 restatement within the derived bound (rooms, image orders,
1 to 64 Legendre orders with a group of one, half lengths 1 to 64, row lengths around the tap count and the tile, a source at 2
radius on a capsule's axis, source patterns and air), the ties to the omni and the first-order entry, the tail, the identity of a
row, the binaural listener through Scene.generate(), the state with its JSON round trip, the refusals of the C ABI and of the Python
layer.  The gfx950 build runs the same scenarios in tests/test_gpu_shoebox_sphere.py."""
import pytest

from audiblelight_amd import _hip, engine, synthesize as syn
from tests import hostemu
from tests import shoebox_sphere_cases as cases


@pytest.fixture(scope="module", autouse=True)
def emu():
    r = engine.Renderer(lib=_hip.Library(hostemu.build()), memory=hostemu.NumpyMemory())
    syn.set_renderer(r)
    yield r
    syn.set_renderer(None)


def test_sphere_filters():
    cases.run_filters()


def test_binaural_differences_of_the_filters_alone():
    cases.run_binaural_physics_restated()


@pytest.mark.parametrize("room,order,n_orders,half,pairs,ir_len,table", cases.PARITY)
def test_emu_parity_with_restatement(emu, room, order, n_orders, half, pairs, ir_len, table):
    cases.run_parity(emu, room, order, n_orders, half, pairs, ir_len, table)


@pytest.mark.parametrize("ir_len", cases.EDGE_LEN)
def test_emu_edge_lengths(emu, ir_len):
    cases.run_edge_length(emu, ir_len)


def test_emu_source_on_a_capsule_axis_at_two_radii(emu):
    cases.run_on_axis(emu)


def test_emu_source_patterns_and_air(emu):
    cases.run_source_and_air(emu)


def test_emu_one_order_is_the_omni_entry(emu):
    cases.run_omni_tie(emu)


def test_emu_two_orders_are_the_first_order_entry(emu):
    cases.run_first_order_tie(emu)


def test_emu_null_arguments(emu):
    cases.run_null_arguments(emu)


def test_emu_tail_past_the_row_is_the_entry_without_a_tail(emu):
    cases.run_no_tail(emu)


def test_emu_past_the_split_is_the_one_band_tail(emu):
    cases.run_past_the_split(emu)


@pytest.mark.parametrize("M,F,ir_len,table,pairs,order,pitch,sid0,cid0,per_pass", cases.TAIL_PARITY)
def test_emu_tail_parity_with_restatement(emu, M, F, ir_len, table, pairs, order, pitch, sid0, cid0, per_pass):
    cases.run_tail_parity(emu, M, F, ir_len, table, pairs, order, pitch, sid0, cid0, per_pass)


def test_emu_identity_and_workspace(emu):
    cases.run_identity(emu)


def test_emu_binaural_scene(emu, monkeypatch, tmp_path):
    cases.run_binaural_scene(emu, monkeypatch, tmp_path)


def test_emu_state_and_json_round_trip(emu):
    cases.run_state(emu)


def test_emu_round_trip_keeps_the_directions_bits(emu):
    cases.run_round_trip_directions(emu)


def test_emu_abi_refusals(emu):
    cases.run_abi_refusals(emu)


def test_emu_python_errors(emu):
    cases.run_python_errors(emu)
