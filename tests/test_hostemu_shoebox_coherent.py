"""The coherent diffuse tail of the device shoebox IR generator (tests/shoebox_coherent_cases.py) on the host-emulated kernels: parity
of every sample with the float64 restatement within the derived bound (random tables over the plane-wave and tap counts, the ends of
the delay range, the split around a tile edge, row lengths, pitches, ids, receiver kinds, source patterns with air, then the tables of
coherent_tail_tables), the ties that need no restatement (the direct evaluator against k_ism_ctail, one shared plane wave, the bits of
al_ism_shoebox_src and of today's tail, the identity of a row), what the numbers mean (the directions against sin(kd) / (kd), the
cross-correlation of a capsule pair against the tables' prediction), the refusals of the C ABI and of the Python layer, the state with
its JSON round trip, a scene end to end.  The gfx950 build runs the same scenarios in tests/test_gpu_shoebox_coherent.py."""
import pytest

from audiblelight_amd import _hip, engine, synthesize as syn
from tests import hostemu
from tests import shoebox_coherent_cases as cases


@pytest.fixture(scope="module", autouse=True)
def emu():
    r = engine.Renderer(lib=_hip.Library(hostemu.build()), memory=hostemu.NumpyMemory())
    syn.set_renderer(r)
    yield r
    syn.set_renderer(None)


def test_philox_restatement():
    cases.run_philox_restatement()


@pytest.mark.parametrize("P,J,M,F,ir_len,kind,pitch,sid0,cid0,gid,source,order,tables", cases.PARITY)
def test_emu_parity_with_restatement(emu, P, J, M, F, ir_len, kind, pitch, sid0, cid0, gid, source, order, tables):
    cases.run_parity(emu, P, J, M, F, ir_len, kind, pitch, sid0, cid0, gid, source, order, tables)


def test_emu_direct_evaluator_against_ctail(emu):
    cases.run_direct_against_ctail(emu)


def test_emu_one_plane_wave_is_shared_by_the_rows(emu):
    cases.run_one_wave_is_shared(emu)


def test_emu_no_tail_is_the_source_entry(emu):
    cases.run_no_tail_is_the_source_entry(emu)


def test_emu_one_row_through_python_is_todays_tail(emu):
    cases.run_one_row_is_todays_tail(emu)


def test_emu_row_identity(emu):
    cases.run_row_identity(emu)


def test_diffuse_directions():
    cases.run_directions()


def test_table_properties():
    cases.run_table_properties()


def test_emu_pair_cross_correlation(emu):
    cases.run_pair_xcorr(emu)


def test_emu_state_pair_metrics_late_iacc(emu):
    cases.run_state_pair_metrics(emu)


def test_emu_foa_channels_at_lag_zero(emu):
    cases.run_foa_lag0(emu)


def test_emu_abi_refusals(emu):
    cases.run_abi_refusals(emu)


def test_emu_python_errors(emu, monkeypatch):
    cases.run_python_errors(emu, monkeypatch)


def test_tail_dictionaries():
    cases.run_tail_dictionaries()


def test_emu_state_and_json_round_trip(emu):
    cases.run_state(emu)


def test_emu_scene_end_to_end(emu, monkeypatch, tmp_path):
    cases.run_end_to_end(emu, monkeypatch, tmp_path)
