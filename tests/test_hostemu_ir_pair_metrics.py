"""The channel-pair IR metrics (tests/ir_pair_metrics_cases.py) on the host-emulated kernels: al_ir_pair_metrics against the float64
restatement within the derived bound, at every row length around a tile and every max_lag around a block of 64 lags and past the
row, both window lengths, T0 on and beside a tile boundary, late windows of one sample and none; the layouts (pitch, stride_c, an
unaligned base, sentinels around and inside the tables), a pair and a source alone against the same among many, with and without
curves; the exact ties (a row against itself, an inverted delayed copy); coherent early and independent late by construction; NaN,
silence, pairs outside the capsules, an absurd rows table; the refusals of the C ABI and of the Python layer; the Python layer, the
states and the band composition.  The gfx950 build runs the same scenarios in tests/test_gpu_ir_pair_metrics.py."""
import pytest

from audiblelight_amd import _hip, engine, synthesize as syn
from tests import hostemu
from tests import ir_pair_metrics_cases as cases


@pytest.fixture(scope="module", autouse=True)
def emu():
    r = engine.Renderer(lib=_hip.Library(hostemu.build()), memory=hostemu.NumpyMemory())
    syn.set_renderer(r)
    yield r
    syn.set_renderer(None)
    for name, frac in sorted(cases.WORST.items()):
        print(f"\n[host emulation] ir pair metrics, {name}: worst error / bound {frac:.3g}")


@pytest.mark.parametrize("ir_len", cases.LENGTHS)
def test_emu_against_the_restatement(emu, ir_len):
    cases.run_length(emu, ir_len)


def test_emu_pair_and_source_counts(emu):
    cases.run_sizes(emu)


def test_emu_window_edges(emu):
    cases.run_windows(emu)


def test_emu_layouts_and_identity(emu):
    cases.run_layouts(emu)


def test_emu_exact_ties(emu):
    cases.run_exact(emu)


def test_emu_coherent_early_independent_late(emu):
    cases.run_meaning(emu)


def test_emu_states(emu):
    cases.run_states(emu)


def test_emu_abi_refusals(emu):
    cases.run_abi_refusals(emu)


def test_emu_python_errors(emu, monkeypatch):
    cases.run_python_errors(emu, monkeypatch)


def test_emu_python_layer(emu):
    cases.run_python_layer(emu)


def test_emu_shoebox_and_static_states(emu, monkeypatch):
    cases.run_state(emu, monkeypatch)


def test_emu_band_composition(emu):
    cases.run_band_composition(emu)
