"""The octave-band IR metrics (tests/ir_band_metrics_cases.py) on the host-emulated kernels: al_ir_band_split against the float64
restatement within the derived bound on every sample, at every row length around a lane's run, a tap chunk and the tile, `half`
below, at and past a tap chunk and far past the row, every band count, the layouts (pitch, stride_c, an unaligned base, out_pitch,
sentinels around and inside `out`), the exact ties (the impulse, a doubled table, the partition of unity); al_ir_band_metrics against
al_ir_metrics over the split's output bit for bit at every pass size; a NaN; the two-rate rows; the refusals of the C ABI and of the
Python layer; the Python layer, the states and the band formulas.  The gfx950 build runs the same scenarios in
tests/test_gpu_ir_band_metrics.py."""
import pytest

from audiblelight_amd import _hip, engine, synthesize as syn
from tests import hostemu
from tests import ir_band_metrics_cases as cases


@pytest.fixture(scope="module", autouse=True)
def emu():
    r = engine.Renderer(lib=_hip.Library(hostemu.build()), memory=hostemu.NumpyMemory())
    syn.set_renderer(r)
    yield r
    syn.set_renderer(None)
    for name, frac in sorted(cases.WORST.items()):
        print(f"\n[host emulation] ir band metrics, {name}: worst error / bound {frac:.3g}")


@pytest.mark.parametrize("ir_len,half,n_bands,pair", cases.SPLIT_SHAPES)
def test_emu_split_against_the_restatement(emu, ir_len, half, n_bands, pair):
    cases.run_split_shape(emu, ir_len, half, n_bands, pair)


def test_emu_split_layouts(emu):
    cases.run_split_layouts(emu)


def test_emu_exact_ties(emu):
    cases.run_exact(emu)


def test_emu_composition(emu):
    cases.run_composition(emu)


def test_emu_non_finite_sample(emu):
    cases.run_non_finite(emu)


def test_emu_two_rate_rows(emu):
    cases.run_meaning(emu)


def test_emu_abi_refusals(emu):
    cases.run_abi_refusals(emu)


def test_emu_python_errors(emu):
    cases.run_python_errors(emu)


def test_emu_python_layer(emu):
    cases.run_python_layer(emu)


def test_emu_states(emu, monkeypatch):
    cases.run_state(emu, cases.FIXTURE, monkeypatch)


def test_band_formulas():
    cases.run_formulas()
