"""tests/render_edges.py on the host-emulated kernels: small blocks (B = 1024, 2048, one quad-tile case at 16384), every scenario
family against its float64 restatement, guard bands around every event block.  The gfx950 build runs the same scenarios at every
block size and layout in tests/test_gpu_render_edges.py."""
import pytest

from audiblelight_amd import _hip, engine
from tests import hostemu, render_edges as rd


@pytest.fixture(scope="module")
def emu():
    return engine.Renderer(lib=_hip.Library(hostemu.build()), memory=hostemu.NumpyMemory())


@pytest.fixture(scope="module", autouse=True)
def margins():
    rd.MARGINS.clear()
    yield
    for family, (seen, bound) in sorted(rd.MARGINS.items()):
        print(f"\n[host emulation] {family}: worst {seen:.3g}, bound {bound:.3g}")


@pytest.mark.parametrize("log2_block", [10, 11])
def test_emu_twiddles(emu, log2_block):
    rd.run_twiddles(emu, log2_block)


@pytest.mark.parametrize("ir_len,C", [(1, 1), (1023, 63), (1024, 64), (1025, 65), (21 * 1024 + 1, 3), (25 * 1024 + 3, 2),
                                      (2049, 129)])
def test_emu_emitter_gains(emu, ir_len, C):
    rd.run_emitter_gains(emu, 10, ir_len, C)


@pytest.mark.parametrize("edge", ["all_zero", "some_zero", "denormal", "nan"])
def test_emu_emitter_gain_edges(emu, edge):
    rd.run_emitter_gains(emu, 10, 1500, 65, edge=edge)


def test_emu_emitter_gains_no_norm(emu):
    rd.run_emitter_gains_flags(emu, 10, 1025, 3)


@pytest.mark.parametrize("C,split,edge", [(5, 2, None), (129, 64, None), (65, 1, "some_zero"), (4, 2, "all_zero"),
                                          (3, 1, "denormal")])
def test_emu_emitter_gains_sharded(emu, C, split, edge):
    rd.run_emitter_gains_sharded(emu, 10, 2049, C, split, edge)


@pytest.mark.parametrize("log2_block", [10, 11])
def test_emu_spectra(emu, log2_block):
    rd.run_spectra(emu, log2_block)


@pytest.mark.parametrize("log2_block", [10, 11])
def test_emu_delta_irs(emu, log2_block):
    B = 1 << log2_block
    P = 3
    rd.run_delta_render(emu, log2_block, P, [0, B - 1, B, B + 1, 2 * B - 1, 2 * B, P * B - 1],
                        [1, 2, B - 1, B, B + 1, 3 * B - 1, 3 * B + 1])


@pytest.mark.parametrize("log2_block,layout", [(10, "plain"), (11, "split"), (11, "runs")])
def test_emu_delta_clip(emu, log2_block, layout):
    rd.run_delta_clip(emu, log2_block, 3, layout=layout)


@pytest.mark.parametrize("P", [1, 2, 21, 22, 24, 25, 26])
def test_emu_flat_irs(emu, P):
    rd.run_flat_render(emu, 10, P, seed=P)


@pytest.mark.parametrize("layout", ["split", "runs"])
def test_emu_flat_irs_layouts(emu, layout):
    rd.run_flat_render(emu, 11, 3, layout=layout, seed=1)


@pytest.mark.parametrize("n_j", [6, 7])
def test_emu_moving_nj(emu, n_j):
    rd.run_flat_render(emu, 10, 4, kinds=("moving", "static"), n_j=n_j, seed=n_j)


def test_emu_quad_tiles(emu):
    rd.run_flat_render(emu, 14, 2, layout="quad", C=1, kinds=("static", "moving"), seed=3)


@pytest.mark.parametrize("reach", ["last", "past"])
def test_emu_emitter_parts_boundary(emu, reach):
    rd.run_emitter_parts_boundary(emu, 10, reach)


@pytest.mark.parametrize("C,n_samples", [(1, 1), (1, 63 * 1024 - 5), (64, 1000), (65, 1024), (1, 4097 * 1024 - 9)])
def test_emu_level_law(emu, C, n_samples):
    rd.run_level_law(emu, 10, C, n_samples, [0.5, 30.0, 17.25], [-65.0, -10.0, -120.0])


@pytest.mark.parametrize("silent", ["clip", "ir"])
def test_emu_level_law_silent(emu, silent):
    rd.run_level_law(emu, 10, 2, 3000, [10.0, 5.0], [-50.0, -65.0], silent=silent)


def test_emu_level_law_from_stats(emu):
    rd.run_level_law(emu, 10, 3, 5000, [10.0, 20.0], [-50.0, -65.0], total_extra=5)


@pytest.mark.parametrize("n_samples", [1, 3, 4, 4095, 4096, 4097, 8191, 40963])
def test_emu_mixdown(emu, n_samples):
    rd.run_mixdown_slots(emu, n_samples, seed=n_samples % 7)


@pytest.mark.parametrize("accumulate,ambience,rows_cut", [(True, False, False), (False, True, False), (False, True, True),
                                                          (False, False, True)])
def test_emu_mixdown_variants(emu, accumulate, ambience, rows_cut):
    rd.run_mixdown_slots(emu, 12289, C=3, accumulate=accumulate, ambience=ambience, rows_cut=rows_cut)


def test_emu_mixdown_ambience_only(emu):
    case = rd.MixCase(2, 8193)
    rd.run_mixdown(emu, case, rd.np.zeros(4, rd.np.float32), [1.0], ambience=True, family="mixdown ambience only")


@pytest.mark.parametrize("n_samples", [20000, 2_880_001])
def test_emu_mixdown_planned(emu, n_samples):
    rd.run_mixdown_planned(emu, n_samples, C=1)


def test_emu_mixdown_refusals(emu):
    rd.run_mixdown_refusals(emu)
