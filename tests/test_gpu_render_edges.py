"""tests/render_edges.py on the real MI355X (gfx950 build): every block size 2^10..2^14, every layout the build dispatches to
(plain, split, quad tiles at 16384, NARROW_FFT, SYNTH_RUN / IR_RUN runs), the device's own sincospi and the full-size mixdown
lengths.  The host emulation runs the same scenarios at small blocks in tests/test_hostemu_render_edges.py."""
import pytest

from tests import render_edges as rd

pytestmark = pytest.mark.gpu

BLOCKS = [10, 11, 12, 13, 14]
LAYOUT_CASES = [(lb, layout) for lb in BLOCKS for layout in rd.LAYOUTS if rd.layout_ok(layout, lb)]


@pytest.fixture(scope="module")
def gpu():
    from audiblelight_amd import engine

    r = engine.Renderer()
    assert r.lib.path.endswith("libaudiblelight_hip.so")
    return r


@pytest.fixture(scope="module", autouse=True)
def margins():
    rd.MARGINS.clear()
    yield
    for family, (seen, bound) in sorted(rd.MARGINS.items()):
        print(f"\n[gfx950] {family}: worst {seen:.3g}, bound {bound:.3g}")


@pytest.mark.parametrize("log2_block", BLOCKS)
def test_twiddles(gpu, log2_block):
    rd.run_twiddles(gpu, log2_block)


@pytest.mark.parametrize("ir_len", [1, 1023, 1024, 1025, 21 * 1024, 21 * 1024 + 1, 24 * 1024 + 1, 25 * 1024 + 3])
@pytest.mark.parametrize("C", [1, 63, 64, 65, 129])
def test_emitter_gains(gpu, ir_len, C):
    rd.run_emitter_gains(gpu, 10, ir_len, C)


@pytest.mark.parametrize("log2_block", [12, 14])
def test_emitter_gains_big_blocks(gpu, log2_block):
    B = 1 << log2_block
    rd.run_emitter_gains(gpu, log2_block, 21 * B + 1, 65)


@pytest.mark.parametrize("edge", ["all_zero", "some_zero", "denormal", "nan"])
def test_emitter_gain_edges(gpu, edge):
    rd.run_emitter_gains(gpu, 10, 1500, 65, edge=edge)


def test_emitter_gains_no_norm(gpu):
    rd.run_emitter_gains_flags(gpu, 10, 1025, 3)


@pytest.mark.parametrize("C,split,edge", [(5, 2, None), (129, 64, None), (65, 1, "some_zero"), (4, 2, "all_zero"),
                                          (3, 1, "denormal")])
def test_emitter_gains_sharded(gpu, C, split, edge):
    rd.run_emitter_gains_sharded(gpu, 10, 2049, C, split, edge)


@pytest.mark.parametrize("log2_block", BLOCKS)
def test_spectra(gpu, log2_block):
    rd.run_spectra(gpu, log2_block)


@pytest.mark.parametrize("log2_block,layout", LAYOUT_CASES)
def test_delta_irs(gpu, log2_block, layout):
    B = 1 << log2_block
    P = 3
    rd.run_delta_render(gpu, log2_block, P, [0, B - 1, B, B + 1, 2 * B - 1, 2 * B, P * B - 1],
                        [1, 2, B - 1, B, B + 1, 3 * B - 1, 3 * B + 1], layout=layout)


@pytest.mark.parametrize("log2_block,layout", LAYOUT_CASES)
def test_delta_clip(gpu, log2_block, layout):
    rd.run_delta_clip(gpu, log2_block, 3, layout=layout)


@pytest.mark.parametrize("P", [1, 2, 21, 22, 24, 25, 26])
@pytest.mark.parametrize("log2_block", [10, 12, 14])
def test_flat_irs(gpu, log2_block, P):
    rd.run_flat_render(gpu, log2_block, P, seed=P, layout="quad" if log2_block == 14 else "plain")


@pytest.mark.parametrize("log2_block,layout", LAYOUT_CASES)
def test_flat_irs_layouts(gpu, log2_block, layout):
    rd.run_flat_render(gpu, log2_block, 3, layout=layout, seed=1)


@pytest.mark.parametrize("n_j", [6, 7])
@pytest.mark.parametrize("log2_block", [10, 13])
def test_moving_nj(gpu, log2_block, n_j):
    rd.run_flat_render(gpu, log2_block, 4, kinds=("moving", "static"), n_j=n_j, seed=n_j)


@pytest.mark.parametrize("reach", ["last", "past"])
@pytest.mark.parametrize("log2_block", [10, 12])
def test_emitter_parts_boundary(gpu, log2_block, reach):
    rd.run_emitter_parts_boundary(gpu, log2_block, reach)


@pytest.mark.parametrize("C,n_samples", [(1, 1), (1, 63 * 1024 - 5), (64, 1000), (65, 1024), (1, 4097 * 1024 - 9)])
def test_level_law(gpu, C, n_samples):
    rd.run_level_law(gpu, 10, C, n_samples, [0.5, 30.0, 17.25], [-65.0, -10.0, -120.0])


@pytest.mark.parametrize("silent", ["clip", "ir"])
def test_level_law_silent(gpu, silent):
    rd.run_level_law(gpu, 10, 2, 3000, [10.0, 5.0], [-50.0, -65.0], silent=silent)


def test_level_law_from_stats(gpu):
    rd.run_level_law(gpu, 10, 3, 5000, [10.0, 20.0], [-50.0, -65.0], total_extra=5)


@pytest.mark.parametrize("n_samples", [1, 3, 4, 4095, 4096, 4097, 8191, 2_880_000, 2_880_001, 2_880_003])
def test_mixdown(gpu, n_samples):
    rd.run_mixdown_slots(gpu, n_samples, seed=n_samples % 7)


@pytest.mark.parametrize("accumulate,ambience,rows_cut", [(True, False, False), (False, True, False), (False, True, True),
                                                          (False, False, True)])
def test_mixdown_variants(gpu, accumulate, ambience, rows_cut):
    rd.run_mixdown_slots(gpu, 12289, C=3, accumulate=accumulate, ambience=ambience, rows_cut=rows_cut)


def test_mixdown_ambience_only(gpu):
    case = rd.MixCase(2, 8193)
    rd.run_mixdown(gpu, case, rd.np.zeros(4, rd.np.float32), [1.0], ambience=True, family="mixdown ambience only")


@pytest.mark.parametrize("n_samples", [20000, 2_880_001])
def test_mixdown_planned(gpu, n_samples):
    rd.run_mixdown_planned(gpu, n_samples, C=2)


def test_mixdown_refusals(gpu):
    rd.run_mixdown_refusals(gpu)
