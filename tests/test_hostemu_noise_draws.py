"""tests/noise_draw_cases.py on the host-emulated kernels: the device-drawn ambience noise pinned element for element (the
chain A, B, C of that module's docstring).  tests/test_gpu_noise_draws.py runs the same scenarios on the gfx950 build and adds
the sizes emulated workgroups are too slow for."""
import numpy as np
import pytest

from audiblelight_amd import _hip, engine, synthesize as syn
from tests import hostemu, kernel_edges as ke, noise_draw_cases as nd


@pytest.fixture(scope="module")
def emu():
    r = engine.Renderer(lib=_hip.Library(hostemu.build()), memory=hostemu.NumpyMemory())
    syn.set_renderer(r)
    yield r
    syn.set_renderer(None)


@pytest.fixture(scope="module", autouse=True)
def margins():
    ke.MARGINS.clear()
    yield
    for family, (seen, bound) in sorted(ke.MARGINS.items()):
        print(f"\n[hostemu] {family}: worst {seen:.3g}, bound {bound:.3g}")


BIG = dict(n=nd.FILL_CAP + 5, seed=0xFEDCBA9876543210, tag=2, scale=-1.25)


@pytest.fixture(scope="module")
def big_fill(emu):
    """One fill that takes a second trip of the grid stride, shared (read-only) by the tests that look at it."""
    got = nd.fill(emu, BIG["n"], BIG["seed"], BIG["tag"], BIG["scale"]).get()
    got.setflags(write=False)
    return got


# ----------------------------------------------------------------------------- A
@pytest.mark.parametrize("n", nd.FILL_SMALL_N)
def test_normal_fill_small_lengths(emu, n):
    nd.run_fill(emu, n, nd.SEEDS[n % 3], nd.TAGS[n % 4])


@pytest.mark.parametrize("seed", nd.SEEDS)
@pytest.mark.parametrize("tag", nd.TAGS)
def test_normal_fill_tags_and_seeds(emu, seed, tag):
    nd.run_fill(emu, 1027, seed, tag)


@pytest.mark.parametrize("n", [5, 1026, 2049])
def test_normal_fill_scales(emu, n):
    for scale in (1.0, -0.37, nd.white_scale(n)):
        nd.run_fill(emu, n, 0xABCDEF0123, 2, scale)


def test_normal_fill_streams_are_independent(emu):
    nd.run_fill_independence(emu)


def test_normal_fill_second_grid_stride_trip(emu, big_fill):
    cap, n = nd.FILL_CAP, BIG["n"]
    mid = int(np.random.default_rng(7).integers(4096, cap - 2 * 4096))
    for lo, hi in ((0, 4096), (cap - 4096, n), (mid, mid + 4096)):
        nd.check_draws(big_fill[lo:hi], nd.restated_normals(BIG["seed"], BIG["tag"], lo, hi), BIG["scale"],
                       "normal_fill (err / tolerance)", ("second trip", lo, hi))
    assert int(np.sum(big_fill[cap:cap + 4096] == big_fill[:n - cap])) == 0          # the second trip did not start over


def test_normal_fill_is_independent_of_the_launch_geometry(emu, big_fill):
    # a fill above the grid cap against fills below it (a k above the cap as well: tests/test_gpu_noise_draws.py; one
    # emulated fill of that size takes several seconds)
    for k in (37, 1025, 4 * 256 * 40 + 2):
        ke.assert_bits_equal(nd.fill(emu, k, BIG["seed"], BIG["tag"], BIG["scale"]).get(), big_fill[:k], ("prefix", k))


def test_normal_fill_refusals(emu):
    nd.run_fill_refusals(emu)


# ----------------------------------------------------------------------------- B
@pytest.mark.parametrize("n", nd.SEEDED_N)
@pytest.mark.parametrize("shaped", [True, False], ids=["pink", "nullptr"])
def test_seeded_irfft_is_the_explicit_irfft_of_the_device_draws(emu, n, shaped):
    rows = 1 + n % 3
    nd.run_seeded(emu, rows, n, nd.SEEDS[n % 3], shaped)


@pytest.mark.parametrize("rows,n", [(3, 513), (5, 514)])
def test_seeded_irfft_rows(emu, rows, n):
    assert (n // 2 + 1) % 4 and (n // 2 + 1) % 256
    nd.run_seeded(emu, rows, n, 0x9E3779B97F4A7C15)


def test_seeded_irfft_seeds_differ(emu):
    a = nd.run_seeded(emu, 2, 514, 21)
    b = nd.run_seeded(emu, 2, 514, 22)
    c = nd.run_seeded(emu, 2, 514, 21 + (1 << 32))
    assert int(np.sum(a == b)) == 0 and int(np.sum(a == c)) == 0


def test_seeded_irfft_refusals(emu):
    nd.run_seeded_refusals(emu)


# ----------------------------------------------------------------------------- C
@pytest.mark.parametrize("rows,n", [(1, 7), (3, 1001), (2, 1026)])
def test_python_white(emu, rows, n):
    nd.run_python_white(emu, rows, n, seed=17)


@pytest.mark.parametrize("rows,n", [(1, 4), (3, 1009), (2, 1920)])
def test_python_coloured(emu, rows, n):
    nd.run_python_coloured(emu, rows, n, seed=19)


def test_python_gaussian(emu):
    nd.run_python_gaussian(emu, 3, 1001, seed=23)


def test_python_seedless_ambience_reproduces_its_device_seed(emu):
    nd.run_python_seedless(emu, 2, 1001)


def test_scene_with_device_drawn_ambience_matches_the_oracle_given_the_restated_noise(emu):
    nd.run_scene_against_restated_noise()
