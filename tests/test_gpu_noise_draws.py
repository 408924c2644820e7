"""tests/noise_draw_cases.py on the real MI355X (gfx950 build): the device-drawn ambience noise pinned element for element
(the chain A, B, C of that module's docstring), with what emulated workgroups are too slow for: a prefix above the grid cap of
al_normal_fill, and the seeded transform at cfg2's scene length and at an odd Bluestein length above 2^20, compared on the
device, every element."""
import ctypes as ct

import numpy as np
import pytest

from tests import kernel_edges as ke, noise_draw_cases as nd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from audiblelight_amd import engine, synthesize as syn

    r = engine.Renderer()
    assert r.lib.path.endswith("libaudiblelight_hip.so")
    syn.set_renderer(r)
    yield r
    syn.set_renderer(None)


@pytest.fixture(scope="module", autouse=True)
def margins():
    ke.MARGINS.clear()
    yield
    for family, (seen, bound) in sorted(ke.MARGINS.items()):
        print(f"\n[gfx950] {family}: worst {seen:.3g}, bound {bound:.3g}")


BIG = dict(n=nd.FILL_CAP + 4 * 256 * 3 + 5, seed=0xFEDCBA9876543210, tag=2, scale=-1.25)


@pytest.fixture(scope="module")
def big_fill(gpu):
    """One fill that takes a second trip of the grid stride, shared (read-only) by the tests that look at it."""
    got = nd.fill(gpu, BIG["n"], BIG["seed"], BIG["tag"], BIG["scale"]).get()
    got.setflags(write=False)
    return got


# ----------------------------------------------------------------------------- A
@pytest.mark.parametrize("n", nd.FILL_SMALL_N)
def test_normal_fill_small_lengths(gpu, n):
    nd.run_fill(gpu, n, nd.SEEDS[n % 3], nd.TAGS[n % 4])


@pytest.mark.parametrize("seed", nd.SEEDS)
@pytest.mark.parametrize("tag", nd.TAGS)
def test_normal_fill_tags_and_seeds(gpu, seed, tag):
    nd.run_fill(gpu, 1027, seed, tag)


@pytest.mark.parametrize("n", [5, 1026, 2049])
def test_normal_fill_scales(gpu, n):
    for scale in (1.0, -0.37, nd.white_scale(n)):
        nd.run_fill(gpu, n, 0xABCDEF0123, 2, scale)


def test_normal_fill_streams_are_independent(gpu):
    nd.run_fill_independence(gpu)


def test_normal_fill_second_grid_stride_trip(gpu, big_fill):
    cap, n = nd.FILL_CAP, BIG["n"]
    mid = int(np.random.default_rng(7).integers(4096, cap - 2 * 4096))
    for lo, hi in ((0, 4096), (cap - 4096, n), (mid, mid + 4096)):
        nd.check_draws(big_fill[lo:hi], nd.restated_normals(BIG["seed"], BIG["tag"], lo, hi), BIG["scale"],
                       "normal_fill (err / tolerance)", ("second trip", lo, hi))
    assert int(np.sum(big_fill[cap:cap + 4096] == big_fill[:n - cap][:4096])) == 0          # the second trip did not start over


def test_normal_fill_is_independent_of_the_launch_geometry(gpu, big_fill):
    for k in (37, 1025, 4 * 256 * 40 + 2, nd.FILL_CAP + 1):          # below and above the grid cap
        ke.assert_bits_equal(nd.fill(gpu, k, BIG["seed"], BIG["tag"], BIG["scale"]).get(), big_fill[:k], ("prefix", k))


def test_normal_fill_refusals(gpu):
    nd.run_fill_refusals(gpu)


# ----------------------------------------------------------------------------- B
@pytest.mark.parametrize("n", nd.SEEDED_N)
@pytest.mark.parametrize("shaped", [True, False], ids=["pink", "nullptr"])
def test_seeded_irfft_is_the_explicit_irfft_of_the_device_draws(gpu, n, shaped):
    rows = 1 + n % 3
    nd.run_seeded(gpu, rows, n, nd.SEEDS[n % 3], shaped)


@pytest.mark.parametrize("rows,n", [(3, 513), (5, 514), (5, 1009)])
def test_seeded_irfft_rows(gpu, rows, n):
    assert (n // 2 + 1) % 4 and (n // 2 + 1) % 256
    nd.run_seeded(gpu, rows, n, 0x9E3779B97F4A7C15)


def test_seeded_irfft_seeds_differ(gpu):
    a = nd.run_seeded(gpu, 2, 514, 21)
    b = nd.run_seeded(gpu, 2, 514, 22)
    c = nd.run_seeded(gpu, 2, 514, 21 + (1 << 32))
    assert int(np.sum(a == b)) == 0 and int(np.sum(a == c)) == 0


def test_seeded_irfft_refusals(gpu):
    nd.run_seeded_refusals(gpu)


@pytest.mark.parametrize("rows,n", [(4, 2_880_000), (2, (1 << 20) + 1)], ids=["cfg2 scene length", "odd Bluestein above 2^20"])
def test_seeded_irfft_at_full_size(gpu, rows, n):
    """The seeded transform against the explicit one on the draws of the tag-1 fill, on the device, every element; the fill is
    held to the restatement at its ends and on both sides of every row's first counter block (row * bins)."""
    torch = gpu.mem.torch
    seed, bins = 0xA5A5A5A55A5A5A5A, n // 2 + 1
    assert bins % 4 and bins % 256
    drawn = nd.fill(gpu, 4 * rows * bins, seed, nd.TAG_SPECTRUM)
    host = drawn.get()
    for at in [0] + [4 * row * bins for row in range(1, rows)] + [4 * rows * bins]:
        lo, hi = max(at - 2048, 0), min(at + 2048, 4 * rows * bins)
        nd.check_draws(host[lo:hi], nd.restated_normals(seed, nd.TAG_SPECTRUM, lo, hi), 1.0, "normal_fill (err / tolerance)", (n, lo, hi))
    flat = drawn.buf[drawn.lo:drawn.hi].view(torch.float32)
    zr, zi = flat[0::4].contiguous(), flat[1::4].contiguous()
    shape, inv_sigma = nd.pink_shape(n)
    d_s = ke.dev(gpu, shape)
    floats = gpu.lib.call("al_noise_workspace_floats", rows, n)
    outs = []
    for explicit in (False, True):
        work, out = ke.workspace(gpu, floats), ke.Guarded(gpu, rows * n)
        if explicit:
            gpu.lib.call("al_noise_irfft", zr.data_ptr(), zi.data_ptr(), gpu.mem.ptr(d_s), rows, n, ct.c_float(inv_sigma), out.ptr,
                         work.ptr, gpu.mem.stream())
        else:
            gpu.lib.call("al_noise_irfft_seeded", ct.c_uint64(seed), gpu.mem.ptr(d_s), rows, n, ct.c_float(inv_sigma), out.ptr,
                         work.ptr, gpu.mem.stream())
        gpu.mem.synchronize()
        outs.append(out)
        work.get()
        del work
    a, b = (o.buf[o.lo:o.hi].view(torch.int32) for o in outs)
    differing = int((a != b).sum().item())
    assert differing == 0, f"{differing} of {rows * n} elements differ between the seeded and the explicit transform"
    got = outs[0].get().reshape(rows, n)
    outs[1].get()
    assert np.all(np.isfinite(got)) and np.all(got.std(axis=1) > 0.5)       # 1 / sigma: unit variance in expectation
    for r0 in range(rows):
        for r1 in range(r0 + 1, rows):
            assert float(np.mean(got[r0] == got[r1])) < 1e-3, ("rows repeat", r0, r1)


# ----------------------------------------------------------------------------- C
@pytest.mark.parametrize("rows,n", [(1, 7), (3, 1001), (2, 1026)])
def test_python_white(gpu, rows, n):
    nd.run_python_white(gpu, rows, n, seed=17)


@pytest.mark.parametrize("rows,n", [(1, 4), (3, 1009), (2, 1920)])
def test_python_coloured(gpu, rows, n):
    nd.run_python_coloured(gpu, rows, n, seed=19)


def test_python_gaussian(gpu):
    nd.run_python_gaussian(gpu, 3, 1001, seed=23)


def test_python_seedless_ambience_reproduces_its_device_seed(gpu):
    nd.run_python_seedless(gpu, 2, 1001)


def test_scene_with_device_drawn_ambience_matches_the_oracle_given_the_restated_noise(gpu):
    nd.run_scene_against_restated_noise()
