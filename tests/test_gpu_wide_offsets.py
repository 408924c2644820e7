"""tests/wide_offset_cases.py on the real MI355X (gfx950 build): every offset, stride and base of the render stage, the mixdown and
the image-source rows next to element 2^31, element 2^32 and byte 2^32 (plain, split and quad layouts), the real-size hspec, and
real passes of the flat kernels over 2^31 + 3077 elements.  No case holds more than 40 GiB of device memory; each skips, with both
figures in the reason, when less than 1.25x its need is free, and hands its memory back before the next one runs."""
import time

import pytest

from tests import wide_offset_cases as wo

pytestmark = pytest.mark.gpu

LAYOUTS = [(10, "plain"), (13, "split"), (14, "quad")]
POSITIONS = ["i31", "i32", "b32"]


@pytest.fixture(scope="module")
def gpu():
    from audiblelight_amd import engine

    r = engine.Renderer()
    assert r.lib.path.endswith("libaudiblelight_hip.so")
    return r


@pytest.fixture(autouse=True)
def release(gpu, request):
    """Wall time and peak device memory of every test (printed: run with -s), and its memory handed back."""
    torch = gpu.mem.torch
    wo.release(gpu)
    torch.cuda.reset_peak_memory_stats(gpu.mem.device)
    t0 = time.perf_counter()
    yield
    gpu.mem.synchronize()
    dt = time.perf_counter() - t0
    peak = torch.cuda.max_memory_allocated(gpu.mem.device)
    print(f"\n[gfx950] {request.node.name}: {dt:.2f} s, peak {peak / 2 ** 30:.2f} GiB")
    assert peak <= wo.CAP_BYTES, f"the case held {peak} bytes of device memory"
    wo.release(gpu)


@pytest.fixture(scope="module", autouse=True)
def margins():
    wo.rd.MARGINS.clear()
    yield
    for family, (seen, bound) in sorted(wo.rd.MARGINS.items()):
        print(f"\n[gfx950] {family}: worst {seen:.3g}, bound {bound:.3g}")


# ----------------------------------------------------------------------------- A. render stage
@pytest.mark.parametrize("position", POSITIONS)
@pytest.mark.parametrize("log2_block,layout", LAYOUTS)
def test_spatial(gpu, log2_block, layout, position):
    wo.run_spatial(gpu, log2_block, layout, position)


@pytest.mark.parametrize("position", POSITIONS)
@pytest.mark.parametrize("log2_block,layout", LAYOUTS)
def test_audio(gpu, log2_block, layout, position):
    wo.run_audio(gpu, log2_block, layout, position)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("which", ["n", "c"])
@pytest.mark.parametrize("log2_block,layout", LAYOUTS)
def test_ir_strides(gpu, log2_block, layout, which, fused):
    wo.run_ir_strides(gpu, log2_block, layout, which, fused)


@pytest.mark.parametrize("position", ["i31", "b32"])
@pytest.mark.parametrize("log2_block,layout", LAYOUTS)
def test_spectra_bases(gpu, log2_block, layout, position):
    wo.run_spectra_bases(gpu, log2_block, layout, position)


@pytest.mark.parametrize("name", [c[0] for c in wo.MAC_CASES])
def test_mac_regime(gpu, name):
    wo.run_mac_regime(gpu, name)


def test_python_layer(gpu):
    wo.run_python_layer(gpu)


def test_hspec_real_size(gpu):
    wo.run_hspec_real_size(gpu)


# ----------------------------------------------------------------------------- B. mixdown
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("position", POSITIONS)
def test_mix_slot_src(gpu, position, accumulate):
    wo.run_mix_slot_src(gpu, position, accumulate=accumulate)


@pytest.mark.parametrize("T,accumulate,ambience", [(2_880_000, False, False), (2_880_001, False, False), (2_880_001, True, False),
                                                   (2_880_000, False, True), (2_880_003, False, True)])
def test_mix_row_base(gpu, T, accumulate, ambience):
    wo.run_mix_row_base(gpu, T, accumulate=accumulate, ambience=ambience)


# ----------------------------------------------------------------------------- C. image-source rows
@pytest.mark.parametrize("tail", [False, True])
def test_ism_shoebox(gpu, tail):
    wo.run_ism_shoebox(gpu, tail=tail)


# ----------------------------------------------------------------------------- D. flat kernels past 2^31 elements
@pytest.mark.parametrize("entry", ["al_scale_rows", "al_scale_rows_f64", "al_axpy", "gain", "clip", "preemph", "al_wrap_copy"])
def test_flat_elementwise(gpu, entry):
    wo.run_flat_elementwise(gpu, entry)


@pytest.mark.parametrize("entry", ["al_scale_matrix_rows", "al_axpy_rows", "al_row_stats", "al_peak_scale"])
def test_flat_rows(gpu, entry):
    wo.run_flat_rows(gpu, entry)


@pytest.mark.parametrize("f64", [False, True])
def test_flat_pack_irs(gpu, f64):
    wo.run_flat_pack_irs(gpu, f64)


def test_flat_normal_fill(gpu):
    wo.run_flat_normal_fill(gpu)


@pytest.mark.parametrize("pcm16,C", [(True, 8), (False, 4), (True, 3), (False, 3)])
def test_flat_encode_frames(gpu, pcm16, C):
    wo.run_flat_encode_frames(gpu, pcm16, C)


def test_flat_pack_ragged(gpu):
    wo.run_flat_pack_ragged(gpu)


def test_flat_fade(gpu):
    wo.run_flat_fade(gpu)


def test_flat_resample_poly(gpu):
    wo.run_flat_resample_poly(gpu)


def test_flat_noise_irfft(gpu):
    wo.run_flat_noise_irfft(gpu)


def test_flat_stft(gpu):
    wo.run_flat_stft(gpu)


def test_ism_dir(gpu):
    wo.run_ism_dir(gpu)


def test_ism_bands(gpu):
    wo.run_ism_bands(gpu)


def test_dry_fetch(gpu):
    wo.run_dry_fetch(gpu)
