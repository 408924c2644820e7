"""tests/kernel_edges.py on the host-emulated kernels: edge lengths, one length past every grid cap, guard bands and misaligned
interior pointers, each family against its float64 restatement (more than 65 535 rows in al_row_stats and the 60 s noise
lengths only on the GPU: emulated workgroups are too slow for them).  The gfx950 build runs the same scenarios in
tests/test_gpu_kernel_edges.py.

The any-length transform (al_noise_irfft, al_stft, al_istft_ola), by what each length is there for:
  NOISE_N 1..64                     every small length, each radix alone and mixed: every pass a single, partly filled workgroup
  256, 1024                         powers of two (len 128, 512: one workgroup)
  255, 257, 514, 1023, 1025, 8191,  a prime factor above 7: Bluestein, whose power-of-two L is where the radix-4 / 2 passes run
  65537, 2^17 +- 1                  in many workgroups
  ke.NOISE_STOCKHAM_N               the radix-3 / 5 / 7 passes past one workgroup: last workgroup exactly full and just over
                                    full per radix, pure prime powers up to 7^5 with ns growing, all five radices in one
                                    transform, both parities of n for one len (each row's reason stands beside it).  With these
                                    NOISE_N covers every radix in a workgroup other than the first.
  STFT / ISTFT sizes                512, 64 (powers of two), 17, 34, 257, 22 (Bluestein) and ke.STFT_GEOMETRIES: smooth sizes
                                    that are no power of two, one of them multi-block, fft < win, win == hop, fft 1 / 2 / 3
  two launch groups                 more than 32 768 series in al_stft (boundary inside a row) and al_istft_ola (boundary
                                    between the channels of a frame), every element compared; fft = 6 here, 6 and 11 on the GPU
Every workspace of the three is a guarded buffer of exactly al_*_workspace_floats floats."""
import pytest

from audiblelight_amd import _hip, engine
from tests import hostemu, kernel_edges as ke


@pytest.fixture(scope="module")
def emu():
    return engine.Renderer(lib=_hip.Library(hostemu.build()), memory=hostemu.NumpyMemory())


@pytest.fixture(scope="module", autouse=True)
def margins():
    ke.MARGINS.clear()
    yield
    for family, (seen, bound) in sorted(ke.MARGINS.items()):
        print(f"\n[host emulation] {family}: worst {seen:.3g}, bound {bound:.3g}")


@pytest.mark.parametrize("n", ke.EDGE_N + (1, ke.GRID_CAP))
@pytest.mark.parametrize("shift", [0, 1])
def test_emu_fx_pointwise(emu, n, shift):
    ke.run_fx_pointwise(emu, n, shift)


@pytest.mark.parametrize("n", ke.EDGE_N + (ke.GRID_CAP,))
def test_emu_fx_preemphasis(emu, n):
    ke.run_fx_preemphasis(emu, n, 0.97, shift=n % 2)


@pytest.mark.parametrize("coef", [1e-6, 0.5, 0.97, 0.999, 0.9999])
@pytest.mark.parametrize("n", ke.EDGE_N + (3, 2049, 1024 * 7 - 1, ke.GRID_CAP, ke.CLIP_60S))
def test_emu_fx_deemphasis(emu, n, coef):
    ke.run_fx_deemphasis(emu, n, coef, shift=n % 2)


FADES = [  # (n, n_in, n_out): overlapping fades, one-sample fades, fades as long as the clip, none
    (1, 1, 1), (2, 1, 2), (257, 200, 100), (1024, 1024, 1024), (1025, 1, 0), (1025, 0, 1), (255, 0, 0), (1023, 511, 513)]


@pytest.mark.parametrize("shape_in,shape_out", [(s, (s + 2) % 6) for s in range(6)])
@pytest.mark.parametrize("n,n_in,n_out", FADES)
def test_emu_fx_fade(emu, n, n_in, n_out, shape_in, shape_out):
    ke.run_fx_fade(emu, n, n_in, n_out, shape_in, shape_out, shift=n % 2)


def test_emu_fx_fade_grid_stride(emu):
    ke.run_fx_fade(emu, ke.GRID_CAP, 300_001, 900_000, 2, 4)


@pytest.mark.parametrize("n,frame_len,row_len,n_rows", [(1, 3, 2, 1), (255, 16, 8, 20), (1025, 7, 5, 9), (4000, 31, 10, 31),
                                                         (ke.GRID_CAP, 480, 100, 480)])
def test_emu_frame_shuffle(emu, n, frame_len, row_len, n_rows):
    ke.run_frame_shuffle(emu, n, frame_len, row_len, n_rows, shift=n % 2)


@pytest.mark.parametrize("m,n", [(1, 1), (1, 257), (3, 2), (255, 256), (1024, 1023), (1025, 1024), (257, ke.GRID_CAP),
                                 (48000, ke.CLIP_60S)])
def test_emu_wrap_copy(emu, m, n):
    ke.run_wrap_copy(emu, m, n, shift=m % 2)


@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 255), (2, 257), (1, 1025), (2, ke.GRID_CAP_ROWS)])
@pytest.mark.parametrize("shift", [0, 1])
def test_emu_row_scalings(emu, rows, cols, shift):
    ke.run_row_scalings(emu, rows, cols, shift)


def test_emu_row_scalings_past_the_flat_grid_cap(emu):
    rows, cols = 5, ke.GRID_CAP_ROWS            # al_scale_rows / al_scale_rows_f64 launch at most 8192 blocks
    assert rows * cols > ke.GRID_CAP_FLAT
    ke.run_row_scalings(emu, rows, cols, shift=1)


@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025, 4097])
def test_emu_peak_scale(emu, n):
    ke.run_peak_scale(emu, n)


@pytest.mark.parametrize("lens", [[1], [2, 1023, 1024, 1025, 5], [4097] * 7])
def test_emu_clip_scales(emu, lens):
    ke.run_clip_scales(emu, lens)


@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 255), (2, 16383), (2, 16384), (2, 16385), (1, 3 * 16384 + 1), (1, ke.CLIP_60S)])
def test_emu_row_stats(emu, rows, cols):
    ke.run_row_stats(emu, rows, cols)
    ke.run_row_stats(emu, rows, cols, nonfinite=True)


@pytest.mark.parametrize("rows", [1, 2, 63, 64, 65, 1024])
def test_emu_ambience_scales(emu, rows):
    ke.run_ambience_scales(emu, rows, 4801)


RESAMPLE = [  # (rows, n_in, up, down, half, pad)
    (1, 1, 1, 1, 0, 0), (2, 5, 147, 160, 40 * 160, 3),        # input far shorter than the filter
    (2, 1025, 160, 147, 20 * 160, 1), (1, 1023, 147, 160, 20 * 160, 4), (3, 257, 2, 1, 24, 5), (2, 256, 1, 3, 30, 0),
    (1, 1000, 1, 1, 7, 2), (1, ke.GRID_CAP, 1, 1, 4, 3)]


@pytest.mark.parametrize("rows,n_in,up,down,half,pad", RESAMPLE)
def test_emu_resample_poly(emu, rows, n_in, up, down, half, pad):
    ke.run_resample(emu, rows, n_in, up, down, half, pad, shift=pad % 2)


@pytest.mark.parametrize("rows,length,pitch", [(1, 1, 4), (3, 255, 256), (2, 256, 260), (2, 257, 260), (5, 1023, 1024),
                                               (2, 1025, 1028), (1, 4000, 4096)])
@pytest.mark.parametrize("shift", [0, 1])
def test_emu_pack_irs(emu, rows, length, pitch, shift):
    ke.run_pack_irs(emu, rows, length, pitch, shift)


@pytest.mark.parametrize("lens,pitch", [([1], 4), ([0, 3, 255], 256), ([257, 1, 1024, 1025], 1028)])
def test_emu_pack_ragged(emu, lens, pitch):
    ke.run_pack_ragged(emu, lens, pitch, shift=pitch % 8 // 4)


NOISE_N = (list(range(1, 65)) + [257, 514, 255, 256, 1023, 1024, 1025, 8191, 65537, 2 ** 17 - 1, 2 ** 17 + 1]
           + [n for n, _why in ke.NOISE_STOCKHAM_N])


@pytest.mark.parametrize("n", NOISE_N)
def test_emu_noise_irfft(emu, n):
    ke.run_noise_irfft(emu, 2, n)


def test_emu_noise_irfft_three_rows(emu):
    ke.run_noise_irfft(emu, 3, ke.NOISE_STOCKHAM_ROWS3)


@pytest.mark.parametrize("fft,win,hop", [(512, 256, 128), (17, 16, 4), (34, 32, 8), (257, 256, 64), (22, 20, 5), (64, 64, 16)]
                         + ke.STFT_GEOMETRIES)
@pytest.mark.parametrize("n", [1, 255, 1025])
def test_emu_stft(emu, n, fft, win, hop):
    ke.run_stft(emu, 2, n, fft, win, hop)


# An emulated workgroup costs 256 context switches whatever it computes, and a series is at least one workgroup per launch: the
# two-group cases take 20-30 s with the four launches of fft = 6 and over a minute with Bluestein's fft = 11, so the emulation
# keeps the smooth size only (the GPU runs both).
@pytest.mark.parametrize("fft", ke.GROUP_FFTS[:1])
def test_emu_stft_two_launch_groups(emu, fft):
    ke.run_stft(emu, fft=fft, last_written=True, **ke.GROUP_STFT)


@pytest.mark.parametrize("n_frames,n_frames_ir,n_freq,n_ch,n_irs", [(1, 1, 1, 1, 1), (7, 3, 257, 2, 5), (9, 12, 33, 3, 1),
                                                                    (40, 6, 300, 1, 2)])
def test_emu_tv_stft_mac(emu, n_frames, n_frames_ir, n_freq, n_ch, n_irs):
    ke.run_tv_stft_mac(emu, n_frames, n_frames_ir, n_freq, n_ch, n_irs)


@pytest.mark.parametrize("fft,win,hop", [(512, 256, 128), (17, 16, 4), (34, 32, 8), (257, 256, 64), (64, 64, 16)] + ke.STFT_GEOMETRIES)
@pytest.mark.parametrize("n_frames,n_ch", [(5, 1), (9, 3)])
def test_emu_istft_ola(emu, n_frames, n_ch, fft, win, hop):
    ke.run_istft(emu, n_frames, n_ch, fft, win, hop)


@pytest.mark.parametrize("fft", ke.GROUP_FFTS[:1])
def test_emu_istft_ola_two_launch_groups(emu, fft):
    ke.run_istft(emu, fft=fft, last_written=True, **ke.GROUP_ISTFT)


@pytest.mark.parametrize("n_capsules", [1, 3, 4, 7, 8, 12, 16, 31, 32, 33, 40, 64, 65])
@pytest.mark.parametrize("n_samples", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("fmt", [_hip.FRAMES_F32, _hip.FRAMES_PCM16])
def test_emu_encode_frames(emu, n_capsules, n_samples, fmt):
    vector = (n_capsules % 8 == 0) if fmt == _hip.FRAMES_PCM16 else (n_capsules % 4 == 0)
    ke.run_encode(emu, n_capsules, n_samples, fmt, shift=0 if vector else 1)
