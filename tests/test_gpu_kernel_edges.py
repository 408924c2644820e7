"""tests/kernel_edges.py on the real MI355X (gfx950 build), at full size: the device math library (tanhf, exp2f, log10f,
sinpif), the 60 s clip lengths on every family, the any-size FFT at 2 880 000 / 2 880 001 points.  The host emulation runs the
same scenarios in tests/test_hostemu_kernel_edges.py.

The any-length transform (al_noise_irfft, al_stft, al_istft_ola), by what each length is there for:
  NOISE_N 1..64                     every small length, each radix alone and mixed: every pass a single, partly filled workgroup
  256, 1024                         powers of two (len 128, 512: one workgroup)
  255 .. 2^20 +- 1, 2 880 001       a prime factor above 7: Bluestein, whose power-of-two L is where the radix-4 / 2 passes run
                                    in many workgroups
  2 880 000                         len 1 440 000 = 2^8 3^2 5^4, the 60 s ambience
  ke.NOISE_STOCKHAM_N               the radix-3 / 5 / 7 passes past one workgroup: last workgroup exactly full and just over
                                    full per radix, pure prime powers up to 7^5 with ns growing, all five radices in one
                                    transform, both parities of n for one len (each row's reason stands beside it).  With these
                                    NOISE_N covers every radix in a workgroup other than the first.
  ke.NOISE_STOCKHAM_N_GPU           a large ns under each odd radix (len 3 2^18, 5 2^17, 7 2^17) and the long prime powers 5^8, 7^7
  STFT / ISTFT sizes                512, 64 (powers of two), 17, 34, 257, 514, 22 (Bluestein) and ke.STFT_GEOMETRIES: smooth
                                    sizes that are no power of two, one of them multi-block, fft < win, win == hop, fft 1 / 2 / 3
  two launch groups                 more than 32 768 series in al_stft (boundary inside a row) and al_istft_ola (boundary
                                    between the channels of a frame) at a smooth and a Bluestein size, every element compared
Every workspace of the three is a guarded buffer of exactly al_*_workspace_floats floats."""
import pytest

from audiblelight_amd import _hip
from tests import kernel_edges as ke

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from audiblelight_amd import engine

    r = engine.Renderer()
    assert r.lib.path.endswith("libaudiblelight_hip.so")
    return r


@pytest.fixture(scope="module", autouse=True)
def margins():
    ke.MARGINS.clear()
    yield
    for family, (seen, bound) in sorted(ke.MARGINS.items()):
        print(f"\n[gfx950] {family}: worst {seen:.3g}, bound {bound:.3g}")


@pytest.mark.parametrize("n", ke.EDGE_N + (1, ke.GRID_CAP, ke.CLIP_60S))
@pytest.mark.parametrize("shift", [0, 1])
def test_fx_pointwise(gpu, n, shift):
    ke.run_fx_pointwise(gpu, n, shift)


@pytest.mark.parametrize("n", ke.EDGE_N + (ke.GRID_CAP, ke.CLIP_60S))
def test_fx_preemphasis(gpu, n):
    ke.run_fx_preemphasis(gpu, n, 0.97, shift=n % 2)


@pytest.mark.parametrize("coef", [1e-6, 0.5, 0.97, 0.99, 0.999, 0.9999])
@pytest.mark.parametrize("n", ke.EDGE_N + (3, 2049, 1024 * 7 - 1, ke.GRID_CAP, ke.CLIP_60S))
def test_fx_deemphasis(gpu, n, coef):
    ke.run_fx_deemphasis(gpu, n, coef, shift=n % 2)


FADES = [(1, 1, 1), (2, 1, 2), (257, 200, 100), (1024, 1024, 1024), (1025, 1, 0), (1025, 0, 1), (255, 0, 0), (1023, 511, 513),
         (ke.CLIP_60S, 48000, ke.CLIP_60S)]


@pytest.mark.parametrize("shape_in,shape_out", [(s, (s + 2) % 6) for s in range(6)] + [(s, s) for s in range(5)])
@pytest.mark.parametrize("n,n_in,n_out", FADES)
def test_fx_fade(gpu, n, n_in, n_out, shape_in, shape_out):
    ke.run_fx_fade(gpu, n, n_in, n_out, shape_in, shape_out, shift=n % 2)


@pytest.mark.parametrize("n,frame_len,row_len,n_rows", [(1, 3, 2, 1), (255, 16, 8, 20), (1025, 7, 5, 9), (4000, 31, 10, 31),
                                                         (ke.GRID_CAP, 480, 100, 480), (ke.CLIP_60S, 1200, 240, 1200)])
def test_frame_shuffle(gpu, n, frame_len, row_len, n_rows):
    ke.run_frame_shuffle(gpu, n, frame_len, row_len, n_rows, shift=n % 2)


@pytest.mark.parametrize("m,n", [(1, 1), (1, 257), (3, 2), (255, 256), (1024, 1023), (1025, 1024), (257, ke.GRID_CAP),
                                 (48000, ke.CLIP_60S), (ke.CLIP_60S - 1, ke.CLIP_60S)])
def test_wrap_copy(gpu, m, n):
    ke.run_wrap_copy(gpu, m, n, shift=m % 2)


@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 255), (2, 257), (1, 1025), (2, ke.GRID_CAP_ROWS), (4, ke.CLIP_60S)])
@pytest.mark.parametrize("shift", [0, 1])
def test_row_scalings(gpu, rows, cols, shift):
    ke.run_row_scalings(gpu, rows, cols, shift)


@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025, 4097, ke.CLIP_60S])
def test_peak_scale(gpu, n):
    ke.run_peak_scale(gpu, n)


@pytest.mark.parametrize("lens", [[1], [2, 1023, 1024, 1025, 5], [4097] * 7, [ke.CLIP_60S, 48000, ke.CLIP_60S - 1]])
def test_clip_scales(gpu, lens):
    ke.run_clip_scales(gpu, lens)


@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 255), (2, 16383), (2, 16384), (2, 16385), (1, 3 * 16384 + 1), (4, ke.CLIP_60S)])
def test_row_stats(gpu, rows, cols):
    ke.run_row_stats(gpu, rows, cols)
    ke.run_row_stats(gpu, rows, cols, nonfinite=True)


def test_row_stats_more_rows_than_grid_y(gpu):
    ke.run_row_stats(gpu, 65537, 2)
    ke.run_row_stats(gpu, 70001, 17)


@pytest.mark.parametrize("rows", [1, 2, 63, 64, 65, 1024])
def test_ambience_scales(gpu, rows):
    ke.run_ambience_scales(gpu, rows, 4801)


RESAMPLE = [(1, 1, 1, 1, 0, 0), (2, 5, 147, 160, 40 * 160, 3), (2, 1025, 160, 147, 20 * 160, 1), (1, 1023, 147, 160, 20 * 160, 4),
            (3, 257, 2, 1, 24, 5), (2, 256, 1, 3, 30, 0), (1, 1000, 1, 1, 7, 2), (1, ke.GRID_CAP, 1, 1, 4, 3),
            (2, ke.CLIP_60S * 147 // 160, 160, 147, 10 * 160, 4), (1, ke.CLIP_60S, 147, 160, 10 * 160, 0)]


@pytest.mark.parametrize("rows,n_in,up,down,half,pad", RESAMPLE)
def test_resample_poly(gpu, rows, n_in, up, down, half, pad):
    ke.run_resample(gpu, rows, n_in, up, down, half, pad, shift=pad % 2)


@pytest.mark.parametrize("rows,length,pitch", [(1, 1, 4), (3, 255, 256), (2, 256, 260), (2, 257, 260), (5, 1023, 1024),
                                               (2, 1025, 1028), (1, 4000, 4096), (70000, 5, 8)])
@pytest.mark.parametrize("shift", [0, 1])
def test_pack_irs(gpu, rows, length, pitch, shift):
    ke.run_pack_irs(gpu, rows, length, pitch, shift)


@pytest.mark.parametrize("lens,pitch", [([1], 4), ([0, 3, 255], 256), ([257, 1, 1024, 1025], 1028)])
def test_pack_ragged(gpu, lens, pitch):
    ke.run_pack_ragged(gpu, lens, pitch, shift=pitch % 8 // 4)


NOISE_N = list(range(1, 65)) + [255, 256, 257, 514, 1023, 1024, 1025, 8191, 65537, 2 ** 17 - 1, 2 ** 17 + 1, 2 ** 20 - 1,
                                 2 ** 20 + 1, ke.CLIP_60S, ke.CLIP_60S + 1]
NOISE_N += [n for n, _why in ke.NOISE_STOCKHAM_N + ke.NOISE_STOCKHAM_N_GPU]


@pytest.mark.parametrize("n", NOISE_N)
def test_noise_irfft(gpu, n):
    ke.run_noise_irfft(gpu, 2, n)


def test_noise_irfft_three_rows(gpu):
    ke.run_noise_irfft(gpu, 3, ke.NOISE_STOCKHAM_ROWS3)


@pytest.mark.parametrize("fft,win,hop", [(512, 256, 128), (17, 16, 4), (34, 32, 8), (257, 256, 64), (514, 512, 128), (22, 20, 5),
                                         (64, 64, 16)] + ke.STFT_GEOMETRIES)
@pytest.mark.parametrize("n", [1, 255, 1025, 48000])
def test_stft(gpu, n, fft, win, hop):
    ke.run_stft(gpu, 2, n, fft, win, hop)


@pytest.mark.parametrize("fft", ke.GROUP_FFTS)
def test_stft_two_launch_groups(gpu, fft):
    ke.run_stft(gpu, fft=fft, last_written=True, **ke.GROUP_STFT)


@pytest.mark.parametrize("n_frames,n_frames_ir,n_freq,n_ch,n_irs", [(1, 1, 1, 1, 1), (7, 3, 257, 2, 5), (9, 12, 33, 3, 1),
                                                                    (40, 6, 300, 1, 2), (377, 9, 257, 4, 8)])
def test_tv_stft_mac(gpu, n_frames, n_frames_ir, n_freq, n_ch, n_irs):
    ke.run_tv_stft_mac(gpu, n_frames, n_frames_ir, n_freq, n_ch, n_irs)


@pytest.mark.parametrize("fft,win,hop", [(512, 256, 128), (17, 16, 4), (34, 32, 8), (257, 256, 64), (514, 512, 128), (64, 64, 16)]
                         + ke.STFT_GEOMETRIES)
@pytest.mark.parametrize("n_frames,n_ch", [(5, 1), (9, 3), (377, 4)])
def test_istft_ola(gpu, n_frames, n_ch, fft, win, hop):
    ke.run_istft(gpu, n_frames, n_ch, fft, win, hop)


@pytest.mark.parametrize("fft", ke.GROUP_FFTS)
def test_istft_ola_two_launch_groups(gpu, fft):
    ke.run_istft(gpu, fft=fft, last_written=True, **ke.GROUP_ISTFT)


@pytest.mark.parametrize("n_capsules", [1, 3, 4, 7, 8, 12, 16, 31, 32, 33, 40, 64, 65])
@pytest.mark.parametrize("n_samples", [1, 63, 64, 65, 257, 48001])
@pytest.mark.parametrize("fmt", [_hip.FRAMES_F32, _hip.FRAMES_PCM16])
def test_encode_frames(gpu, n_capsules, n_samples, fmt):
    vector = (n_capsules % 8 == 0) if fmt == _hip.FRAMES_PCM16 else (n_capsules % 4 == 0)
    ke.run_encode(gpu, n_capsules, n_samples, fmt, shift=0 if vector else 1)
