"""The host-device transfer paths and the switches no other test sets, on the gfx950 build (scenarios: tests/transfer_cases.py).

Staging buffers (TorchMemory.upload_f64_as_f32 past one chunk, upload_staged, upload_tables), upload_async, kernels storing into
page-locked host memory (AL_D2H=kernel), the batch driver under AL_D2H x AL_H2D x AL_F64_UPLOAD, the alignment gaps of the
packed audio, TorchMemory.download around its threshold, AL_CONVERT_THREADS, AL_TRIM_PARTITIONS=0 and AL_STATIC_MAC_MAX_P.
Everything is compared bit for bit; the only tolerance is the suite's parity contract on the driver's baseline run.
"""
import itertools

import numpy as np
import pytest

from audiblelight_amd import _hip
from tests import transfer_cases as tc
from tests.conftest import PARITY_TOL, assert_parity, pcm16, set_switch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from audiblelight_amd import engine

    r = engine.Renderer()
    assert r.lib.path.endswith("libaudiblelight_hip.so")
    return r


# ----------------------------------------------------------------------------- 1. float64 -> float32 upload across chunks
@pytest.fixture(scope="module")
def f64_a():
    irs = tc.f64_tensor(tc.F64_A, seed=1)
    assert irs.size == 12_582_930 and list(tc.chunk_bounds(irs.size)) == [0, 4194310, 8388620, 12582930]
    return irs, irs.astype(np.float32)


@pytest.mark.parametrize("threads", [1, 7, 16])
def test_f64_upload_three_chunks(gpu, monkeypatch, f64_a, threads):
    """upload_f64_as_f32 past one chunk (chunk k + 1 cast while chunk k is on its way), AL_CONVERT_THREADS threads per chunk:
    every row equals ``irs.astype(float32)``, the pad floats of the re-pitched rows are finite."""
    set_switch(monkeypatch, "AL_CONVERT_THREADS", threads)
    tc.run_f64_upload_threads(gpu, f64_a[0], f64_a[1], threads)


def test_f64_upload_three_chunks_equals_device_cast(gpu, monkeypatch, f64_a):
    """The host cast over three chunks and the device cast (AL_F64_UPLOAD=device: al_pack_irs_f64) put the same bits into HBM;
    so does the switch itself, which is what ``host_cast=None`` reads."""
    set_switch(monkeypatch, "AL_F64_UPLOAD", None)
    host, s_host = gpu.upload_irs(f64_a[0])
    dev, s_dev = gpu.upload_irs(f64_a[0], host_cast=False)
    assert s_host == s_dev and tc.same_device_bits(host, dev)
    tc.check_irs(gpu, dev, s_dev, f64_a[0], f64_a[1], "device cast")
    del host, dev
    set_switch(monkeypatch, "AL_F64_UPLOAD", "device")
    calls = []
    monkeypatch.setattr(gpu.mem, "upload_f64_as_f32", lambda *a, **k: calls.append(1))
    by_switch, s_switch = gpu.upload_irs(f64_a[0])
    assert not calls and s_switch == s_dev
    tc.check_irs(gpu, by_switch, s_switch, f64_a[0], f64_a[1], "AL_F64_UPLOAD=device")


def test_f64_staging_buffer_reuse(gpu, f64_a):
    """The reuse guard of the float64 cast's page-locked buffer (``cv["last"]``) and its growth: transfer_cases.run_f64_staging_reuse.
    The ordering of the uploads makes a missing guard likely to show, not certain; the content check is the assertion."""
    tensors = (f64_a[0], tc.f64_tensor(tc.F64_B, 2), tc.f64_tensor(tc.F64_C, 3), tc.f64_tensor(tc.F64_ONE_CHUNK, 4),
               tc.f64_tensor(tc.F64_ONE_CHUNK, 5))
    tc.run_f64_staging_reuse(gpu.lib, tensors)


# ----------------------------------------------------------------------------- 2. upload_staged, upload_tables
def test_upload_staged_reuse_and_growth(gpu):
    """One tag's page-locked staging buffer reused and regrown with nothing synchronised in between (``slot[1].synchronize()``)."""
    tc.run_upload_staged_reuse(gpu.mem)


def test_upload_tables_pieces(gpu):
    """Five tables of five dtypes through one arena: alignment, dtype and bytes of every piece; a second call leaves the first alone."""
    tc.run_upload_tables(gpu.mem)


# ----------------------------------------------------------------------------- 3. upload_async (AL_H2D=async)
@pytest.mark.parametrize("name,view", [("f32_aligned", False), ("f32_aligned", True), ("f32_ragged", False), ("f32_ragged", True),
                                       ("f64_ragged", False)])
def test_upload_async(gpu, name, view):
    """Page-locked in place + asynchronous DMA (what AL_H2D=async does per scene) against the inline upload, for the three routes
    behind it (no kernel, al_pack_irs_f32, al_pack_irs_f64) and from a non-contiguous view."""
    tc.run_upload_async(gpu, name, view)


@pytest.mark.parametrize("name", sorted(tc.ASYNC_INPUTS))
def test_upload_async_falls_back_when_registration_fails(gpu, monkeypatch, name):
    """hipHostRegister refusing the array: the inline copy puts the same bits into HBM, ``release`` does nothing and nothing is
    unregistered."""
    rt = gpu.mem.torch.cuda.cudart()
    unregistered = []
    monkeypatch.setattr(rt, "cudaHostRegister", lambda *a: 1)
    monkeypatch.setattr(rt, "cudaHostUnregister", lambda *a: unregistered.append(a) or 0)
    tc.run_upload_async(gpu, name, False, expect_registered=False)
    assert not unregistered


# ----------------------------------------------------------------------------- 4. kernels storing into page-locked host memory
@pytest.mark.parametrize("n_capsules", [1, 2, 3, 5, 4, 8])      # 4 (float32) and 8 (PCM_16): the 16-byte vector stores
@pytest.mark.parametrize("n_samples", [1, 7, 8, 9, 1025])
@pytest.mark.parametrize("fmt", [_hip.FRAMES_F32, _hip.FRAMES_PCM16])
def test_encode_frames_into_pinned_host_memory(gpu, n_capsules, n_samples, fmt):
    """What AL_D2H=kernel does with the frames: kernel_edges.run_encode's cases, the destination a guarded page-locked host buffer."""
    vector = (n_capsules % 8 == 0) if fmt == _hip.FRAMES_PCM16 else (n_capsules % 4 == 0)
    tc.run_encode_to_host(gpu, n_capsules, n_samples, fmt, shift=0 if vector else n_samples % 2)


@pytest.mark.parametrize("m", [1, 255, 257])
@pytest.mark.parametrize("long", [False, True])
def test_wrap_copy_into_pinned_host_memory(gpu, m, long):
    """What AL_D2H=kernel does with the scene: kernel_edges.run_wrap_copy's cases into a guarded page-locked host buffer."""
    tc.run_wrap_copy_to_host(gpu, m, 2 * m + 1 if long else m, shift=m % 2)


# ----------------------------------------------------------------------------- 5. the batch driver under its switch matrix
@pytest.fixture(scope="module")
def driver_baseline(gpu, tmp_path_factory):
    """One default-switch run per subtype, held to the oracle at the suite's contract tolerance; the matrix compares with it."""
    from audiblelight_amd import switches
    from tests.test_gpu_configs import oracle_scene

    sw = switches.reload()
    assert (sw.d2h, sw.h2d, sw.f64_upload) == ("dma", "blocking", "host"), sw.non_default()
    scenes = tc.driver_scenes()
    jobs = tc.driver_jobs(scenes)
    assert [j.irs.dtype == np.float64 for j in jobs] == [False, True] * 3 + [False] and jobs[3].irs.shape[2] % 4 == 1
    assert len(jobs[5].clips) == len(jobs[4].clips) - 1
    base = {}
    out = tmp_path_factory.mktemp("driver_baseline")
    for subtype in ("FLOAT", "PCM_16"):
        _, _, got, wavs = tc.run_driver(gpu, jobs, out / subtype, subtype)
        for i, sc in enumerate(scenes):
            assert_parity(got[f"s{i}"], oracle_scene(sc), PARITY_TOL, what=(subtype, i))
            want_wav = got[f"s{i}"].T if subtype == "FLOAT" else pcm16(got[f"s{i}"].T)
            np.testing.assert_array_equal(wavs[f"s{i}"], want_wav)
        base[subtype] = (got, wavs)
    return jobs, base


@pytest.mark.parametrize("d2h,h2d,f64", list(itertools.product(tc.D2H, tc.H2D, tc.F64)),
                         ids=["-".join(p) for p in itertools.product(tc.D2H, tc.H2D, tc.F64)])
def test_batch_driver_switch_matrix(gpu, monkeypatch, tmp_path, driver_baseline, d2h, h2d, f64):
    """Every point of AL_D2H x AL_H2D x AL_F64_UPLOAD (the default point again, on a fresh driver): the kernels are the same and
    only the route differs, so every on_scene array and every WAV payload equals the baseline's bit for bit; files come back in
    job order; float64 IRs count 4 bytes per element under ``host`` and 8 under ``device``.  The same driver object runs twice
    (FLOAT, then PCM_16), so the second run starts on used input slots and used page-locked scene buffers."""
    from audiblelight_amd import batch

    jobs, base = driver_baseline
    set_switch(monkeypatch, "AL_D2H", d2h)
    set_switch(monkeypatch, "AL_H2D", h2d)
    set_switch(monkeypatch, "AL_F64_UPLOAD", f64)
    drv = batch.BatchDriver(gpu, depth=2, writers=2)            # the switches are read here
    assert drv.zero_copy_d2h == (d2h == "kernel") and drv.async_h2d == (h2d == "async") and (drv.cast_threads > 0) == (f64 == "host")
    for subtype in ("FLOAT", "PCM_16"):
        _, _, got, wavs = tc.run_driver(gpu, jobs, tmp_path / subtype, subtype, drv=drv, f64_upload=f64)
        tc.assert_same_run(got, wavs, base[subtype][0], base[subtype][1], (d2h, h2d, f64, subtype))


# ----------------------------------------------------------------------------- 6. gaps of the packed audio are never heard
@pytest.mark.parametrize("fold", [False, True], ids=["plain_clips", "folded_clips"])
@pytest.mark.parametrize("layout,log2_block", tc.GAP_LAYOUTS, ids=[f"{name}{lb}" for name, lb in tc.GAP_LAYOUTS])
def test_audio_gaps_are_never_read(gpu, layout, log2_block, fold):
    """prepare() and BatchDriver._plan hand pack_audio a REUSED buffer, whose alignment gaps hold the previous scene's samples:
    no kernel output may depend on them (transfer_cases.run_gap_render: zeros against the sentinel NaN in every gap).
    Outcome: no kernel reads a gap -- the signal transforms clamp their loads to the clip and mask by position, the dry path and
    al_clip_scales stop at ``len`` -- so nothing had to change in pack_audio."""
    tc.run_gap_render(gpu, log2_block, layout, fold)


# ----------------------------------------------------------------------------- 8. download on both sides of its threshold
def test_download_threshold(gpu):
    """TorchMemory.download below and at 4 MiB (pageable / page-locked); a downloaded array keeps its block."""
    tc.run_download_threshold(gpu.mem)


# ----------------------------------------------------------------------------- 9. the accumulate and transform switches
def test_trim_partitions_off(gpu, monkeypatch):
    """AL_TRIM_PARTITIONS=0 (transfer_cases.run_untrimmed_moving): every partition transformed, every row at the oracle, and the
    kept samples bit for bit those of the trimmed render -- k_spectral_mac_moving adds the partitions in the same order either way."""
    tc.run_untrimmed_moving(gpu, lambda name, value: set_switch(monkeypatch, name, value))


@pytest.mark.parametrize("log2_block", [11, 13])      # at B = 1024 the case's IR is exactly 6 partitions long: not its shape
def test_static_mac_max_p(gpu, monkeypatch, log2_block):
    """AL_STATIC_MAC_MAX_P on both sides of P = 7: capsule loop (3120701) at 7, tile kernel (81201) at 6."""
    tc.run_static_mac_max_p(gpu, lambda name, value: set_switch(monkeypatch, name, value), log2_block)
