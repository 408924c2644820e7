"""Scenarios for the layer that carries bytes between the host and the kernels: the staging paths of engine.TorchMemory
(upload_f64_as_f32, upload_staged, upload_tables, upload_async, download), Renderer.pack_audio, the kernels that store into
page-locked host memory, the batch driver under its AL_D2H x AL_H2D x AL_F64_UPLOAD switch matrix, and the two dispatch
switches no other test sets (AL_TRIM_PARTITIONS, AL_STATIC_MAC_MAX_P).  Run by tests/test_gpu_transfers.py (gfx950) and, for the
host-only part, tests/test_host_logic.py.

These are data-movement claims: every comparison is bit for bit (kernel_edges.assert_bits_equal / np.array_equal) unless a
scenario says otherwise.  The reuse guards of the page-locked staging buffers (an event of the last DMA out of a buffer, waited
for before the buffer is written again) cannot be tested for certain: a missing guard is a race.  The scenarios order the calls
so that the race, if it were there, would very likely be lost -- a write into the part of the buffer the DMA has not reached
yet -- and then assert the CONTENT of every device buffer, each against its own source.
"""
import numpy as np

from audiblelight_amd import _hip, engine
from audiblelight_amd import plan as planning
from tests import kernel_edges as ke
from tests import mac_regimes as mr
from tests import render_edges as re_

# ----------------------------------------------------------------------------- 1. float64 -> float32 upload across chunks
# upload_f64_as_f32 cuts n elements into max(1, min(8, n // 2^22)) chunks and every chunk into one range per thread.
F64_A = (2, 3, 2_097_155)       # 12 582 930 elements: three chunks [0, 4194310, 8388620, 12582930], nothing divides by 7 or 16,
                                # and an odd row length (al_pack_irs_f32 re-pitches behind the upload)
F64_B = (1, 1, 1001)
F64_C = (2, 3, 2_621_443)       # 15 728 658 elements: more than A's page-locked buffer holds (12 648 448), less than 5/4 of it, so
                                # the buffer is reallocated and the "at least a quarter more" rule sets its size
F64_ONE_CHUNK = (1, 2, 4_194_301)   # 8 388 602 elements < 2^23: ONE chunk, so the next cast starts while all of it is on its way
# float64 values whose float32 rounding is a tie, a denormal, or just above / below one: planted on both sides of every chunk bound
ROUNDING_EDGES = np.array([1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 0.5 + 2.0 ** -25, -0.0, 1e-42, 7e-46, -(1 + 2.0 ** -24), 1 - 2.0 ** -25])


def chunk_bounds(n):
    """The chunk bounds upload_f64_as_f32 takes for n elements (restated: the test's own arithmetic, not a call)."""
    return np.linspace(0, n, max(1, min(8, n // (1 << 22))) + 1).astype(np.int64)


def f64_tensor(shape, seed):
    """Gaussian float64 IRs with the rounding edges around every chunk bound and at both ends."""
    x = np.random.default_rng(seed).standard_normal(shape)
    flat = x.reshape(-1)
    k = min(len(ROUNDING_EDGES), flat.size // 2)
    for b in chunk_bounds(flat.size):
        lo = int(min(max(b - k // 2, 0), flat.size - k))
        flat[lo: lo + k] = ROUNDING_EDGES[:k]
    return x


def irs_rows(r, dev, strides, shape):
    """The (C, N, pitch) float32 rows behind what upload_irs returned."""
    c, n, l = shape
    lp = (l + 3) // 4 * 4
    assert tuple(strides) == (n * lp, lp), (strides, shape)
    return np.asarray(r.mem.download(dev))[: c * n * lp].reshape(c, n, lp)


def check_irs(r, dev, strides, irs, want32=None, what=None):
    """Every row holds the float32 cast of its source (numpy's round-to-nearest-even), the pad floats of every row are finite."""
    rows = irs_rows(r, dev, strides, irs.shape)
    l = irs.shape[2]
    ke.assert_bits_equal(rows[:, :, :l], irs.astype(np.float32) if want32 is None else want32, what)
    assert np.isfinite(rows[:, :, l:]).all(), (what, "pad floats")
    return rows


def same_device_bits(a, b):
    import torch

    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


def run_f64_upload_threads(r, irs, want32, threads):
    """AL_CONVERT_THREADS (set by the caller) is the pool's size; the upload holds ``irs.astype(float32)`` in every row."""
    dev, strides = r.upload_irs(irs, host_cast=True)
    assert r.mem._convert["threads"] == threads, (r.mem._convert["threads"], threads)
    check_irs(r, dev, strides, irs, want32, ("host cast", threads))
    return dev, strides


def run_f64_staging_reuse(lib, tensors):
    """A, B, C (see above) and then two one-chunk tensors uploaded back to back on a memory provider of its own (so the
    page-locked buffer starts empty and C does reallocate it), nothing synchronised in between; only then is every upload
    downloaded and compared with its own source.

    What a missing ``cv["last"].synchronize()`` would do: A's last chunk (16.8 MB, 0.3 ms of DMA at the 56 GB/s of
    profiles/r02_h2d_probe.txt) is still on its way when the cast of B begins microseconds later.  B only writes the first 1001
    floats of the buffer, which that DMA does not read, so B by itself would rarely show it; the pair X, Y at the end does:
    both are ONE chunk of 8 388 602 elements, and Y's cast writes every thread's range of the buffer at once while X's 33.5 MB
    DMA (0.6 ms) has barely started.  Likely to show, not certain: the content check is the assertion.  (Tried once on an MI355X
    with the guard taken out: X came back holding Y's samples and the test failed there.)"""
    r = engine.Renderer(lib=lib, memory=engine.TorchMemory())
    (a, b, c, x, y) = tensors
    ups = [r.upload_irs(a, host_cast=True)]
    cap_a = r.mem._convert["host"].numel()
    ups.append(r.upload_irs(b, host_cast=True))
    assert r.mem._convert["host"].numel() == cap_a                      # B fits: the same buffer
    assert cap_a == (a.size + 65535) // 65536 * 65536 and cap_a < c.size < cap_a * 5 // 4
    ups.append(r.upload_irs(c, host_cast=True))
    cap_c = r.mem._convert["host"].numel()
    assert cap_c == (cap_a * 5 // 4 + 65535) // 65536 * 65536 and cap_c >= c.size      # a new buffer, a quarter larger
    ups.append(r.upload_irs(x, host_cast=True))
    ups.append(r.upload_irs(y, host_cast=True))
    assert r.mem._convert["host"].numel() == cap_c
    for name, src, (dev, strides) in zip("ABCXY", (a, b, c, x, y), ups):
        check_irs(r, dev, strides, src, what=("staging reuse", name))


# ----------------------------------------------------------------------------- 2. upload_staged, upload_tables
def pattern(n, base):
    """float32[n] with a distinct bit pattern per call (``base``) and per index."""
    return (np.arange(n, dtype=np.uint32) + np.uint32(base)).view(np.float32)


def run_upload_staged_reuse(mem, tag="transfer-test"):
    """Calls under one tag, back to back, nothing synchronised in between: 2^24 floats P, 1000 floats Q (the buffer is reused),
    2^24 floats P2 and at once a call R of the same size whose ``fill`` rewrites ONLY the last 1000 floats (the buffer still
    holds P2 elsewhere), then one larger than 5/4 of the first (the buffer is reallocated).  Every returned device buffer must hold its own pattern.

    Without ``slot[1].synchronize()`` Q would land in the first 4 KB of a 67 MB DMA that has been going for microseconds
    (likely already read), but Q's own 4 KB DMA queues behind that one and P2's fill rewrites its source first; R's tail write
    lands where P2's DMA arrives a millisecond later, so P2's device copy would end in R's pattern.  Likely, not certain: the
    contents are the assertion.  (Tried once on an MI355X with the guard taken out: Q came back holding P2's pattern.)"""
    n = 1 << 24
    p, q, p2, tail = pattern(n, 0x10000000), pattern(1000, 0x20000000), pattern(n, 0x30000000), pattern(1000, 0x40000000)
    big_n = n * 5 // 4 + 70001
    big = pattern(big_n, 0x50000000)
    put = lambda src: (lambda view: np.copyto(view, src))  # noqa: E731
    d_p = mem.upload_staged(n, put(p), tag=tag)
    host0 = mem._staging_by_tag[tag][0]
    d_q = mem.upload_staged(1000, put(q), tag=tag)
    d_p2 = mem.upload_staged(n, put(p2), tag=tag)
    d_r = mem.upload_staged(n, lambda view: np.copyto(view[-1000:], tail), tag=tag)
    assert mem._staging_by_tag[tag][0] is host0                          # one buffer so far
    d_big = mem.upload_staged(big_n, put(big), tag=tag)
    assert mem._staging_by_tag[tag][0] is not host0 and mem._staging_by_tag[tag][0].numel() >= big_n
    r_want = p2.copy()
    r_want[-1000:] = tail
    for name, dev, want in (("P", d_p, p), ("Q", d_q, q), ("P2", d_p2, p2), ("R", d_r, r_want), ("big", d_big, big)):
        assert dev.numel() == want.size, name
        ke.assert_bits_equal(np.asarray(mem.download(dev)), want, ("upload_staged", name))
    del mem._staging_by_tag[tag]                                        # 84 MB of page-locked memory: back to the allocator


def table_set(seed):
    rng = np.random.default_rng(seed)
    events = np.zeros(3, _hip.EVENT_DTYPE)
    events.view(np.uint8)[:] = rng.integers(0, 256, events.nbytes, dtype=np.uint8)
    return [events, rng.integers(0, 256, 1, dtype=np.uint8), np.zeros(0, np.float32),
            rng.integers(-2 ** 31, 2 ** 31, 5).astype(np.int32), rng.standard_normal(3)]


def run_upload_tables(mem):
    """A structured table, a 1-byte table, an empty one, an int32 and a float64 one in ONE call: every piece 16-byte aligned,
    in its dtype (uint8 for the structured one), with its own bytes; a second call right behind the first (same arena, no
    synchronisation in between) leaves the first call's device tensors as they were."""
    import torch

    first, second = table_set(1), table_set(2)
    d_first = mem.upload_tables(first)
    d_second = mem.upload_tables(second)
    for tabs, devs in ((first, d_first), (second, d_second)):
        assert len(devs) == len(tabs)
        for i, (a, d) in enumerate(zip(tabs, devs)):
            assert d.data_ptr() % 16 == 0, (i, d.data_ptr())
            want_dtype = torch.uint8 if a.dtype.fields is not None else getattr(torch, a.dtype.name)
            assert d.dtype == want_dtype and d.is_cuda, (i, d.dtype)
            want = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
            got = d.cpu().numpy().reshape(-1).view(np.uint8)
            if a.dtype == np.uint8:                      # a uint8 piece is handed out whole (at least one byte)
                got = got[: want.size]
            assert got.size == want.size and np.array_equal(got, want), (i, "bytes")
    assert d_first[2].numel() == 0 and d_first[4].numel() == 3 and d_first[3].numel() == 5


# ----------------------------------------------------------------------------- 3. upload_async
ASYNC_INPUTS = {      # name -> (dtype, row length, the kernel behind the copy)
    "f32_aligned": (np.float32, 4100, None),
    "f32_ragged": (np.float32, 4101, "al_pack_irs_f32"),
    "f64_ragged": (np.float64, 4099, "al_pack_irs_f64"),
}


def async_input(name, view):
    """(3, 2, l) IRs; ``view``: every other emitter column of a (3, 4, l) array (not contiguous)."""
    dtype, l, _ = ASYNC_INPUTS[name]
    x = np.random.default_rng(len(name) + l).standard_normal((3, 4 if view else 2, l)).astype(dtype)
    x.reshape(-1)[:4] = [-0.0, 1e-42, 1 + 2.0 ** -24, -1.0]
    return x[:, ::2] if view else x


def run_upload_async(r, name, view, expect_registered=True):
    """upload_irs(async_release=...) puts the same bits into HBM as the inline upload, appends exactly one ``release``, and
    leaves the caller's array as it was, writable.  Returns what ``release()`` returned."""
    irs = async_input(name, view)
    assert irs.flags.c_contiguous != view
    before = irs.copy()
    want, want_strides = r.upload_irs(irs)
    rel = []
    got, strides = r.upload_irs(irs, async_release=rel, host_cast=False)
    assert tuple(strides) == tuple(want_strides)
    assert len(rel) == 1 and callable(rel[0])
    r.mem.synchronize()
    assert same_device_bits(got, want), name
    check_irs(r, got, strides, irs, what=("upload_async", name, view))
    rc = rel[0]()
    ke.assert_bits_equal(irs, before, ("source changed", name))
    assert irs.flags.writeable
    irs[0, 0, :8] = 3.0                                   # still ordinary memory after the pages were unlocked
    assert np.all(irs[0, 0, :8] == 3.0)
    if expect_registered:
        assert rc is not None and int(rc) == 0, rc
    else:
        assert rc is None
    return rc


# ----------------------------------------------------------------------------- 4. kernels storing into page-locked host memory
class PinnedGuarded:
    """The host twin of kernel_edges.Guarded: ONE page-locked allocation, ``guard`` sentinel elements on each side of the
    interior, checked after a stream synchronisation.  ``ptr`` is the HOST address of the interior (page-locked memory is
    mapped into the GPU's address space under the same address); a stray store lands in the same allocation and is seen."""

    def __init__(self, r, n, dtype=np.float32, shift=0, init=None, guard=ke.G):
        import torch

        self.r, self.n, self.dtype = r, int(n), np.dtype(dtype)
        item = self.dtype.itemsize
        self.lo = (guard + shift) * item
        self.hi = self.lo + self.n * item
        total = (self.hi + guard * item + 3) // 4 * 4
        self.host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        assert self.host.is_pinned()
        raw = self.host.numpy()
        raw[:] = ke.sentinel_bytes(total)
        if init is not None:
            raw[self.lo:self.hi] = np.ascontiguousarray(init, dtype=self.dtype).reshape(-1).view(np.uint8)
        self.ptr = self.host.data_ptr() + self.lo
        assert shift != 0 or self.ptr % 16 == 0, "guarded interior lost its 16-byte alignment"

    def get(self):
        self.r.mem.synchronize()
        raw = self.host.numpy()
        expect = ke.sentinel_bytes(len(raw))
        bad = np.flatnonzero(np.concatenate([raw[:self.lo] != expect[:self.lo], raw[self.hi:] != expect[self.hi:]]))
        assert bad.size == 0, f"{bad.size} guard bytes overwritten (first at byte {int(bad[0])} of the guards)"
        return raw[self.lo:self.hi].view(self.dtype).copy()


def run_encode_to_host(r, n_capsules, n_samples, fmt, shift=0):
    """al_encode_frames with ``out`` in page-locked host memory (BatchDriver under AL_D2H=kernel): kernel_edges.run_encode's
    own inputs and expected frames, the destination swapped."""
    return ke.run_encode(r, n_capsules, n_samples, fmt, shift=shift, guarded=PinnedGuarded)


def run_wrap_copy_to_host(r, m, n, shift=0):
    return ke.run_wrap_copy(r, m, n, shift=shift, guarded=PinnedGuarded)


# ----------------------------------------------------------------------------- 5. the batch driver under its switch matrix
N_SCENES = 7          # more than the driver's four input slots: slots are reused
D2H, H2D, F64 = ("dma", "kernel"), ("blocking", "async"), ("host", "device")


def driver_scenes():
    """Seven cfg1 scenes at a quarter of the size that differ in size and dtype from one to the next: odd ones carry float64
    IRs, scene 3 an odd row length, scene 5 one event (and one IR column) fewer -- the clip buffer of its slot shrinks."""
    from audiblelight_amd import synthetic

    scenes = [synthetic.make_scene("cfg1", scene_index=i, scale=0.25) for i in range(N_SCENES)]
    scenes[3].irs = np.ascontiguousarray(scenes[3].irs[:, :, :-3])
    scenes[3].ir_len -= 3
    sc = scenes[5]
    sc.clips, sc.specs, sc.starts, sc.irs = sc.clips[:-1], sc.specs[:-1], sc.starts[:-1], np.ascontiguousarray(sc.irs[:, :-1])
    for i in range(1, N_SCENES, 2):
        scenes[i].irs = scenes[i].irs.astype(np.float64)
    return scenes


def driver_jobs(scenes):
    from audiblelight_amd import batch

    return [batch.SceneJob(specs=sc.specs, clips=sc.clips, irs=sc.irs, starts=sc.starts, ends=sc.ends, duration=sc.duration,
                           sample_rate=sc.sr, name=f"s{i}") for i, sc in enumerate(scenes)]


def expected_h2d_bytes(r, jobs, f64_upload):
    """IR bytes as they cross PCIe (float64 tensors: 4 bytes per element when the planner casts them, 8 when the device does)
    plus the packed clips."""
    total = 0
    for job in jobs:
        c, _, l = job.irs.shape
        pl = planning.plan_batch(job.specs, c, l, job.sample_rate, lib=r.lib)
        per = 4 if (job.irs.dtype == np.float32 or f64_upload == "host") else 8
        total += job.irs.size * per + pl.audio_floats * 4
    return total


def run_driver(r, jobs, out_dir, subtype, drv=None, f64_upload="host"):
    """One run with files and callbacks; returns (driver, report, {name: (C, T) array}, {name: WAV payload})."""
    import os

    from scipy.io import wavfile

    from audiblelight_amd import batch

    drv = drv or batch.BatchDriver(r, depth=2, writers=2)
    scenes = {}
    rep = drv.run(jobs, output_dir=str(out_dir), on_scene=scenes.__setitem__, subtype=subtype)
    assert rep.n_scenes == len(jobs) and sorted(scenes) == sorted(j.name for j in jobs)
    assert rep.files == [os.path.join(str(out_dir), f"{j.name}.wav") for j in jobs], rep.files        # job order
    assert rep.h2d_bytes == expected_h2d_bytes(r, jobs, f64_upload), (rep.h2d_bytes, f64_upload)
    wavs = {}
    for job, path in zip(jobs, rep.files):
        sr, wav = wavfile.read(path)
        assert sr == job.sample_rate and wav.dtype == (np.int16 if subtype == "PCM_16" else np.float32)
        wavs[job.name] = wav
    return drv, rep, scenes, wavs


def assert_same_run(scenes, wavs, base_scenes, base_wavs, what):
    for name in base_scenes:
        ke.assert_bits_equal(scenes[name], base_scenes[name], (what, name, "on_scene"))
        ke.assert_bits_equal(wavs[name], base_wavs[name], (what, name, "wav"))


# ----------------------------------------------------------------------------- 6. gaps of the packed audio are never heard
GAP_LAYOUTS = [(layout, 10) for layout in re_.LAYOUTS if re_.layout_ok(layout, 10)] + [("quad", 14), ("split", 11)]


def gap_scene(log2_block, C=2, seed=0):
    """A static event, one moving over three emitters and a dry one; clip lengths 4k + 1, 4k + 2, 4k + 3 (every alignment gap
    of the packed audio is non-empty), several blocks long so that interior and edge windows are both read."""
    B = 1 << log2_block
    rng = np.random.default_rng(4100 + log2_block + seed)
    lens = [4 * int(4.3 * B / 4) + 1, 4 * int(4.9 * B / 4) + 2, 4 * int(3.4 * B / 4) + 3]
    Lir = int(2.3 * B)
    clips = []
    for n in lens:
        a = rng.standard_normal(n).astype(np.float32)
        clips.append(a / np.abs(a).max())
    irs = (rng.standard_normal((C, 4, Lir)) * np.exp(-np.arange(Lir) / (Lir / 5.0))).astype(np.float32)
    specs = [planning.EventSpec(n_samples=lens[0], n_emitters=1, snr=12.0, emitter0=0),
             planning.EventSpec(n_samples=lens[1], n_emitters=3, snr=9.0, emitter0=1, is_moving=True, duration=lens[1] / re_.SR),
             planning.EventSpec(n_samples=lens[2], n_emitters=0, snr=15.0, emitter0=0)]
    pl = planning.plan_batch(specs, C, Lir, re_.SR, log2_block=log2_block)
    return pl, clips, irs


def gap_mask(pl, clips):
    """True for every float of the packed audio outside all clips."""
    outside = np.ones(pl.audio_floats, dtype=bool)
    for off, clip in zip(pl.audio_offsets, clips):
        outside[int(off): int(off) + len(clip)] = False
    return outside


def run_gap_render(r, log2_block, layout, fold):
    """The scene rendered twice through prepare(audio_dev=...): the floats of the packed audio outside every clip zero, then
    the sentinel NaN.  ``spatial`` (every event's rows), ``event_scale``, ``event_stats`` and, with folded clips
    (ClipSource(normalize=True): al_clip_scales reads the clips too), ``clip_scale`` must come out bit for bit the same: no
    kernel output depends on a gap."""
    pl, clips, irs = gap_scene(log2_block)
    outside = gap_mask(pl, clips)
    assert all(int(o) % 4 == 0 for o in pl.audio_offsets) and int(outside.sum()) == 3 + 2 + 1
    sources = [engine.ClipSource(host=c, n=len(c), prescale=p, normalize=True) for c, p in zip(clips, (1.0, -2.0, 0.5))] if fold else clips
    irs_dev, strides = r.upload_irs(irs)
    outs = []
    for fill in (np.float32(0.0), re_.SENTINEL_F32):
        host = np.empty(pl.audio_floats, np.float32)
        host[:] = re_.SENTINEL_F32                      # pack_audio(out=...) writes the clips and nothing else
        r.pack_audio(pl, sources, out=host)
        assert np.array_equal(ke.bits(host[outside]), ke.bits(np.full(int(outside.sum()), re_.SENTINEL_F32)))
        host[outside] = fill
        batch = r.prepare(pl, sources, irs_dev, strides, audio_dev=r.mem.upload(host))
        for desc in batch.descs:
            desc.flags = re_.layout_flags(desc, layout)
        res = batch.run()
        res.check_finite()
        sp = np.asarray(r.mem.download(res.spatial))
        rows = np.concatenate([sp[int(ev["out_off"]): int(ev["out_off"]) + pl.n_capsules * int(ev["len"])] for ev in pl.events])
        out = dict(spatial=rows, event_scale=np.asarray(r.mem.download(res.event_scale))[: len(pl.events)],
                   event_stats=np.asarray(r.mem.download(res.event_stats))[: 4 * len(pl.events)])
        if fold:
            out["clip_scale"] = np.asarray(r.mem.download(batch.bufs["clip_scale"]))[: len(pl.events)]
        assert np.abs(rows).max() > 0
        outs.append(out)
    for key in outs[0]:
        ke.assert_bits_equal(outs[1][key], outs[0][key], ("gaps", layout, log2_block, key))
    return outs[0]


# ----------------------------------------------------------------------------- 7. pack_audio, threaded (host only)
def run_pack_audio_threaded():
    """Five clips of 900 001 .. 900 005 samples (more than 2^22 in total: the thread-pool branch): pack_audio equals a plain
    loop over audio_offsets with zeros elsewhere, and with ``out=`` it writes exactly the clip ranges."""
    rng = np.random.default_rng(77)
    clips = [rng.standard_normal(900_001 + i).astype(np.float32) for i in range(5)]
    assert sum(len(c) for c in clips) >= 1 << 22
    specs = [planning.EventSpec(n_samples=len(c), n_emitters=1, snr=10.0, emitter0=0) for c in clips]
    pl = planning.plan_batch(specs, 1, 1000, 48000)
    want = np.zeros(pl.audio_floats, np.float32)
    inside = np.zeros(pl.audio_floats, dtype=bool)
    for off, c in zip(pl.audio_offsets, clips):
        want[int(off): int(off) + len(c)] = c
        inside[int(off): int(off) + len(c)] = True
    assert inside.sum() == sum(len(c) for c in clips) and not inside.all()       # disjoint ranges, and gaps between them
    r = object.__new__(engine.Renderer)               # pack_audio needs neither a library nor a device
    got = r.pack_audio(pl, clips)
    assert got.dtype == np.float32 and got.shape == want.shape
    ke.assert_bits_equal(got, want, "pack_audio")
    buf = np.full(pl.audio_floats, np.nan, np.float32)
    back = r.pack_audio(pl, clips, out=buf)
    assert back is buf
    assert np.array_equal(np.isnan(buf), ~inside), "pack_audio(out=...) wrote outside the clips, or left part of one unwritten"
    ke.assert_bits_equal(buf[inside], want[inside], "pack_audio(out=)")


# ----------------------------------------------------------------------------- 8. download on both sides of its threshold
def run_download_threshold(mem):
    """2^20 - 1 floats (4 bytes under 4 MiB: ``Tensor.cpu()``) and 2^20 floats (4 MiB: page-locked memory from torch's host
    allocator).  Both equal their source; the larger array stays intact after its device buffer has been overwritten and a
    second large download has been made: the page-locked block belongs to the array."""
    small, large = pattern((1 << 20) - 1, 0x01000000), pattern(1 << 20, 0x02000000)
    d_small, d_large = mem.upload(small), mem.upload(large)
    assert d_small.numel() * 4 == (1 << 22) - 4 and d_large.numel() * 4 == 1 << 22
    got_small, got_large = mem.download(d_small), mem.download(d_large)
    ke.assert_bits_equal(np.asarray(got_small), small, "download below the threshold")
    ke.assert_bits_equal(np.asarray(got_large), large, "download at the threshold")
    other = pattern(1 << 20, 0x03000000)
    d_large.copy_(mem.upload(other))
    got_other = mem.download(d_large)
    ke.assert_bits_equal(np.asarray(got_other), other, "second large download")
    third = mem.download(mem.upload(pattern(1 << 20, 0x04000000)))
    ke.assert_bits_equal(np.asarray(got_large), large, "first large download after two more")
    ke.assert_bits_equal(np.asarray(got_other), other, "second large download after one more")
    assert third.shape == got_large.shape


# ----------------------------------------------------------------------------- 9. AL_TRIM_PARTITIONS, AL_STATIC_MAC_MAX_P
def event_rows(r, res):
    pl = res.plan
    sp = np.asarray(r.mem.download(res.spatial))
    rows = np.concatenate([sp[int(ev["out_off"]): int(ev["out_off"]) + pl.n_capsules * int(ev["len"])] for ev in pl.events])
    return rows, np.asarray(r.mem.download(res.event_scale))[: len(pl.events)]


def run_untrimmed_moving(r, switch):
    """mac_regimes.run_moving_case(r, 10, p_mult=5.002, n_irs=3, k_mult=3.3, expect_moving=612)'s scene (6 partitions against
    clips of 4 blocks, so the planner trims) with AL_TRIM_PARTITIONS=0: no emitter_parts in the descriptor, EVERY IR partition
    transformed, every row at the oracle, and the kept samples bit for bit those of the trimmed render.

    Why bit for bit: k_spectral_mac_moving never reads al_batch.emitter_parts.  It trims on its own (``pl = min(P, K - j_lo)``;
    partitions from ``pl`` on are loaded from partition ``pl - 1`` and scaled by zero) and adds the live partitions in the same
    order either way; the masked ones only feed accumulators of blocks >= K, which are never stored.  The switch changes only
    whether the forward transform computes spectra nobody reads, and the IR energies (emitter gains) are summed by the same
    code on both paths."""
    args = dict(log2_block=10, p_mult=5.002, n_irs=3, k_mult=3.3)
    clips, irs, specs, mic_ir, pl = mr.moving_scene(**args)
    B = pl.block
    switch("AL_TRIM_PARTITIONS", None)
    trimmed = mr.run_moving_case(r, expect_moving=612, **args)          # asserts the trimmed layout, as it always did
    rows_trimmed, scale_trimmed = event_rows(r, trimmed)
    switch("AL_TRIM_PARTITIONS", "0")
    parts = pl.emitter_parts()
    assert parts is not None and parts.min() < pl.n_partitions          # the planner WOULD trim
    batch = r.prepare(pl, clips, mic_ir)
    assert not batch.descs[0].emitter_parts and "emitter_parts" not in batch.bufs
    assert mr.mac_codes(r, batch)[1] == 612
    n_real = pl.hspec_blocks * B * 2
    batch.bufs["hspec"][:n_real] = float("nan")
    res = batch.run()
    res.check_finite()
    h = np.asarray(r.mem.download(batch.bufs["hspec"]))[:n_real]
    assert not np.isnan(h).any(), "a partition was left untransformed with the trimming switched off"
    mr.check_moving_events(res, clips, irs, specs)
    rows, scale = event_rows(r, res)
    ke.assert_bits_equal(rows, rows_trimmed, "untrimmed vs trimmed render")
    ke.assert_bits_equal(scale, scale_trimmed, "untrimmed vs trimmed event_scale")


def run_static_mac_max_p(r, switch, log2_block):
    """The tile_8_12_1-shaped static case (K = 6 blocks, P = 7 partitions): AL_STATIC_MAC_MAX_P=7 keeps the capsule-loop
    accumulate (3120701), 6 sends it to the tile kernel (81201); under both every row meets the oracle.  For ``log2_block`` >= 11:
    at B = 1024 the case's IR (6.0004 blocks) rounds to exactly 6 partitions."""
    name, tile_code, k_mult, p_mult = next(c for c in mr.STATIC_CASES if c[0] == "tile_8_12_1")
    assert tile_code == 81201
    switch("AL_STATIC_MAC_MAX_P", "7")
    mr.run_static_case(r, log2_block, 3120701, k_mult, p_mult)
    switch("AL_STATIC_MAC_MAX_P", "6")
    mr.run_static_case(r, log2_block, tile_code, k_mult, p_mult)
