"""Scenarios for two paths only the benchmark drives: Renderer.prepare(..., lanes=N) (chunk i on workspace / HIP stream
i % N, joined into the current stream) and PreparedMix.retarget (the mixdown descriptor copied by value with another scene
pointer).  Shared by tests/test_hostemu_kernels.py and tests/test_gpu_lanes.py.

Host emulation runs the lane descriptors in order on one "stream": it checks the descriptor tables and that the chunks over
alternating workspaces give the one-chunk bits, and cannot see two lanes sharing a workspace (the descriptor assertions stand
for that).  The streams, their joins and the overlap of chunks exist only on the GPU."""
import ctypes as ct

import numpy as np

from audiblelight_amd import _hip
from tests.kernel_edges import Guarded, assert_bits_equal

LANE_OWNED = ("hspec", "xspec", "yspec")
POINTERS = [name for name, kind in _hip.AlBatch._fields_ if kind is ct.c_void_p]


def check_lane_descriptors(batch, lanes, n_chunks):
    """The descriptors of a multi-lane batch: H / X / Y workspaces in the pattern i % lanes over exactly `lanes` distinct
    buffers (lane 0: the batch's own, lane k: bufs["_lanes"][k - 1]), every other pointer shared, each lane's all-zero spill block
    behind H and X in place."""
    mem, bufs = batch.renderer.mem, batch.bufs
    assert batch.lanes == lanes and len(batch.descs) == n_chunks and len(bufs["_lanes"]) == lanes - 1
    owners = [bufs] + list(bufs["_lanes"])
    for name in LANE_OWNED:
        lane_ptr = [mem.ptr(ws[name]) for ws in owners]
        assert len(set(lane_ptr)) == lanes and all(lane_ptr), (name, lane_ptr)
        assert [getattr(d, name) for d in batch.descs] == [lane_ptr[i % lanes] for i in range(n_chunks)], name
    for name in POINTERS:
        if name not in LANE_OWNED:
            assert len({getattr(d, name) for d in batch.descs}) == 1, f"{name} differs between the chunks"
    for name in ("spatial", "event_scale", "event_stats", "emitter_gain", "ir_energy", "partials"):
        assert getattr(batch.descs[0], name) == mem.ptr(bufs[name]), name
    # workspaces of different lanes do not overlap
    spans = sorted((mem.ptr(ws[name]), mem.ptr(ws[name]) + 4 * len(ws[name])) for ws in owners for name in LANE_OWNED)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans
    check_spill_blocks(batch)


def check_spill_blocks(batch):
    """One block of zeros behind every lane's H and X workspace, at the index the descriptors name."""
    mem, two_b = batch.renderer.mem, 2 * batch.plan.block
    d = batch.descs[0]
    for ws in [batch.bufs] + list(batch.bufs["_lanes"]):
        for name, at in (("hspec", d.hspec_zero_block), ("xspec", d.xspec_zero_block)):
            flat = np.asarray(mem.download(ws[name]))
            assert len(flat) == (at + 1) * two_b, (name, len(flat), at)
            assert not flat[at * two_b:].view(np.uint32).any(), f"the spill block behind {name} is not zero"


def render_bits(res):
    """Everything a render leaves behind, as host arrays: the whole spatial buffer, the event scales and statistics."""
    mem, n_ev = res.memory, len(res.plan.events)
    return (np.asarray(mem.download(res.spatial))[: res.plan.spatial_floats].copy(), np.asarray(mem.download(res.event_scale))[:n_ev].copy(),
            np.asarray(mem.download(res.event_stats))[: 4 * n_ev].copy())


def assert_same_render(got, want, what):
    for g, w, name in zip(got, want, ("spatial", "event_scale", "event_stats")):
        assert_bits_equal(g, w, (what, name))


def interior(g):
    """The interior of a guarded float32 buffer as a buffer of the memory provider's own type (its pointer is g.ptr)."""
    piece = g.buf[g.lo:g.hi]
    view = piece.view(g.r.mem.torch.float32) if hasattr(g.r.mem, "torch") else piece.view(np.float32)
    assert g.r.mem.ptr(view) == g.ptr
    return view


def run_retarget(r, mix_plan, result, ambience=(), prefill=None):
    """mix.retarget(buf2).run() writes into buf2 the bits mix.run() writes into its own buffer, leaves that buffer's bytes
    alone, and leaves the original descriptor's scene pointer where it was.  ``ambience``: one (noise, multipliers) pair is fused
    into the mixdown kernel.  ``prefill``: both buffers start from it and the mixdown accumulates
    (prepare_mixdown(..., scene=...)); a retargeted run that still wrote to the first buffer would add the events twice."""
    n = mix_plan.n_capsules * mix_plan.n_samples
    junk = np.random.default_rng(2).uniform(-1, 1, n).astype(np.float32)
    first = Guarded(r, n, init=junk if prefill is None else prefill)
    if prefill is None:
        base = r.prepare_mixdown(mix_plan, result, list(ambience))
        assert base.desc.accumulate == 0 and bool(base.desc.ambience) == bool(ambience)
        own = np.asarray(r.mem.download(base.run()))[:n].copy()       # the buffer prepare_mixdown made itself
        mix = base.retarget(interior(first))          # ... and from here on guarded buffers on both sides
    else:
        mix = r.prepare_mixdown(mix_plan, result, list(ambience), scene=interior(first))
        assert mix.desc.accumulate == 1
    assert mix.desc.scene == first.ptr
    mix.run()
    want = first.get()
    assert np.all(np.isfinite(want)) and np.abs(want).max() > 0
    if prefill is not None:
        assert not np.array_equal(want, prefill)
    else:
        assert_bits_equal(want, own, "retargeted from the buffer prepare_mixdown made")
    second = Guarded(r, n, init=junk[::-1] if prefill is None else prefill)
    twin = mix.retarget(interior(second))
    assert twin is not mix and twin.desc is not mix.desc
    assert twin.desc.scene == second.ptr and mix.desc.scene == first.ptr
    for name, _ in _hip.AlMix._fields_:
        if name != "scene":
            assert getattr(twin.desc, name) == getattr(mix.desc, name), name
    out = twin.run()
    assert r.mem.ptr(out) == second.ptr
    assert_bits_equal(second.get(), want, "the retargeted mixdown")
    assert_bits_equal(first.get(), want, "the original buffer after the retargeted run")
    assert mix.desc.scene == first.ptr
    mix.run()                                          # the original still writes where it did
    if prefill is None:
        assert_bits_equal(first.get(), want, "the original mixdown run again")
    else:
        assert not np.array_equal(first.get(), want)   # accumulated once more, into its own buffer
    assert_bits_equal(second.get(), want, "the retargeted buffer after the original ran again")
    if prefill is None:
        assert base.desc.scene == r.mem.ptr(base.scene)
        assert_bits_equal(np.asarray(r.mem.download(base.scene))[:n], own, "the buffer prepare_mixdown made, after every retargeted run")
    return want
