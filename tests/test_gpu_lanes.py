"""Renderer.prepare(..., lanes=N) and PreparedMix.retarget on the real MI355X (tests/lane_cases.py; the descriptor half also
runs under host emulation in tests/test_hostemu_kernels.py).

A multi-lane batch enqueues chunk i on HIP stream i % N over that lane's own H / X / Y workspaces and joins every lane back
into the current stream.  The scenes are the smallest at which the chunks' kernels still overlap in time (32 capsules, 4800-tap
IRs, 9600-sample clips, six events: one chunk each).  The comparison is bit for bit with the single-lane, single-chunk render,
and the mixdown is enqueued on the current stream straight behind run() with no synchronisation in between, so a lane that was
not joined would be read while it is still being written.  A pass makes such a race unlikely, not impossible: the GPU may
happen to run the racing kernels in the right order."""
import numpy as np
import pytest

from audiblelight_amd import plan as planning, synthetic
from tests import lane_cases as lc

pytestmark = pytest.mark.gpu

E = 6


@pytest.fixture(scope="module")
def gpu():
    from audiblelight_amd import engine

    r = engine.Renderer()
    assert r.lib.path.endswith("libaudiblelight_hip.so")
    return r


def _scene(kind):
    """(clips, irs, specs, starts, sr, duration, C) of six events: static (one IR each), moving (four IRs each) or alternating."""
    if kind == "static":
        sc = synthetic.make_scene("cfg2", scale=0.05, E=E)
        return sc.clips, sc.irs, sc.specs, sc.starts, sc.sr, sc.duration, sc.n_capsules
    sc = synthetic.make_scene("cfg2", scale=0.05, E=E, N=4)
    if kind == "moving":
        assert all(sp.is_moving and sp.n_emitters == 4 for sp in sc.specs)
        return sc.clips, sc.irs, sc.specs, sc.starts, sc.sr, sc.duration, sc.n_capsules
    cols, specs = [], []
    for e, sp in enumerate(sc.specs):       # events 0, 2, 4 keep their four IRs, events 1, 3, 5 become static on their first
        n_ir = 4 if e % 2 == 0 else 1
        specs.append(planning.EventSpec(n_samples=sp.n_samples, n_emitters=n_ir, snr=sp.snr, emitter0=len(cols), is_moving=n_ir > 1,
                                        duration=sp.duration, ref_db=sp.ref_db))
        cols += list(range(4 * e, 4 * e + n_ir))
    return sc.clips, np.ascontiguousarray(sc.irs[:, cols, :]), specs, sc.starts, sc.sr, sc.duration, sc.n_capsules


@pytest.fixture(scope="module", params=["static", "moving", "mixed"])
def rendered(gpu, request):
    """The scene, its plans and the single-lane, single-chunk render and mixdown every lane count is compared with (computed
    once per scene, left unchanged)."""
    clips, irs, specs, starts, sr, duration, C = _scene(request.param)
    pl = planning.plan_batch(specs, C, irs.shape[2], sr, lib=gpu.lib)
    ends = [s + len(c) / sr for s, c in zip(starts, clips)]
    mp = planning.plan_mixdown(starts, ends, [len(c) for c in clips], [C] * E, pl.events["out_off"], list(range(E)), duration, sr, C,
                               lib=gpu.lib)
    irs_dev, strides = gpu.upload_irs(irs)
    one = gpu.prepare(pl, clips, irs_dev, ir_strides=strides)
    assert one.lanes == 1 and len(one.descs) == 1
    res = one.run()
    assert res.keep == ()                       # a single-lane result does not pin the batch
    scene = np.asarray(gpu.mem.download(gpu.prepare_mixdown(mp, res).run()))[: C * mp.n_samples].copy()
    want = lc.render_bits(res)
    assert np.all(np.isfinite(want[0])) and np.abs(scene).max() > 0 and not want[2].reshape(-1, 4)[:, 2].any()
    return dict(kind=request.param, pl=pl, mp=mp, clips=clips, irs=(irs_dev, strides), want=want, scene=scene, n=C * mp.n_samples)


def _prepare(gpu, rd, **kw):
    return gpu.prepare(rd["pl"], rd["clips"], rd["irs"][0], ir_strides=rd["irs"][1], **kw)


@pytest.mark.parametrize("lanes", [2, 3, 8])
def test_lanes_give_the_single_lane_bits(gpu, rendered, lanes):
    """Two runs of one multi-lane batch (the second over the lanes' used streams and dirty workspaces), each followed at once,
    without a synchronisation, by the mixdown on the current stream: render and scene equal the single-lane ones bit for bit.
    lanes = 8 is more than there are chunks and is clamped to six.  (See the module docstring: a pass makes a missing join
    unlikely, not impossible.)"""
    batch = _prepare(gpu, rendered, chunk_events=1, lanes=lanes)
    lc.check_lane_descriptors(batch, min(lanes, E), n_chunks=E)
    for turn in range(2):
        res = batch.run()
        scene_dev = gpu.prepare_mixdown(rendered["mp"], res).run()        # current stream, straight behind the joins
        assert res.keep == (batch,)                                        # side streams: the result keeps the batch alive
        scene = np.asarray(gpu.mem.download(scene_dev))[: rendered["n"]]
        lc.assert_bits_equal(scene, rendered["scene"], (rendered["kind"], lanes, "scene", turn))
        lc.assert_same_render(lc.render_bits(res), rendered["want"], (rendered["kind"], lanes, turn))
    assert len(batch._streams) == min(lanes, E)
    lc.check_spill_blocks(batch)


def test_staged_run_of_a_multi_lane_batch_takes_one_stream(gpu, rendered):
    batch = _prepare(gpu, rendered, chunk_events=1, lanes=3)
    res = batch.run(stages=list(batch.STAGES))
    assert batch._streams is None                                          # no side stream was made
    lc.assert_same_render(lc.render_bits(res), rendered["want"], (rendered["kind"], "staged"))
    scene = np.asarray(gpu.mem.download(gpu.prepare_mixdown(rendered["mp"], res).run()))[: rendered["n"]]
    lc.assert_bits_equal(scene, rendered["scene"], (rendered["kind"], "staged scene"))


def test_graph_capture_refuses_a_multi_lane_batch(gpu, rendered):
    from audiblelight_amd import engine

    batch = _prepare(gpu, rendered, chunk_events=2, lanes=2)
    assert batch.lanes == 2
    with pytest.raises(ValueError, match="capture a single-lane batch"):
        engine.CapturedScene(batch)


@pytest.mark.parametrize("form", ["overwrite", "fused ambience", "accumulate"])
def test_retargeted_mixdown_writes_the_same_bits_elsewhere(gpu, rendered, form):
    mp = rendered["mp"]
    res = _prepare(gpu, rendered).run()
    rng = np.random.default_rng(8)
    ambience = [(gpu.mem.upload(rng.standard_normal(rendered["n"]).astype(np.float32)),
                 gpu.mem.upload(rng.uniform(0.01, 0.1, mp.n_capsules).astype(np.float32)))] if form == "fused ambience" else []
    prefill = rng.uniform(-1, 1, rendered["n"]).astype(np.float32) if form == "accumulate" else None
    got = lc.run_retarget(gpu, mp, res, ambience, prefill)
    if form == "overwrite":
        lc.assert_bits_equal(got, rendered["scene"], "the retargeted scene")
