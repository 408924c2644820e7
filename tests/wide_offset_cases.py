"""Small work at a huge address: every offset, stride, block base and row base the C ABI carries as 64 bits (or as a 32-bit block
index that the kernels widen before they multiply) put next to element 2^31, element 2^32 and byte 2^32 of a buffer that really
is that large.  An index overflow depends on where the data lies, not on how much of it there is, so each case renders the
smallest problem that launches the kernel; the buffers are allocated UNTOUCHED (torch.empty on the device, np.empty under host
emulation) and only the pages a case uses are ever written.

Shared by tests/test_hostemu_wide_offsets.py (the host-emulated kernels, which compile the same index expressions: sections A, B
and C; of the scene row bases of B and of section C, which are real passes over 2^31 floats and take minutes under emulation, one
case each) and tests/test_gpu_wide_offsets.py (gfx950 build: A, B, C and section D, real passes over 2^31 + 3077 elements).

Every offset case is checked twice:
  1. bit for bit against the same inputs through the same library with every offset small.  The two runs differ by multiples of
     1024 floats in every offset, so each alignment predicate of the kernels (the pair parity of the synthesis stores, the 16-byte
     arms, the float4 runs of the mixdown) takes the same branch in both;
  2. against the float64 bound of the module the case comes from, on the high-offset output itself: render_edges.check_render with
     render_bound, render_edges.mixdown64 with gamma, shoebox_cases.assert_within_bound.  No tolerance is introduced here.
Sentinel guard bands of kernel_edges.G floats lie on both sides of every output block at its high position.

Positions (POSITIONS): "i31" straddles element 2^31 of the type the kernel indexes the buffer with (float, or float2 for the
spectra), "i32" element 2^32, "b32" byte offset 2^32.  The spectra workspaces are left out at "i32": 2^32 float2 are 32 GiB for one
buffer, and a case holds at most 40 GiB.

Left out on purpose: the one-workgroup scans with n past 2^31 (al_fx_sos, the de-emphasis op of al_fx_apply, al_fx_delay,
al_fx_chorus, al_fx_phaser, al_fx_compressor, al_fx_limiter, al_fx_time_stretch).  A clip of 2^31 samples is twelve hours of audio
at 48 kHz, and a serial scan over it is no test of a few seconds.
"""
import ctypes as ct

import numpy as np
import pytest

from audiblelight_amd import _hip, engine
from audiblelight_amd import plan as planning
from tests import render_edges as rd
from tests import shoebox_cases as sb
from tests.kernel_edges import G, SENTINEL, assert_bits_equal, bits, record, ulps

POSITIONS = {"i31": 1 << 31, "i32": 1 << 32, "b32": 1 << 30}      # element indices of a float buffer
SPECTRA_POSITIONS = {"i31": 1 << 31, "b32": 1 << 29}              # element indices of a float2 buffer
SENTINEL_U32 = int(np.resize(SENTINEL, 4).view(np.uint32)[0])
CAP_BYTES = 40 << 30                                              # the most device memory one case may hold


# ----------------------------------------------------------------------------- memory
def reserve(r, n, dtype=np.float32):
    """An UNTOUCHED buffer of n elements.  On the device: skipped unless 1.25x the case's need is free (``need`` below)."""
    return r.mem.empty(int(n), dtype)


def need(r, nbytes):
    """Skip -- a condition of the shared machine, not a pass -- unless 1.25x the bytes the case is about to hold are free."""
    nbytes = int(nbytes)
    assert nbytes <= CAP_BYTES, f"a case may hold at most {CAP_BYTES} bytes, this one wants {nbytes}"
    if hasattr(r.mem, "free_bytes"):
        free = r.mem.free_bytes()
        if free < 1.25 * nbytes:
            pytest.skip(f"needs {nbytes} bytes of device memory with 1.25x that free; {free} bytes are free")


def release(r):
    """Hand back what the case no longer refers to (the runners call this after every test, too)."""
    import gc

    gc.collect()
    if hasattr(r.mem, "torch"):
        r.mem.torch.cuda.empty_cache()


def fill_u32(buf, lo, hi, value):
    """buf[lo:hi] (float32 elements) := the 32-bit pattern ``value``, on either memory provider."""
    if isinstance(buf, np.ndarray):
        buf[lo:hi].view(np.uint32)[:] = value
    else:
        import torch

        buf[lo:hi].view(torch.int32).fill_(value - (1 << 32) if value >= 1 << 31 else value)


def fill_sentinel(buf, lo, hi):
    fill_u32(buf, lo, hi, SENTINEL_U32)


def assert_sentinel(r, buf, lo, hi, what):
    got = bits(rd.download(r, buf[lo:hi]))
    bad = np.flatnonzero(got != SENTINEL_U32)
    assert bad.size == 0, f"{what}: {bad.size} guard floats overwritten (first at {lo + int(bad[0])})"


# ----------------------------------------------------------------------------- A. render stage
def scene(log2_block, P, C=2, kinds=("static", "moving", "dry"), k_blocks=2.3, seed=0):
    """Random clips and flat random IRs (render_edges.flat_scene's kind of scene with fixed lengths): the static clip comes
    first and spans ``k_blocks`` blocks, so that its output block, its clip and its spectra are long enough to straddle a
    position; the moving event cross-fades over 3 emitters; the dry one is tiled over the capsules."""
    B = 1 << log2_block
    rng = np.random.default_rng(8100 + 17 * log2_block + P + seed)
    Lir = P * B - 37
    specs, clips, col = [], [], 0
    for kind in kinds:
        if kind == "moving":
            n = max(int(2.6 * B), 700)
            specs.append(planning.EventSpec(n_samples=n, n_emitters=3, snr=12.0, emitter0=col, is_moving=True, duration=n / rd.SR))
            col += 3
        else:
            n = int(k_blocks * B) + 17 if kind == "static" else B + 301
            specs.append(planning.EventSpec(n_samples=n, n_emitters=1 if kind == "static" else 0, snr=9.0, emitter0=col))
            col += 1 if kind == "static" else 0
        clips.append(rng.uniform(-1, 1, n).astype(np.float32))
    h = rng.uniform(-1, 1, (C, max(col, 1), Lir)).astype(np.float32)
    return dict(specs=specs, clips=clips, h=h, Lir=Lir, C=C, log2_block=log2_block, P=P)


SEPARATE = ("al_ir_spectra", "al_signal_spectra", "al_emitter_gains", "al_spectral_mac", "al_block_synthesis", "al_event_levels")


def render(r, sc, layout="plain", spatial=0, audio=0, ir_strides=None, xshift=0, yshift=0, pshift=0, block0=False, stages=None,
           flags=0, family="wide"):
    """One batch with its data at the given places, rendered and checked against render_edges' float64 restatement.

    spatial, audio: floats by which every al_event.out_off / audio_off moves.  ir_strides = (ir_stride_c, ir_stride_n): the IR rows
    laid out with those strides in a device buffer (None: the host tensor, uploaded as it is).  xshift / yshift: blocks added to
    every al_stream.xspec_base / al_event.yspec_base; pshift: entries added to every part_base.  block0: the shifted bases stay in
    the tables but al_batch.xspec_block0 / yspec_block0 bring them back to small indices, in workspaces of the usual size.
    Returns what the bit comparison needs: every event's raw (C, len) block, its partial statistics, the event scales and
    statistics, the accumulate codes, and the batch."""
    specs, clips, h, Lir, C, lb = sc["specs"], sc["clips"], sc["h"], sc["Lir"], sc["C"], sc["log2_block"]
    mem = r.mem
    pl = rd.make_plan(specs, C, Lir, lb, guards=True, odd=True, base=spatial)
    B = pl.block
    blocks_bytes = 8 * B
    high_spectra = 0 if block0 else ((yshift + pl.yspec_blocks) * blocks_bytes if yshift else 0) + \
        ((xshift + pl.xspec_blocks + 1) * blocks_bytes if xshift else 0)
    ir_floats = 0
    if ir_strides is not None:
        pitch = -(-Lir // 1024) * 1024
        ir_floats = (C - 1) * ir_strides[0] + (h.shape[1] - 1) * ir_strides[1] + pitch
    need(r, 4 * (pl.spatial_floats + audio + pl.audio_floats + ir_floats + 4 * (pl.n_partials + pshift)) + high_spectra + pl.workspace_bytes())

    packed = r.pack_audio(pl, [engine.as_clip_source(c) for c in clips])      # the clips at the planner's (small) offsets
    audio_dev = reserve(r, audio + pl.audio_floats)
    rd.put(r, audio_dev[audio:], packed)
    pl.events["audio_off"] += audio
    pl.events["yspec_base"] += yshift
    pl.events["part_base"] += pshift
    pl.n_partials += pshift
    if len(pl.streams):
        pl.streams["xspec_base"] += xshift

    if ir_strides is None:
        batch = r.prepare(pl, clips, h, audio_dev=audio_dev)
    else:
        ir_dev = reserve(r, ir_floats)
        for c in range(C):
            for n in range(h.shape[1]):
                rd.put(r, ir_dev[c * ir_strides[0] + n * ir_strides[1]:], np.pad(h[c, n], (0, pitch - Lir)))
        batch = r.prepare(pl, clips, ir_dev, ir_strides=tuple(int(s) for s in ir_strides), audio_dev=audio_dev)
    assert len(batch.descs) == 1
    desc = batch.descs[0]
    desc.flags = rd.layout_flags(desc, layout) | flags
    if block0:
        desc.xspec_block0, desc.yspec_block0 = xshift, yshift
    else:
        if yshift:
            batch.bufs["yspec"] = reserve(r, (yshift + pl.yspec_blocks) * 2 * B)
            desc.yspec = mem.ptr(batch.bufs["yspec"])
        if xshift:
            x = batch.bufs["xspec"] = reserve(r, (xshift + pl.xspec_blocks + 1) * 2 * B)
            x[(xshift + pl.xspec_blocks) * 2 * B:] = 0
            desc.xspec, desc.xspec_zero_block = mem.ptr(x), xshift + pl.xspec_blocks
    rd.sentinel_spatial(r, batch)
    code = ct.c_int32(-1), ct.c_int32(-1)
    r.lib.call("al_spectral_mac_variant", ct.byref(desc), ct.byref(code[0]), ct.byref(code[1]))
    batch.run(stages=stages)
    res, outs = rd.check_render(r, batch, clips, h, family)
    parts = [rd.download(r, batch.bufs["partials"][4 * int(ev["part_base"]): 4 * (int(ev["part_base"]) + C * int(ev["n_blocks"]))])
             for ev in pl.events]
    return dict(outs=outs, partials=parts, scales=rd.download(r, batch.bufs["event_scale"], len(specs)), stats=res.stats(),
                codes=(code[0].value, code[1].value), res=res, batch=batch, plan=pl)


def assert_same_render(high, low, what):
    """The high-offset run against its low-offset twin: every output the stages leave behind, bit for bit."""
    assert high["codes"] == low["codes"], (what, high["codes"], low["codes"])
    for i, (a, b) in enumerate(zip(high["outs"], low["outs"])):
        assert_bits_equal(a, b, (what, "spatial of event", i))
    for i, (a, b) in enumerate(zip(high["partials"], low["partials"])):
        assert_bits_equal(a, b, (what, "partials of event", i))
    assert_bits_equal(high["scales"], low["scales"], (what, "event_scale"))
    assert_bits_equal(high["stats"], low["stats"], (what, "event_stats"))


def straddles(lo, n, position):
    return lo < position < lo + n


def run_spatial(r, log2_block, layout, position, P=2):
    """al_event.out_off: the first (static) event's (C, len) block straddles the position, the moving and the dry one lie past it."""
    sc = scene(log2_block, P)
    shift = POSITIONS[position] - 1024
    high = render(r, sc, layout, spatial=shift, family=f"wide spatial {position}")
    ev = high["plan"].events[0]
    assert straddles(int(ev["out_off"]), sc["C"] * int(ev["len"]), POSITIONS[position])
    low = render(r, sc, layout, family="wide spatial low")
    assert_same_render(high, low, ("spatial", log2_block, layout, position))
    return high


def run_audio(r, log2_block, layout, position, P=2):
    """al_event.audio_off: the clips lie in a device buffer of that size, the first one across the position."""
    sc = scene(log2_block, P)
    shift = POSITIONS[position] - 1024
    high = render(r, sc, layout, audio=shift, family=f"wide audio {position}")
    ev = high["plan"].events[0]
    assert straddles(int(ev["audio_off"]), int(ev["len"]), POSITIONS[position])
    low = render(r, sc, layout, family="wide audio low")
    assert_same_render(high, low, ("audio", log2_block, layout, position))


def run_ir_strides(r, log2_block, layout, which, fused, P=2):
    """ir_stride_n (two emitters) or ir_stride_c (two capsules) just above 2^31, through al_forward_spectra (``fused``) or
    al_ir_spectra + al_signal_spectra.  The rows are 1024-float aligned in both runs and the strides differ by exactly 2^31."""
    kinds = ("static", "static") if which == "n" else ("static", "moving", "dry")
    sc = scene(log2_block, P, kinds=kinds)
    C, N, Lir = sc["h"].shape
    pitch = -(-Lir // 1024) * 1024
    small = (pitch, C * pitch) if which == "n" else (N * pitch, pitch)
    wide = (small[0], small[1] + (1 << 31)) if which == "n" else (small[0] + (1 << 31), small[1])
    stages = None if fused else SEPARATE
    high = render(r, sc, layout, ir_strides=wide, stages=stages, family=f"wide ir_stride_{which}")
    low = render(r, sc, layout, ir_strides=small, stages=stages, family="wide ir stride low")
    assert_same_render(high, low, ("ir_stride_" + which, log2_block, layout, fused))


def spectra_shift(position, B):
    """Blocks to add so that block 1 of the first event / stream starts exactly at float2 element ``position``."""
    return SPECTRA_POSITIONS[position] // B - 1


def run_spectra_bases(r, log2_block, layout, position, P=2):
    """xspec_base, yspec_base and part_base moved so that (base + c n_blocks + k) B crosses the position as a float2 index (the
    partials: 4 (part_base + ...) as a float index), with xspec_block0 = yspec_block0 = 0; once more with block0 values that bring
    the same table entries back to small indices; both against the unshifted batch."""
    sc = scene(log2_block, P)
    B = 1 << log2_block
    shift = spectra_shift(position, B)
    pshift = (POSITIONS["i31" if position == "i31" else "b32"] >> 2) - 2
    family = f"wide spectra {position}"
    low = render(r, sc, layout, pshift=254, family="wide spectra low")      # 254 + 2^k - 256: the entries move by whole KiB
    high = render(r, sc, layout, xshift=shift, yshift=shift, pshift=254, family=family)
    ev = high["plan"].events[0]
    assert straddles(int(ev["yspec_base"]) * B, sc["C"] * int(ev["n_blocks"]) * B, SPECTRA_POSITIONS[position])
    assert straddles(int(high["plan"].streams[0]["xspec_base"]) * B, int(high["plan"].streams[0]["n_j"]) * B, SPECTRA_POSITIONS[position])
    assert_same_render(high, low, ("spectra bases", log2_block, layout, position))
    del high, ev
    release(r)
    rebased = render(r, sc, layout, xshift=shift, yshift=shift, pshift=254, block0=True, family=family + " block0")
    assert_same_render(rebased, low, ("spectra bases through block0", log2_block, layout, position))
    del rebased
    release(r)
    high = render(r, sc, layout, pshift=pshift, family=family + " partials")      # a pass of its own: 40 GiB hold either, not both
    ev = high["plan"].events[0]
    assert straddles(4 * int(ev["part_base"]), 4 * sc["C"] * int(ev["n_blocks"]), 4 * (pshift + 2))
    assert_same_render(high, low, ("part_base", log2_block, layout, position))


# (name, kinds, clip blocks, partitions, flags, static code, moving code): one batch per accumulate kernel, at B = 1024
MAC_CASES = [
    ("static", ("static",), 2.3, 3, 0, 3120301, 0),                                      # k_spectral_mac_static<12,3,1>
    ("static_lds", ("static",), 26.3, 2, 0, 3120203, 0),                                 # k_spectral_mac_static_lds<12,2>
    ("static_glds", ("static",), 13.4, 2, _hip.FLAG_MAC_LDS_DMA, 3120204, 0),            # k_spectral_mac_static_glds
    ("tile", ("static",), 2.3, 22, 0, 81201, 0),                                         # k_spectral_mac<8,12,1>: P > 21
    ("moving", ("moving",), 2.3, 3, 0, None, 612),                                       # k_spectral_mac_moving
]


def run_mac_regime(r, name, position="i31", log2_block=10):
    """Each accumulate kernel once with xspec and yspec at the high position; the code al_spectral_mac_variant reports is asserted."""
    _, kinds, k_blocks, P, flags, static_code, moving_code = next(c for c in MAC_CASES if c[0] == name)
    sc = scene(log2_block, P, kinds=kinds * 2, k_blocks=k_blocks, seed=len(name))     # the first event across the position, the second past it
    shift = spectra_shift(position, 1 << log2_block)
    high = render(r, sc, xshift=shift, yshift=shift, flags=flags, family=f"wide mac {name}")
    if static_code is not None:
        assert high["codes"][0] == static_code, high["codes"]
    assert high["codes"][1] == moving_code, high["codes"]
    low = render(r, sc, flags=flags, family="wide mac low")
    assert_same_render(high, low, ("accumulate", name, position))


def run_python_layer(r, position="i31", log2_block=10):
    """RenderResult.raw_spatial, spatial_audio and scaled_copy on a result whose events lie past the position: the arrays of the
    same render at low offsets.  (The dry render's lazy fetch: run_dry_fetch.)"""
    sc = scene(log2_block, 2)
    high = render(r, sc, spatial=POSITIONS[position] - 1024, family="wide python layer")
    low = render(r, sc, family="wide python layer low")
    C = sc["C"]
    for i in range(len(sc["specs"])):
        a, b = high["res"], low["res"]
        assert_bits_equal(a.raw_spatial(i), b.raw_spatial(i), ("raw_spatial", i))
        assert_bits_equal(a.raw_spatial(i), high["outs"][i], ("raw_spatial against the checked block", i))
        assert_bits_equal(a.spatial_audio(i, dtype=np.float32), b.spatial_audio(i, dtype=np.float32), ("spatial_audio", i))
        want = (high["outs"][i].astype(np.float64) * float(high["scales"][i])).astype(np.float32)   # one float32 product
        np.testing.assert_array_equal(a.spatial_audio(i, dtype=np.float32), want)
        n = C * int(a.plan.events[i]["len"])
        ptrs = [r.mem.ptr(a.event_scale) + 4 * i], [r.mem.ptr(a.event_stats) + 8 * (4 * i + 3)]
        ptrs_low = [r.mem.ptr(b.event_scale) + 4 * i], [r.mem.ptr(b.event_stats) + 8 * (4 * i + 3)]
        got = rd.download(r, a.scaled_copy(int(a.plan.events[i]["out_off"]), n, *ptrs), n)
        assert_bits_equal(got, rd.download(r, b.scaled_copy(int(b.plan.events[i]["out_off"]), n, *ptrs_low), n), ("scaled_copy", i))
    rd.check_guards(r, high["batch"])       # scaled_copy works on a copy: the render and its guards are as they were


def run_hspec_real_size(r):
    """hspec is indexed from emitter0 and cannot be moved: one batch of real size, B = 16384, 26 partitions, 64 capsules and 80
    emitters (2.18e9 float2, 16.3 GiB; 40 emitters, 1.09e9 float2, stay below float2 index 2^31, which is what the kernels index
    hspec with), IRs drawn on the device.  One event on emitter 0 and one on the LAST emitter, so that the chunk spans all 80 IR
    columns and the last event's spectra start past float2 element 2^31; both against render64 from their own emitter's rows."""
    lb, P, C, N = 14, 26, 64, 80
    B = 1 << lb
    Lir = P * B
    assert (N - 1) * C * P * B > 1 << 31                 # the last emitter's first spectrum block, as a float2 index
    n = B + 77
    specs = [planning.EventSpec(n_samples=n, n_emitters=1, snr=9.0, emitter0=e) for e in (0, N - 1)]
    clips = [np.random.default_rng(5 + i).uniform(-1, 1, n).astype(np.float32) for i in range(2)]
    pl = rd.make_plan(specs, C, Lir, lb, guards=True, odd=True)
    assert pl.n_emitters == N
    need(r, 4 * C * N * Lir + pl.workspace_bytes() + 4 * pl.spatial_floats)
    ir_dev = reserve(r, C * N * Lir)
    r.lib.call("al_normal_fill", r.mem.ptr(ir_dev), C * N * Lir, 1234, 7, 1.0, r.mem.stream())
    batch = r.prepare(pl, clips, ir_dev, ir_strides=(N * Lir, Lir))
    desc = batch.descs[0]
    assert len(batch.descs) == 1 and (desc.emitter0, desc.n_emitters) == (0, N), (desc.emitter0, desc.n_emitters)
    hspec = batch.bufs["hspec"]
    floats = int(hspec.numel()) if hasattr(hspec, "numel") else int(hspec.size)
    assert floats == (N * C * P + 1) * 2 * B and floats * 4 > 16 << 30, floats        # the whole tensor's spectra + the zero block
    assert int(pl.streams[1]["emitter"]) == N - 1
    desc.flags = rd.layout_flags(desc, "quad")
    rd.sentinel_spatial(r, batch)
    batch.run()
    # render64 reads irs[c, emitter]: a host tensor that holds the two emitters' rows at their own columns, zeros elsewhere
    h = np.zeros((C, N, Lir), np.float32)
    for e in (0, N - 1):
        for c in range(C):
            h[c, e] = rd.download(r, ir_dev[(c * N + e) * Lir: (c * N + e + 1) * Lir])
    rd.check_render(r, batch, clips, h, "wide hspec real size")


# ----------------------------------------------------------------------------- B. mixdown
def mix_desc(r, tabs, C, T, accumulate, spatial, scales, scene_ptr, amb=None, amb_scale=None):
    dev = {k: r.mem.upload(v) for k, v in tabs.items() if k != "n_tiles"}
    p = r.mem.ptr
    desc = _hip.AlMix(n_capsules=C, n_samples=T, tile=4096, n_tiles=tabs["n_tiles"], accumulate=1 if accumulate else 0,
                      tile_ptr=p(dev["tile_ptr"]), tile_events=p(dev["tile_events"]), slot_src=p(dev["slot_src"]),
                      slot_len=p(dev["slot_len"]), slot_start=p(dev["slot_start"]), slot_count=p(dev["slot_count"]),
                      slot_rows=p(dev["slot_rows"]), slot_event=p(dev["slot_event"]), spatial=p(spatial), event_scale=p(scales),
                      scene=scene_ptr, ambience=p(amb) if amb is not None else None,
                      ambience_scale=p(amb_scale) if amb_scale is not None else None)
    return desc, dev


def mix_slots(C, T, L, offs, n_ev, rows=None):
    """Slots at 0, around the tile seams, ending at T and running past it, at odd sources: a small cut of run_mixdown_slots."""
    case = rd.MixCase(C, T)
    starts = [0, 37, T - L, T - L // 2, T - 1] + [s + d for s in range(4096, min(T, 3 * 4096), 4096) for d in (-3, 1, 2)]
    for q, s in enumerate(x for x in starts if 0 <= x < T):
        count = min(L if q % 3 else L - 17, T - s + (5 if q % 4 == 0 else 0))
        case.add(offs[q % n_ev] + (q % 3), L - 3, s, max(min(count, L - 3), 0), C if rows is None else rows, q % n_ev)
    return case


def check_mix(got, tabs, C, T, window, base, scales, prefill, amb, amb_scale, family):
    """render_edges.run_mixdown's bound: |err| <= gamma_(adds + 1) sum|terms| per sample, from mixdown64 over the window of
    ``spatial`` that starts at ``base``."""
    local = dict(tabs, slot_src=tabs["slot_src"] - base)
    want, mag, adds = rd.mixdown64(local, C, T, window, scales, prefill, amb, amb_scale)
    bound = rd.gamma(adds + 1) * mag
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= bound).all(), (family, float(np.max(err - bound)), np.unravel_index(np.argmax(err - bound), err.shape))
    nz = bound > 0
    record(f"{family} (err / gamma bound)", float(np.max(err[nz] / bound[nz])) if nz.any() else 0.0, 1.0)


def run_mix_slot_src(r, position, T=12289, C=3, accumulate=False):
    """al_mix.slot_src past the position: the event blocks lie there inside a ``spatial`` of that size, the first across it."""
    L, n_ev = 700, 6
    rng = np.random.default_rng(41)
    window, offs = rd.mix_spatial(n_ev, C, L, 3)
    scales = rng.uniform(0.1, 3.0, n_ev).astype(np.float32)
    prefill = rng.uniform(-1, 1, (C, T)).astype(np.float32) if accumulate else None
    out = {}
    for base in (POSITIONS[position] - 1024, 0):
        need(r, 4 * (base + window.size))
        spatial = reserve(r, base + window.size)
        rd.put(r, spatial[base:], window)
        case = mix_slots(C, T, L, [base + o for o in offs], n_ev)
        tabs = case.tables()
        scene_buf = rd.Guarded(r, C * T, init=prefill)
        sc_dev = r.mem.upload(scales)
        desc, keep = mix_desc(r, tabs, C, T, accumulate, spatial, sc_dev, scene_buf.ptr)
        r.lib.call("al_mixdown", ct.byref(desc), r.mem.stream())
        out[base] = scene_buf.get().reshape(C, T)
        check_mix(out[base], tabs, C, T, window, base, scales, prefill, None, None, f"wide mixdown slot_src {position}")
        del spatial
    assert straddles(POSITIONS[position] - 1024 + offs[0], C * L, POSITIONS[position])
    high, low = out[POSITIONS[position] - 1024], out[0]
    assert_bits_equal(high, low, ("mixdown slot_src", position, accumulate))


def run_mix_row_base(r, T, accumulate=False, ambience=False):
    """A scene whose row base c n_samples passes 2^31: enough capsules of an existing test_mixdown length to cross, with the row
    that lies across 2^31, the row past it and row 0 checked (downloaded alone; the rows between are written and never read
    back).  Every row's twin is a one-capsule scene reading the same floats of ``spatial``.  ``ambience``: the (C, T) noise has
    the same row bases; only the checked rows of it are filled."""
    C = (1 << 31) // T + 2                  # row C - 2 lies across 2^31, row C - 1 past it
    rows = (0, C - 2, C - 1)
    assert (C - 2) * T < 1 << 31 < (C - 1) * T
    L, n_ev = 700, 4
    rng = np.random.default_rng(43)
    window, offs = rd.mix_spatial(n_ev, C, L, 5)
    scales = rng.uniform(0.1, 3.0, n_ev).astype(np.float32)
    need(r, 4 * (C * T + 2 * G) * (2 if ambience else 1) + 4 * window.size)
    spatial = r.mem.upload(window)
    sc_dev = r.mem.upload(scales)
    case = mix_slots(C, T, L, offs, n_ev)
    tabs = case.tables()
    scene_buf = reserve(r, G + C * T + G)
    fill_sentinel(scene_buf, 0, G)
    fill_sentinel(scene_buf, G + C * T, 2 * G + C * T)
    prefill = {c: rng.uniform(-1, 1, T).astype(np.float32) for c in rows} if accumulate else {}
    for c, x in prefill.items():
        rd.put(r, scene_buf[G + c * T:], x)
    amb = amb_dev = amb_scale = amb_scale_dev = None
    if ambience:
        amb = {c: rng.standard_normal(T).astype(np.float32) for c in rows}
        amb_scale = np.linspace(0.25, 2.0, C).astype(np.float32)
        amb_dev, amb_scale_dev = reserve(r, C * T), r.mem.upload(amb_scale)
        for c, x in amb.items():
            rd.put(r, amb_dev[c * T:], x)
    desc, keep = mix_desc(r, tabs, C, T, accumulate, spatial, sc_dev, r.mem.ptr(scene_buf) + 4 * G, amb_dev, amb_scale_dev)
    r.lib.call("al_mixdown", ct.byref(desc), r.mem.stream())
    r.mem.synchronize()
    assert_sentinel(r, scene_buf, 0, G, "scene, guard below")
    assert_sentinel(r, scene_buf, G + C * T, 2 * G + C * T, "scene, guard above")
    family = f"wide mixdown row base T={T}"
    for c in rows:
        got = rd.download(r, scene_buf[G + c * T: G + (c + 1) * T]).reshape(1, T)
        # the twin: one capsule, every slot reading row c of its event's block
        twin = dict(tabs, slot_src=tabs["slot_src"] + c * tabs["slot_len"].astype(np.int64))
        pre = prefill[c].reshape(1, T) if accumulate else None
        a = amb[c].reshape(1, T) if ambience else None
        a_s = amb_scale[c: c + 1] if ambience else None
        check_mix(got, twin, 1, T, window, 0, scales, pre, a, a_s, family)
        low = rd.Guarded(r, T, init=pre)
        a_dev = r.mem.upload(amb[c]) if ambience else None
        a_s_dev = r.mem.upload(a_s) if ambience else None
        d1, keep1 = mix_desc(r, twin, 1, T, accumulate, spatial, sc_dev, low.ptr, a_dev, a_s_dev)
        r.lib.call("al_mixdown", ct.byref(d1), r.mem.stream())
        assert_bits_equal(got.reshape(-1), low.get(), (family, "row", c))


# ----------------------------------------------------------------------------- C. image-source entries
ISM_ROOM, ISM_BETAS, ISM_FS = (4.1, 3.3, 2.6), (0.8, 0.9, 0.75, 0.85, 0.6, 0.7), 16000.0
ISM_PITCH = (1 << 20) + 4          # does not divide 2^31: one row lies across it


def ism_geometry(n_cap, n_src):
    rng = np.random.default_rng(77)
    src = rng.uniform(0.3, 1.0, (n_src, 3)) * np.array(ISM_ROOM) * 0.5
    cap = np.array(ISM_ROOM) * 0.5 + rng.uniform(0.2, 0.45, (n_cap, 3)) * np.array(ISM_ROOM)
    return src, cap


ISM_TAIL = dict(M=100, F=50, seed=0xA5A5F00D12345678)      # the tail kernel takes every row from sample 256 on


def ism_call(r, src, cap, ir_len, pitch, out_ptr, max_order=1, tail=False, sid0=0, cid0=0):
    """al_ism_shoebox, or al_ism_shoebox_tail with ISM_TAIL and the envelope table of the room; returns that table (or None)."""
    from audiblelight_amd import shoebox

    mem = r.mem
    s_dev, c_dev = mem.upload(np.ascontiguousarray(src, np.float64).reshape(-1)), mem.upload(np.ascontiguousarray(cap, np.float64).reshape(-1))
    room, betas = (ct.c_double * 3)(*ISM_ROOM), (ct.c_double * 6)(*ISM_BETAS)
    ln_env = None
    if tail:
        ln_env = np.ascontiguousarray(shoebox.tail_envelope(ISM_ROOM, ISM_BETAS, ir_len, ISM_FS, min(ISM_TAIL["M"], ir_len), sb.C_SOUND),
                                      dtype=np.float64)
        env_dev = mem.upload(ln_env)
        r.lib.call("al_ism_shoebox_tail", mem.ptr(s_dev), len(src), mem.ptr(c_dev), len(cap), room, betas, sb.C_SOUND, ISM_FS, max_order,
                   int(ir_len), int(pitch), ISM_TAIL["M"], ISM_TAIL["F"], ISM_TAIL["seed"], int(sid0), int(cid0), mem.ptr(env_dev),
                   len(ln_env), out_ptr, mem.stream())
    else:
        r.lib.call("al_ism_shoebox", mem.ptr(s_dev), len(src), mem.ptr(c_dev), len(cap), room, betas, sb.C_SOUND, ISM_FS, max_order,
                   int(ir_len), int(pitch), out_ptr, mem.stream())
    mem.synchronize()
    return ln_env


def ism_rows(n_cap, n_src, pitch):
    """The pairs to look at: the first, the one whose row lies across float 2^31, the last two, and a drawn sample."""
    pairs = n_cap * n_src
    across = (1 << 31) // pitch
    drawn = np.random.default_rng(5).integers(0, pairs, 6).tolist()
    return sorted({0, across - 1, min(across, pairs - 1), pairs - 3, pairs - 2, pairs - 1, *drawn})


def run_ism_shoebox(r, tail=False, ir_len=300):
    """al_ism_shoebox (or, ``tail``, al_ism_shoebox_tail: k_ism_shoebox<true> below sample 256, k_ism_tail from there on) with
    n_capsules x n_sources x pitch just past 2^31 floats: a short row at a wide pitch, max_order = 1.  The looked-at rows against
    shoebox_cases' oracle and bound (with a tail: shoebox_tail_cases' restatement and bound), against the same pair rendered
    alone, and zero behind ir_len."""
    from tests import shoebox_tail_cases as tc

    n_cap, n_src, pitch = 3, 683, ISM_PITCH
    total = n_cap * n_src * pitch
    assert total > 1 << 31 and total - pitch < (1 << 31) + pitch
    need(r, 4 * (total + 2 * G))
    src, cap = ism_geometry(n_cap, n_src)
    out = reserve(r, total + 2 * G)
    fill_sentinel(out, 0, G)
    fill_sentinel(out, G + total, 2 * G + total)
    ln_env = ism_call(r, src, cap, ir_len, pitch, r.mem.ptr(out) + 4 * G, tail=tail)
    assert_sentinel(r, out, 0, G, "ism rows, guard below")
    assert_sentinel(r, out, G + total, 2 * G + total, "ism rows, guard above")
    for pair in ism_rows(n_cap, n_src, pitch):
        ci, ni = divmod(pair, n_src)
        row = rd.download(r, out[G + pair * pitch: G + pair * pitch + 4096])
        assert not bits(row[ir_len:]).any(), ("pad samples must be +0", pair)
        end = rd.download(r, out[G + (pair + 1) * pitch - 4096: G + (pair + 1) * pitch])
        assert not bits(end).any(), ("the end of the pitch must be +0", pair)
        y64, A, _ = sb.oracle(ISM_ROOM, ISM_BETAS, src[ni], cap[ci], ir_len, ISM_FS, max_order=1)
        if tail:
            h, bound = tc.restate(y64[0, 0], A[0, 0], ln_env, ir_len, ISM_TAIL["M"], ISM_TAIL["F"], ISM_TAIL["seed"], ni, ci)
            err = np.abs(row[:ir_len].astype(np.float64) - h)
            assert np.all(err <= bound), ("wide pitch with a tail, pair", pair, "err / bound", float((err / bound).max()))
            record("wide ism tail (err / bound)", float((err / bound).max()), 1.0)
        else:
            sb.assert_within_bound(row[:ir_len], y64[0, 0], A[0, 0], f"wide pitch, pair {pair}")
        alone = rd.Guarded(r, 304)
        ism_call(r, src[ni: ni + 1], cap[ci: ci + 1], ir_len, 304, alone.ptr, tail=tail, sid0=ni, cid0=ci)
        assert_bits_equal(row[:ir_len], alone.get()[:ir_len], ("ism pair alone", pair))


# ----------------------------------------------------------------------------- D. flat kernels past 2^31 elements (device only)
N_FLAT = (1 << 31) + 3077
CHUNK = 1 << 28
PRIME = 8191


def ramp(torch, device, lo, hi, dtype=None):
    """The exact pattern: (i mod 8191) - 4095 as float32, for i in [lo, hi)."""
    i = torch.arange(lo, hi, device=device, dtype=torch.int64)
    return ((i % PRIME) - 4095).to(dtype or torch.float32)


def ramp_fill(r, n):
    torch = r.mem.torch
    x = reserve(r, n)
    for lo in range(0, n, CHUNK):
        hi = min(lo + CHUNK, n)
        x[lo:hi] = ramp(torch, x.device, lo, hi)
    return x


def assert_chunks(r, got, want_of, what):
    """got[lo:hi] == want_of(lo, hi) over the whole buffer, verified ON THE DEVICE in chunks of 2^28 elements."""
    torch, n = r.mem.torch, got.numel()
    for lo in range(0, n, CHUNK):
        hi = min(lo + CHUNK, n)
        want = want_of(lo, hi)
        if not torch.equal(got[lo:hi], want):
            first = lo + int(torch.nonzero(got[lo:hi] != want)[0, 0])
            raise AssertionError(f"{what}: differs first at element {first}: {got[first].item()!r} against {want[first - lo].item()!r}")


def windows(n):
    """The two ends and a window around every multiple of 2^31 below n: what is downloaded to the host."""
    w = [(0, 4096), (n - 4096, n)]
    w += [(m - 2048, min(m + 2048, n)) for m in range(1 << 31, n, 1 << 31)]
    return w


def run_flat_elementwise(r, entry):
    """One pass of an element-wise entry over 2^31 + 3077 floats of the exact ramp; every result is exactly representable."""
    torch, mem = r.mem.torch, r.mem
    n = N_FLAT
    need(r, 4 * n * (2 if entry in ("al_axpy", "al_wrap_copy", "preemph") else 1) + 12 * CHUNK * 4)
    x = ramp_fill(r, n)
    dev = x.device
    if entry == "al_scale_rows":
        s = mem.upload(np.array([0.5], np.float32))
        r.lib.call(entry, mem.ptr(x), n, mem.ptr(s), mem.stream())
        want = lambda lo, hi: ramp(torch, dev, lo, hi) * 0.5                                   # noqa: E731
    elif entry == "al_scale_rows_f64":
        s = mem.upload(np.array([-0.25], np.float64))
        r.lib.call(entry, mem.ptr(x), n, mem.ptr(s), mem.stream())
        want = lambda lo, hi: ramp(torch, dev, lo, hi) * -0.25                                 # noqa: E731
    elif entry == "al_axpy":
        y = ramp_fill(r, n)
        a = mem.upload(np.array([2.0], np.float32))
        r.lib.call(entry, mem.ptr(y), mem.ptr(x), mem.ptr(a), n, mem.stream())
        x = y
        want = lambda lo, hi: ramp(torch, dev, lo, hi) * 3.0                                   # noqa: E731
    elif entry == "gain":
        p = (ct.c_float * 1)(0.125)
        r.lib.call("al_fx_apply", _hip.FX_GAIN, mem.ptr(x), mem.ptr(x), n, ct.cast(p, ct.c_void_p), None, mem.stream())
        want = lambda lo, hi: ramp(torch, dev, lo, hi) * 0.125                                 # noqa: E731
    elif entry == "clip":
        p = (ct.c_float * 1)(1000.0)
        r.lib.call("al_fx_apply", _hip.FX_CLIP, mem.ptr(x), mem.ptr(x), n, ct.cast(p, ct.c_void_p), None, mem.stream())
        want = lambda lo, hi: ramp(torch, dev, lo, hi).clamp_(-1000.0, 1000.0)                 # noqa: E731
    elif entry == "preemph":       # y[t] = x[t] - 0.5 x[t-1] (integers and halves: exact); y[0] = x[0] + (2 x[0] - x[1])
        y = reserve(r, n)
        p = (ct.c_float * 1)(0.5)
        r.lib.call("al_fx_apply", _hip.FX_PREEMPH, mem.ptr(x), mem.ptr(y), n, ct.cast(p, ct.c_void_p), None, mem.stream())

        def want(lo, hi):
            w = ramp(torch, dev, lo, hi) - 0.5 * ramp(torch, dev, lo - 1, hi - 1)
            if lo == 0:
                w[0] = -4095.0 + (2 * -4095.0 - -4094.0)
            return w
        x = y
    elif entry == "al_wrap_copy":   # dst[t] = src[t mod n_src]
        n_src = 3 * PRIME + 5
        y = reserve(r, n)
        r.lib.call(entry, mem.ptr(x), n_src, mem.ptr(y), n, mem.stream())
        want = lambda lo, hi: ramp(torch, dev, 0, n_src)[torch.arange(lo, hi, device=dev) % n_src]    # noqa: E731
        x = y
    else:
        raise AssertionError(entry)
    assert_chunks(r, x, want, entry)
    for lo, hi in windows(n):       # and the same windows once on the host, through the download path
        assert_bits_equal(rd.download(r, x[lo:hi]), want(lo, hi).cpu().numpy(), (entry, lo))


def run_flat_rows(r, entry):
    """rows x cols with a high row base: 3 rows of 2^30 + 1025 floats (row 2 starts past 2^31)."""
    torch, mem = r.mem.torch, r.mem
    rows, cols = 3, (1 << 30) + 1025
    n = rows * cols
    need(r, 4 * n * (2 if entry == "al_axpy_rows" else 1) + 12 * CHUNK * 4)
    x = ramp_fill(r, n)
    dev = x.device
    a = np.array([0.5, -2.0, 0.25], np.float32)
    a_dev = mem.upload(a)
    if entry == "al_scale_matrix_rows":
        r.lib.call(entry, mem.ptr(x), rows, cols, mem.ptr(a_dev), mem.stream())
        got, k = x, a
    elif entry == "al_axpy_rows":
        y = ramp_fill(r, n)
        r.lib.call(entry, mem.ptr(y), mem.ptr(x), mem.ptr(a_dev), rows, cols, mem.stream())
        got, k = y, a + 1
    elif entry == "al_row_stats":
        # out[r] = {sum|x|, max|x|, non-finite count, sum x^2} in float64, against float64 torch reductions with the bound of
        # kernel_edges.run_row_stats: a partial of 16384 samples takes at most 73 roundings, asserted as 40 eps of the sum
        out = rd.download(r, r.row_stats(x, rows, cols), 4 * rows).reshape(rows, 4)
        for row in range(rows):
            s1 = s2 = 0.0
            mx = 0.0
            for lo in range(row * cols, (row + 1) * cols, CHUNK):
                v = x[lo: min(lo + CHUNK, (row + 1) * cols)].double()
                s1 += float(v.abs().sum())
                s2 += float((v * v).sum())
                mx = max(mx, float(v.abs().max()))
            assert out[row, 1] == mx and out[row, 2] == 0, (row, out[row])
            record("wide row_stats sums (rel err / eps)", abs(out[row, 0] - s1) / s1 / rd.EPS, 40.0)
            record("wide row_stats sums (rel err / eps)", abs(out[row, 3] - s2) / s2 / rd.EPS, 40.0)
        return
    elif entry == "al_peak_scale":
        # the peak of the whole buffer sits in its LAST element: 1 / (|p| max|x| + tiny) must see it.  One flat buffer of N_FLAT
        # elements (the entry takes n alone): two thirds of the three rows' reduction time
        n = N_FLAT
        x[n - 1] = 70000.0
        out = mem.upload(np.zeros(1, np.float32))
        r.lib.call(entry, mem.ptr(x), n, 1.5, mem.ptr(out), mem.stream())
        want = 1.5 / (1.5 * 70000.0 + float(np.finfo(np.float32).tiny))       # in float64, rounded once: kernel_edges.run_peak_scale
        got = np.float64(rd.download(r, out, 1)[0])
        record("wide peak_scale (ulp)", float(ulps(got, want)), 0.5 + 1e-6)
        return
    else:
        raise AssertionError(entry)

    def want(lo, hi):
        w = ramp(torch, dev, lo, hi)
        row = torch.arange(lo, hi, device=dev) // cols
        return w * torch.tensor(k, device=dev)[row]
    assert_chunks(r, got, want, entry)


def run_flat_pack_irs(r, f64):
    """al_pack_irs_f32 / _f64 with rows x dst_pitch past 2^31: rows of 1021 samples at a pitch of 1024."""
    torch, mem = r.mem.torch, r.mem
    length, pitch = 1021, 1024
    rows = (1 << 31) // pitch + 3
    need(r, rows * (length * (8 if f64 else 4) + pitch * 4) + 16 * CHUNK * 4)
    src = reserve(r, rows * length, np.float64 if f64 else np.float32)
    dev = src.device
    for lo in range(0, rows * length, CHUNK):
        hi = min(lo + CHUNK, rows * length)
        src[lo:hi] = ramp(torch, dev, lo, hi, src.dtype)
    dst = reserve(r, rows * pitch)
    r.lib.call("al_pack_irs_f64" if f64 else "al_pack_irs_f32", mem.ptr(src), mem.ptr(dst), rows, length, pitch, mem.stream())

    def want(lo, hi):
        i = torch.arange(lo, hi, device=dev, dtype=torch.int64)
        row, t = i // pitch, i % pitch
        return torch.where(t < length, (((row * length + t) % PRIME) - 4095).float(), torch.zeros((), device=dev))
    assert_chunks(r, dst, want, "al_pack_irs")


def run_flat_normal_fill(r):
    """al_normal_fill over 2^31 + 3077 floats: element i is a function of (seed, tag, i) alone, so the first 4096 elements equal
    a short call's; past 2^31 the draws are compared with the host restatement of tests/noise_draw_cases.py, and the whole
    buffer is finite with the moments of a standard normal (mean and variance within 6 standard errors)."""
    from tests import noise_draw_cases as nd

    torch, mem = r.mem.torch, r.mem
    n = N_FLAT
    need(r, 4 * n + 12 * CHUNK * 4)
    out = reserve(r, n + 2 * G)
    fill_sentinel(out, 0, G)
    fill_sentinel(out, G + n, 2 * G + n)
    r.lib.call("al_normal_fill", mem.ptr(out) + 4 * G, n, 99, 3, 1.0, mem.stream())
    mem.synchronize()
    assert_sentinel(r, out, 0, G, "normal fill, guard below")
    assert_sentinel(r, out, G + n, 2 * G + n, "normal fill, guard above")
    short = reserve(r, 4096)
    r.lib.call("al_normal_fill", mem.ptr(short), 4096, 99, 3, 1.0, mem.stream())
    assert torch.equal(out[G: G + 4096], short)
    s1 = s2 = 0.0
    for lo in range(0, n, CHUNK):
        v = out[G + lo: G + min(lo + CHUNK, n)].double()
        assert bool(torch.isfinite(v).all())
        s1 += float(v.sum())
        s2 += float((v * v).sum())
    mean, var = s1 / n, s2 / n - (s1 / n) ** 2
    assert abs(mean) <= 6 / np.sqrt(n) and abs(var - 1) <= 6 * np.sqrt(2 / n), (mean, var)
    for lo, hi in ((n - 512, n), ((1 << 31) - 256, (1 << 31) + 256)):
        nd.check_draws(rd.download(r, out[G + lo: G + hi]), nd.restated_normals(99, 3, lo, hi), 1.0,
                       "wide normal_fill (err / tolerance)", (lo, hi))


def run_flat_encode_frames(r, pcm16, C):
    """al_encode_frames with n_samples x n_capsules past 2^31: the (C, T) scene of the ramp / 8192 (exact; times 32768 an integer
    below 2^15) to (T, C) frames.  C = 8 (PCM_16) and C = 4 (float32) take the two 16-byte store arms, C = 3 the scalar one."""
    torch, mem = r.mem.torch, r.mem
    T = (1 << 31) // C + 1027
    n = C * T
    assert n > 1 << 31
    need(r, 4 * n + (2 if pcm16 else 4) * n + 16 * CHUNK * 4)
    scene = ramp_fill(r, n)
    for lo in range(0, n, CHUNK):
        scene[lo: lo + CHUNK] *= 1.0 / 8192
    out = reserve(r, n, np.int16 if pcm16 else np.float32)
    r.lib.call("al_encode_frames", mem.ptr(scene), C, T, _hip.FRAMES_PCM16 if pcm16 else _hip.FRAMES_F32, mem.ptr(out), mem.stream())
    rows, frames = scene.view(C, T), out.view(T, C)
    step = CHUNK // 8
    for t0 in range(0, T, step):
        t1 = min(t0 + step, T)
        want = rows[:, t0:t1].t()
        want = (want * 32768.0).to(torch.int16) if pcm16 else want        # an exact integer in int16's range: no rounding, no clipping
        if not torch.equal(frames[t0:t1], want):
            bad = torch.nonzero(frames[t0:t1] != want)[0]
            raise AssertionError(f"al_encode_frames: frame {t0 + int(bad[0])}, capsule {int(bad[1])} differs")


def run_flat_pack_ragged(r):
    """al_pack_ragged_irs with rows x dst_pitch past 2^31 AND offsets[] entries past 2^31: row q = src[offsets[q] : offsets[q] +
    lens[q]], lens 1021, 1020, 1019 in turn, zeros up to the pitch of 1024."""
    torch, mem = r.mem.torch, r.mem
    length, pitch = 1021, 1024
    rows = (1 << 31) // length + 3
    need(r, rows * (length * 4 + pitch * 4 + 12) + 16 * CHUNK * 4)
    src = ramp_fill(r, rows * length)
    dev = src.device
    q = torch.arange(rows, device=dev, dtype=torch.int64)
    offsets, lens = q * length, (length - q % 3).to(torch.int32)
    assert int(offsets[-1]) > 1 << 31 and rows * pitch > 1 << 31
    dst = reserve(r, rows * pitch)
    r.lib.call("al_pack_ragged_irs", mem.ptr(src), 0, mem.ptr(offsets), mem.ptr(lens), rows, pitch, mem.ptr(dst), mem.stream())

    def want(lo, hi):
        i = torch.arange(lo, hi, device=dev, dtype=torch.int64)
        row, t = i // pitch, i % pitch
        return torch.where(t < length - row % 3, (((row * length + t) % PRIME) - 4095).float(), torch.zeros((), device=dev))
    assert_chunks(r, dst, want, "al_pack_ragged_irs")


def run_flat_fade(r, shape_in="linear", shape_out="logarithmic", n_fade=4096):
    """The fade op of al_fx_apply over N_FLAT floats of the ramp, in place: a fade-in over the first and a fade-out over the last
    4096 samples (the last ones past element 2^31), checked with kernel_edges.run_fx_fade's bound (8 eps of |x|) against the
    oracle's envelope -- that of a clip of 4 n_fade samples, whose two ends are the long clip's -- and x itself, exactly, between."""
    from oracle import synth_oracle as orc
    from tests.kernel_edges import EPS, TINY32, fx

    torch, mem = r.mem.torch, r.mem
    n = N_FLAT
    need(r, 4 * n + 12 * CHUNK * 4)
    x = ramp_fill(r, n)
    dev = x.device
    fx(r, _hip.FX_FADE, mem.ptr(x), mem.ptr(x), n, 0.0, [n_fade, n_fade, _hip.FADE_SHAPES[shape_in], _hip.FADE_SHAPES[shape_out]])
    env = np.asarray(orc.fade_envelope(4 * n_fade, 1, n_fade, n_fade, shape_in, shape_out), dtype=np.float64).reshape(-1)
    for lo, hi, e in ((0, n_fade, env[:n_fade]), (n - n_fade, n, env[-n_fade:])):
        got = rd.download(r, x[lo:hi]).astype(np.float64)
        x64 = ramp(torch, dev, lo, hi).cpu().numpy().astype(np.float64)
        record("wide fx_fade (err / (eps |x|))", float(np.max(np.abs(got - x64 * e) / np.maximum(np.abs(x64), TINY32))) / EPS, 8.0)
    middle = x[n_fade: n - n_fade]

    def want(lo, hi):
        return ramp(torch, dev, n_fade + lo, n_fade + hi)
    assert_chunks(r, middle, want, "al_fx_apply fade, between the fades")


def run_flat_resample_poly(r):
    """al_resample_poly with rows x out_pitch (and rows x n_in) past 2^31: 2 rows of 2^30 + 1025 samples of the ramp, up = down = 1,
    three taps (0.25, 1, 0.5): out[m] = 0.5 x[m-1] + x[m] + 0.25 x[m+1] (integers and quarters: every fma exact), zeros up to the
    pitch of n_out + 3."""
    torch, mem = r.mem.torch, r.mem
    rows, n_in = 2, (1 << 30) + 1025
    pitch = n_in + 3
    need(r, 4 * rows * (n_in + pitch) + 16 * CHUNK * 4)
    x = ramp_fill(r, rows * n_in)
    dev = x.device
    taps = mem.upload(np.array([0.25, 1.0, 0.5], np.float32))
    out = reserve(r, rows * pitch)
    r.lib.call("al_resample_poly", mem.ptr(x), rows, n_in, mem.ptr(taps), 1, 1, 1, mem.ptr(out), n_in, pitch, mem.stream())

    def sample(row, t):
        return (((row * n_in + t) % PRIME) - 4095).float()

    def want(lo, hi):
        i = torch.arange(lo, hi, device=dev, dtype=torch.int64)
        row, m = i // pitch, i % pitch
        zero = torch.zeros((), device=dev)
        w = sample(row, m) + torch.where(m > 0, 0.5 * sample(row, m - 1), zero) + torch.where(m < n_in - 1, 0.25 * sample(row, m + 1), zero)
        return torch.where(m < n_in, w, zero)
    assert_chunks(r, out, want, "al_resample_poly")


def run_flat_noise_irfft(r, n=4096):
    """al_noise_irfft with rows x n past 2^31: 2^19 + 3 series of 4096 samples, the draws made on the device (al_normal_fill).
    Looked at: row 0, the row that starts at float 2^31, the last two.  Each against numpy's float64 irfft of its own draws with
    kernel_edges.run_noise_irfft's bound, and bit for bit against the same row transformed alone; every output finite."""
    from tests.kernel_edges import EPS, fft_bound, peak_error

    torch, mem = r.mem.torch, r.mem
    rows, bins = (1 << 31) // n + 3, n // 2 + 1
    work_floats = r.lib.call("al_noise_workspace_floats", rows, n)
    need(r, 4 * (2 * rows * bins + rows * n + work_floats + 2 * G) + 2 * CHUNK * 4)
    zr, zi = reserve(r, rows * bins), reserve(r, rows * bins)
    r.lib.call("al_normal_fill", mem.ptr(zr), rows * bins, 11, 5, 1.0, mem.stream())
    r.lib.call("al_normal_fill", mem.ptr(zi), rows * bins, 12, 5, 1.0, mem.stream())
    shape = (1.0 / np.sqrt(1.0 + np.arange(bins))).astype(np.float32)
    d_s = mem.upload(shape)
    inv_sigma = float(np.float32(0.37))
    work = reserve(r, work_floats)
    out = reserve(r, rows * n + 2 * G)
    fill_sentinel(out, 0, G)
    fill_sentinel(out, G + rows * n, 2 * G + rows * n)
    r.lib.call("al_noise_irfft", mem.ptr(zr), mem.ptr(zi), mem.ptr(d_s), rows, n, ct.c_float(inv_sigma), mem.ptr(out) + 4 * G,
               mem.ptr(work), mem.stream())
    mem.synchronize()
    assert_sentinel(r, out, 0, G, "noise rows, guard below")
    assert_sentinel(r, out, G + rows * n, 2 * G + rows * n, "noise rows, guard above")
    for lo in range(0, rows * n, CHUNK):
        assert bool(torch.isfinite(out[G + lo: G + min(lo + CHUNK, rows * n)]).all()), lo
    lg, blue = fft_bound(n // 2)
    assert not blue
    work1 = reserve(r, r.lib.call("al_noise_workspace_floats", 1, n))
    for row in (0, (1 << 31) // n - 1, (1 << 31) // n, rows - 2, rows - 1):
        got = rd.download(r, out[G + row * n: G + (row + 1) * n])
        a, b = rd.download(r, zr[row * bins: (row + 1) * bins]).astype(np.float64), rd.download(r, zi[row * bins: (row + 1) * bins]).astype(np.float64)
        S = shape.astype(np.float64) * (a + 1j * b)
        S[0] = S[0].real * np.sqrt(2)
        S[-1] = S[-1].real * np.sqrt(2)
        ref = np.fft.irfft(S, n=n) * inv_sigma
        record("wide noise_irfft (err/peak / ((log2+1) eps))", peak_error(got, ref) / ((lg + 1) * EPS), 2.0)
        alone = rd.Guarded(r, n)
        r.lib.call("al_noise_irfft", mem.ptr(zr) + 4 * row * bins, mem.ptr(zi) + 4 * row * bins, mem.ptr(d_s), 1, n, ct.c_float(inv_sigma),
                   alone.ptr, mem.ptr(work1), mem.stream())
        assert_bits_equal(got, alone.get(), ("noise_irfft row alone", row))


def run_flat_stft(r, fft=512, win=256, hop=128):
    """al_stft with series x fft_size past 2^31: one row of (2^22 + 64) x 128 samples, 2^22 + 65 frames of 512 points (the spectrum:
    2.16e9 floats).  The last 64 frames equal, bit for bit, the frames of the row's last 66 x 128 samples transformed alone (whose
    first two frames see the left padding instead of the signal and are not compared); those against the oracle's float64 frames
    with kernel_edges.run_stft's bound; the first frames likewise; every output finite."""
    from oracle import synth_oracle as orc
    from tests.kernel_edges import EPS, fft_bound, peak_error

    torch, mem = r.mem.torch, r.mem
    n = ((1 << 22) + 64) * hop
    n_frames, nf = orc.frame_count(n, hop), fft // 2 + 1
    assert n_frames * fft > 1 << 31
    work_floats = r.lib.call("al_stft_workspace_floats", n_frames, fft)
    need(r, 4 * (n + n_frames * nf * 2 + 2 * G + work_floats) + 8 * CHUNK * 4)
    y = reserve(r, n)
    r.lib.call("al_normal_fill", mem.ptr(y), n, 21, 5, 0.25, mem.stream())
    work = reserve(r, work_floats)
    total = n_frames * nf * 2
    out = reserve(r, total + 2 * G)
    fill_sentinel(out, 0, G)
    fill_sentinel(out, G + total, 2 * G + total)
    r.lib.call("al_stft", mem.ptr(y), 1, n, fft, win, hop, mem.ptr(out) + 4 * G, mem.ptr(work), mem.stream())
    mem.synchronize()
    assert_sentinel(r, out, 0, G, "stft, guard below")
    assert_sentinel(r, out, G + total, 2 * G + total, "stft, guard above")
    for lo in range(0, total, CHUNK):
        assert bool(torch.isfinite(out[G + lo: G + min(lo + CHUNK, total)]).all()), lo
    lg, blue = fft_bound(fft)
    assert not blue
    m = 66 * hop                                     # the sub-signals: the first and the last 66 hops of the row
    for start in (0, n - m):
        sub = rd.download(r, y[start: start + m])
        ref = orc.stft_frames(sub.astype(np.float64), fft, win, hop)
        f_sub = ref.shape[0]
        first = start // hop                         # frame j of the sub-signal is frame first + j of the row
        keep = slice(0, f_sub - 2) if start == 0 else slice(2, f_sub)      # away from the end the sub-signal pads and the row does not
        got = rd.download(r, out[G + first * nf * 2: G + (first + f_sub) * nf * 2]).view(np.complex64).reshape(f_sub, nf)
        assert np.abs(got[keep]).max() > 0
        record("wide stft (err/peak / ((log2+1) eps))", peak_error(got[keep], ref[keep]) / ((lg + 1) * EPS), 2.0)
        alone = rd.Guarded(r, f_sub * nf * 2)
        work1 = reserve(r, r.lib.call("al_stft_workspace_floats", f_sub, fft))
        r.lib.call("al_stft", mem.ptr(y) + 4 * start, 1, m, fft, win, hop, alone.ptr, mem.ptr(work1), mem.stream())
        assert_bits_equal(got[keep].view(np.float32), alone.get().view(np.complex64).reshape(f_sub, nf)[keep].view(np.float32),
                          ("stft frames alone", start))
    assert first + f_sub == n_frames, (first, f_sub, n_frames)


def ism_wide_rows(r, n_rows, pitch, launch, check_row, ir_len):
    """The frame of the image-source cases with other entries: ``launch(out_ptr)`` fills n_rows x pitch floats just past 2^31 in a
    guarded buffer; ``check_row(row index, its first ir_len samples)`` for the rows of ism_rows; +0 behind ir_len."""
    total = n_rows * pitch
    assert total > 1 << 31 and total < (1 << 31) + 5 * pitch
    need(r, 4 * (total + 2 * G))
    out = reserve(r, total + 2 * G)
    fill_sentinel(out, 0, G)
    fill_sentinel(out, G + total, 2 * G + total)
    launch(r.mem.ptr(out) + 4 * G)
    r.mem.synchronize()
    assert_sentinel(r, out, 0, G, "ism rows, guard below")
    assert_sentinel(r, out, G + total, 2 * G + total, "ism rows, guard above")
    for row in ism_rows(n_rows, 1, pitch):
        head = rd.download(r, out[G + row * pitch: G + row * pitch + 4096])
        assert not bits(head[ir_len:]).any(), ("pad samples must be +0", row)
        end = rd.download(r, out[G + (row + 1) * pitch - 4096: G + (row + 1) * pitch])
        assert not bits(end).any(), ("the end of the pitch must be +0", row)
        check_row(row, head[:ir_len])


def run_ism_dir(r, ir_len=300):
    """al_ism_shoebox_dir: 684 receiver positions x 3 channels x 1 source x ISM_PITCH, just past 2^31 floats.  The kernel forms the
    row of a position's channel 0 and steps to the other channels by a stride, so the LAST position's channel 0 (row 2049) must
    itself start past 2^31: 683 positions would leave it below.  The rows against shoebox_directional_cases' oracle with
    shoebox_cases' bound, and against their position rendered alone."""
    from tests import shoebox_directional_cases as dc

    mem = r.mem
    P, K = 684, 3
    assert (P - 1) * K * ISM_PITCH > 1 << 31
    src, pos = ism_geometry(P, 1)
    pat = np.ascontiguousarray(np.broadcast_to(dc.mixed4()[:K], (P, K, 4)), dtype=np.float64)
    room, betas = (ct.c_double * 3)(*ISM_ROOM), (ct.c_double * 6)(*ISM_BETAS)
    s_dev = mem.upload(src.reshape(-1))

    def call(positions, patterns, pitch, out_ptr):
        p_dev, t_dev = mem.upload(np.ascontiguousarray(positions).reshape(-1)), mem.upload(np.ascontiguousarray(patterns).reshape(-1))
        r.lib.call("al_ism_shoebox_dir", mem.ptr(s_dev), 1, mem.ptr(p_dev), len(positions), mem.ptr(t_dev), K, room, betas, sb.C_SOUND,
                   ISM_FS, 1, ir_len, pitch, out_ptr, mem.stream())
        mem.synchronize()

    def check_row(row, got):
        p, k = divmod(row, K)
        y64, A, _ = dc.oracle_point(ISM_ROOM, ISM_BETAS, src[0], pos[p], pat[p], ir_len, ISM_FS, max_order=1)
        sb.assert_within_bound(got, y64[k], A[k], f"wide pitch, directional row {row}")
        alone = rd.Guarded(r, K * 304)
        call(pos[p: p + 1], pat[p: p + 1], 304, alone.ptr)
        assert_bits_equal(got, alone.get().reshape(K, 304)[k, :ir_len], ("directional position alone", row))

    ism_wide_rows(r, P * K, ISM_PITCH, lambda out_ptr: call(pos, pat, ISM_PITCH, out_ptr), check_row, ir_len)


def run_ism_bands(r, ir_len=300, n_bands=2, half=16):
    """al_ism_shoebox_bands: 3 capsules x 683 sources x ISM_PITCH, just past 2^31 floats, two bands, a workspace of 512 pairs (five
    passes); the rows against shoebox_bands_cases' restatement and bound, and against their pair rendered alone."""
    from audiblelight_amd import shoebox
    from tests import shoebox_bands_cases as bc

    mem = r.mem
    n_cap, n_src = 3, 683
    src, cap = ism_geometry(n_cap, n_src)
    beta = np.ascontiguousarray(bc.BETA_8[:, :n_bands], dtype=np.float64)
    centres = bc.centres_of(n_bands, ISM_FS)
    phi_dev = mem.upload(np.ascontiguousarray(shoebox.band_filters(centres, ISM_FS, half), dtype=np.float64).reshape(-1))
    per_pair = bc.per_pair_bytes(r, n_bands, half, ir_len)
    room = (ct.c_double * 3)(*ISM_ROOM)

    def call(sources, capsules, pitch, pairs_per_pass, out_ptr):
        s_dev, c_dev = mem.upload(np.ascontiguousarray(sources).reshape(-1)), mem.upload(np.ascontiguousarray(capsules).reshape(-1))
        ws = reserve(r, per_pair * pairs_per_pass // 8, np.float64)
        r.lib.call("al_ism_shoebox_bands", mem.ptr(s_dev), len(sources), mem.ptr(c_dev), len(capsules), room,
                   beta.ctypes.data_as(ct.POINTER(ct.c_double)), n_bands, mem.ptr(phi_dev), half, sb.C_SOUND, ISM_FS, 1, ir_len, pitch,
                   mem.ptr(ws), per_pair * pairs_per_pass, out_ptr, mem.stream())
        mem.synchronize()

    def check_row(row, got):
        ci, ni = divmod(row, n_src)
        h64, bound = bc.restate(ISM_ROOM, beta, centres, half, src[ni], cap[ci], ir_len, ISM_FS, max_order=1)
        bc.assert_within(got, h64[0, 0], bound[0, 0], f"wide pitch, bands row {row}")
        alone = rd.Guarded(r, 304)
        call(src[ni: ni + 1], cap[ci: ci + 1], 304, 1, alone.ptr)
        assert_bits_equal(got, alone.get()[:ir_len], ("bands pair alone", row))

    ism_wide_rows(r, n_cap * n_src, ISM_PITCH, lambda out_ptr: call(src, cap, ISM_PITCH, 512, out_ptr), check_row, ir_len)


class _DryEvent:
    """What synthesize._dry_batch reads of an Event."""

    def __init__(self, clip):
        self.clip, self.sample_rate, self.ref_ir_channel, self.direct_path_time_ms = clip, rd.SR, 0, (1.0, 20.0)

    def load_audio(self, ignore_cache=False):
        return self.clip


def run_dry_fetch(r, position="i31", log2_block=10):
    """The dry render's lazy fetch (synthesize._dry_batch): the dry batch planned with its ``spatial`` moved past the position (the
    planner's out_off shifted as make_plan shifts it), then ``event._spatial_audio_dry[mic]`` read through the closure the package
    installs.  The same arrays as with the plan where the planner put it, and within render_bound of the float64 convolution of
    the clip with the windowed IR row times the two scalars of the main render."""
    from audiblelight_amd import synthesize as syn

    sc = scene(log2_block, 2, kinds=("static", "static"))
    main = render(r, sc, family="wide dry fetch, main render")
    res, h = main["res"], sc["h"]
    shift = POSITIONS[position] - 1024
    real_plan = planning.plan_batch
    made = []

    def moved_plan(*args, **kw):
        pl = real_plan(*args, **kw)
        need(r, 4 * (pl.spatial_floats + shift))
        pl.events["out_off"] += shift
        pl.spatial_floats += shift
        made.append(pl)
        return pl

    got = {}
    for name, planner in (("low", real_plan), ("high", moved_plan)):
        events = [_DryEvent(c) for c in sc["clips"]]
        syn.planning.plan_batch = planner
        try:
            syn._dry_batch(r, [(ev, h[:, i: i + 1], i, i) for i, ev in enumerate(events)], "mic", res)
        finally:
            syn.planning.plan_batch = real_plan
        got[name] = [np.asarray(ev._spatial_audio_dry["mic"]) for ev in events]
    pl = made[0]
    assert straddles(int(pl.events["out_off"][0]), int(pl.events["len"][0]), POSITIONS[position]) and int(pl.events["out_off"][1]) > POSITIONS[position]
    gains = rd.download(r, res.emitter_gain, 2).astype(np.float64)
    for i, clip in enumerate(sc["clips"]):
        assert_bits_equal(got["high"][i], got["low"][i], ("dry fetch", i))
        ir = h[0, i].astype(np.float64).copy()
        peak, sr = int(np.argmax(h[0, i])), rd.SR
        ir[peak + int(20.0 * sr / 1000):] = 0
        ir[: max(peak - int(1.0 * sr / 1000), 0)] = 0
        k = gains[i] * float(np.float32(main["stats"][i, 3]))
        want = np.convolve(clip.astype(np.float64), ir) * k
        assert got["high"][i].shape == want.shape
        scale = float(np.linalg.norm(clip)) * float(np.linalg.norm(ir)) * abs(k)
        bound = rd.render_bound(pl.block, pl.n_partitions, scale) + 2 * rd.EPS * np.abs(want)
        record("wide dry fetch (err / bound)", float(np.max(np.abs(got["high"][i].astype(np.float64) - want) / bound)), 1.0)
