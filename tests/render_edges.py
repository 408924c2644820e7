"""Edge-shape scenarios for the render stage: the twiddle table, the IR energies and emitter gains, the forward spectra, the
accumulate + block synthesis (read back as the raw, unscaled ``spatial`` output), the partial statistics, the level law and the
mixdown.  Each one calls the C ABI through ``r.lib.call`` or drives a prepared batch stage by stage, and compares the result with a
float64 restatement written here (direct convolution, the formulas spelled out).  Shared by tests/test_hostemu_render_edges.py
(host emulation, small blocks) and tests/test_gpu_render_edges.py (gfx950 build, every block size and layout).

The helpers (guarded buffers, sentinels, margins) are those of tests/kernel_edges.py.  Bounds (eps = 2^-23, u = eps / 2):
  twiddles                                  bit-exact against the correctly rounded float32 value (float64 near-ties excepted)
  ir_energy, partial / event sums of |x|    gamma_d = d u / (1 - d u) relative to the float64 sum, d the summation depth
  emitter gain, level law                   a float64 formula of float32 inputs, rounded once: <= 1 ulp of float32
  spectra                                   2 (log2 2B + 1) eps of the spectrum's peak (the FFT bound of kernel_edges.py)
  rendered samples                          8 sigma of the rounding-error model derived at ``render_bound``, and 1e-5 of the peak
  mixdown                                   gamma_(k+1) of the sum of |terms| per sample (k additions, one product each)
"""
import ctypes as ct

import mpmath
import numpy as np
from scipy import signal as sp_signal

from audiblelight_amd import _hip
from audiblelight_amd import plan as planning
from tests.kernel_edges import EPS, FLT_MAX, G, MARGINS, SENTINEL, U, Guarded, assert_bits_equal, bits, peak_error, record  # noqa: F401

TINY64 = 2.2250738585072014e-308
SR = 48000
LAYOUTS = ("plain", "split", "quad", "narrow", "runs")
SENTINEL_F32 = np.resize(SENTINEL, 4).view(np.float32)[0]


def gamma(d):
    return d * U / (1 - d * U)


def sum_depth(B):
    """Summation depth of every per-block float32 sum of the transform kernels: a thread adds its own samples in sequence (at
    most 64: the quad-tile kernels' 256 threads over B = 16384; 32 in the plain and split forms), then the workgroup reduces
    the thread sums in a tree of log2(threads) <= log2(B) levels; +2 for the wave / LDS hand-over."""
    return 64 + int(np.log2(B)) + 2


def layout_flags(desc, layout):
    """al_batch.flags for one layout variant, on top of the accumulate flags the planner chose."""
    flags = desc.flags & ~(_hip.FLAG_SPLIT_SPECTRA | _hip.FLAG_QUAD_SPECTRA | _hip.FLAG_NARROW_FFT | (0xff << 16) | (0x7f << 24))
    if layout == "split":
        flags |= _hip.FLAG_SPLIT_SPECTRA
    elif layout == "quad":
        flags |= _hip.FLAG_SPLIT_SPECTRA | _hip.FLAG_QUAD_SPECTRA
    elif layout == "narrow":
        flags |= _hip.FLAG_NARROW_FFT
    elif layout == "runs":
        flags |= (3 << 16) | (2 << 24)              # AL_FLAG_SYNTH_RUN(3) | AL_FLAG_IR_RUN(2)
    return flags


def layout_ok(layout, log2_block):
    return {"split": log2_block >= 11, "quad": log2_block == 14}.get(layout, True)


def download(r, buf, n=None, dtype=None):
    r.mem.synchronize()
    a = np.asarray(r.mem.download(buf))
    return a[:n] if n is not None else a


def put(r, buf, arr):
    """Overwrite the start of a device buffer with a host array (numpy memory: in place; torch: a copy through the device)."""
    arr = np.ascontiguousarray(arr)
    if isinstance(buf, np.ndarray):
        buf[: arr.size] = arr.reshape(-1).view(buf.dtype) if arr.dtype != buf.dtype else arr.reshape(-1)
    else:
        import torch

        src = torch.from_numpy(arr.reshape(-1).view(np.float32) if arr.dtype != np.float32 else arr.reshape(-1)).to(buf.device)
        buf[: src.numel()].copy_(src.view(buf.dtype) if src.dtype != buf.dtype else src)


# ----------------------------------------------------------------------------- 1. twiddles
def run_twiddles(r, log2_block):
    """k_twiddle_init: tw[k] = (cos, sin)(-pi k / m), m = 2^log2_block, from float64 sincospi rounded to float32 once.  The
    reference is the correctly rounded float32 value (50 significant digits through mpmath).  A float64 result can round the
    other way only when the exact value lies within one float64 ulp of a float32 rounding boundary; such near-ties are listed
    from the same mpmath values, and only they may differ."""
    m = 1 << log2_block
    out = Guarded(r, 2 * m)
    r.lib.call("al_twiddle_init", ct.c_void_p(out.ptr), log2_block, r.mem.stream())
    got = out.get().reshape(m, 2)
    mpmath.mp.dps = 50
    want = np.empty((m, 2), dtype=np.float32)
    near_tie = np.zeros((m, 2), dtype=bool)
    for k in range(m):
        for j, f in enumerate((mpmath.cospi, mpmath.sinpi)):
            v = f(mpmath.mpf(-k) / m)
            w = np.float32(float(v))                    # float(v): float64 nearest; then to float32 (double rounding checked below)
            # the two float32 neighbours of the exact value and the boundary between them
            lo, hi = (w, np.nextafter(w, np.float32(np.inf))) if mpmath.mpf(float(w)) <= v else (np.nextafter(w, np.float32(-np.inf)), w)
            mid = (mpmath.mpf(float(lo)) + mpmath.mpf(float(hi))) / 2
            w = lo if v < mid else hi if v > mid else w
            want[k, j] = w if (k or j == 0) else np.float32(-0.0)      # sinpi(-0) = -0
            near_tie[k, j] = abs(v - mid) <= abs(v) * 2.0 ** -52 if v != 0 else False
    diff = (bits(got) != bits(want)) & ~((got == 0) & (want == 0))      # cospi(1/2) = 0 of either sign: a zero multiplier
    listed = [(k, "cs"[j]) for k, j in zip(*np.nonzero(diff))]
    assert not (diff & ~near_tie).any(), f"twiddles differ away from a float64 near-tie at {listed[:8]}"
    record(f"twiddle near-ties taken (B=2^{log2_block})", float(diff.sum()), max(float(near_tie.sum()), 1.0))
    return listed


# ----------------------------------------------------------------------------- batch construction
def make_plan(specs, C, Lir, log2_block, guards=False, odd=False, base=0):
    """plan_batch + optional guard bands: every event's (C, len) block moves to its own place in ``spatial`` with G sentinel
    floats before and after it (al_event.out_off rewritten in the plan's ``events`` table, spatial_floats enlarged before
    ``prepare``); ``odd`` starts every other block at an odd float offset, so both synth_store_block pair paths run.  ``base``
    (with guards) moves the whole guarded region that many floats into ``spatial``: the floats below it are never touched, the
    checks below read [base, spatial_floats) only (tests/wide_offset_cases.py puts it next to 2^31)."""
    pl = planning.plan_batch(specs, C, Lir, SR, log2_block=log2_block)
    if guards:
        off = base + G
        for i, ev in enumerate(pl.events):
            if odd and (i % 2 == 0) != (off % 2 == 1):
                off += 1
            pl.events["out_off"][i] = off
            off += C * int(ev["len"]) + G
        pl.spatial_floats = off + G
        pl.spatial_base = int(base)
    return pl


def spatial_base(pl):
    return getattr(pl, "spatial_base", 0)


def sentinel_spatial(r, batch):
    """Replace the batch's ``spatial`` by a buffer filled with the sentinel pattern (every chunk descriptor repointed).  With a
    plan moved to ``base``, the batch's own buffer is kept and only [base, spatial_floats) is filled."""
    n, base = batch.plan.spatial_floats, spatial_base(batch.plan)
    if base:
        buf = batch.bufs["spatial"]
        put(r, buf[base:], np.resize(SENTINEL, 4 * (n - base)).view(np.float32))
        return buf
    buf = r.mem.upload(np.resize(SENTINEL, 4 * n).view(np.float32))
    batch.bufs["spatial"] = buf
    for desc in batch.descs:
        desc.spatial = r.mem.ptr(buf)
    return buf


def check_guards(r, batch):
    """Every float of ``spatial`` outside the events' (C, len) blocks still holds the sentinel; returns the buffer from
    ``spatial_base(plan)`` on (the whole buffer unless the plan was moved)."""
    pl = batch.plan
    base = spatial_base(pl)
    sp = download(r, batch.bufs["spatial"][base: pl.spatial_floats])
    inside = np.zeros(pl.spatial_floats - base, dtype=bool)
    for ev in pl.events:
        inside[int(ev["out_off"]) - base: int(ev["out_off"]) - base + pl.n_capsules * int(ev["len"])] = True
    outside = bits(sp[~inside]) != bits(np.full(1, SENTINEL_F32))[0]
    assert not outside.any(), f"{int(outside.sum())} floats outside the event blocks overwritten (first at {base + int(np.flatnonzero(~inside)[np.argmax(outside)])})"
    return sp


def emitter_gains64(irs):
    """normalize_irs (synthesize.py:404-428) in float64: g[n] = 1 / mean_c(||h_{n,c}|| + tiny)."""
    norms = np.sqrt(np.sum(np.asarray(irs, dtype=np.float64) ** 2, axis=2))        # (C, N)
    return 1.0 / np.mean(norms + TINY64, axis=0)


def stream_signal(pl, s, clip):
    """The float64 weighted clip of stream s: gain * envelope(t) * a(t), the envelope W[q+1] win(r) + W[q] (1 - win(r)) of the
    stream's frame weights (1 for a static stream; W past its last frame is 0)."""
    st = pl.streams[s]
    a = np.asarray(clip, dtype=np.float64)
    x = a * float(np.float32(st["gain"]))
    if int(st["w_off"]) >= 0 and int(st["w_len"]) > 0:
        w = pl.wtab[int(st["w_off"]): int(st["w_off"]) + int(st["w_len"])].astype(np.float64)
        t = np.arange(len(a))
        q, rr = t // pl.hop, t % pl.hop
        win = np.sin(np.pi * rr / (2 * pl.hop)) ** 2
        wq = np.where(q < len(w), w[np.minimum(q, len(w) - 1)], 0.0)
        wq1 = np.where(q + 1 < len(w), w[np.minimum(q + 1, len(w) - 1)], 0.0)
        x = x * (wq + (wq1 - wq) * win)
    return x                        # NOT cut to the stream's blocks: a window the planner left out would show


def render64(pl, i, clip, irs, gains):
    """Event i's raw (C, len) render in float64 by direct convolution, truncated to len, zero from valid_len on."""
    ev = pl.events[i]
    C, n, valid = pl.n_capsules, int(ev["len"]), int(ev["valid_len"])
    out = np.zeros((C, n))
    if int(ev["n_streams"]) == 0:                   # dry: the clip tiled over the capsules, times the stream's gain
        out[:] = np.asarray(clip, dtype=np.float64) * float(np.float32(pl.streams[int(ev["stream0"])]["gain"]))
        return out, np.zeros(C), 0.0
    term = 0.0                                      # the largest single product |x(t)| |g h(tau)| of the convolution
    scale = np.zeros(C)                             # (sum_s max_j ||x_s window j||^2 sum_p g^2 ||h_p||^2)^(1/2): the error model's weight
    B = pl.block
    for s in range(int(ev["stream0"]), int(ev["stream0"]) + int(ev["n_streams"])):
        x = stream_signal(pl, s, clip)
        nn = int(pl.streams[s]["emitter"])
        g = float(np.float32(gains[nn]))
        pad = np.concatenate([np.zeros(B), x, np.zeros(2 * B)])
        wn = max(float(np.linalg.norm(pad[j * B:(j + 2) * B])) for j in range(len(pad) // B - 1))
        term = max(term, float(np.abs(x).max()) * g * float(np.abs(irs[:, nn]).max()))
        for c in range(C):
            h = irs[c, nn].astype(np.float64) * g
            out[c] += sp_signal.oaconvolve(x, h)[:n] if len(h) > 1 else (x * h[0])[:n]
            hp = np.linalg.norm(np.pad(h, (0, -len(h) % B)).reshape(-1, B), axis=1)
            scale[c] += wn * wn * float(np.sum(hp * hp))
    out[:, valid:] = 0.0
    return out, np.sqrt(scale), term


def render_bound(B, P, scale):
    """Per-sample bound of one overlap-save output sample y[t] = sum_p irfft(X_(k-p) H_p)[t].

    Worst case (Cauchy-Schwarz through the three transforms): |dy| <= (3 log2 2B + P + c) u sum_p ||x window|| ||h_p||.  For
    random 2B-sample windows that is 4e-4 of the peak at B = 16384 (||x window|| ~ sqrt(2B/3) ~ 100): looser than the contract,
    so it cannot hold the kernels to a tenth of it (check_render asserts that tenth on the error directly).  The test uses the rounding-error model instead (Higham, Accuracy and
    Stability of Numerical Algorithms, 2nd ed., sections 3.5 and 24.1): every rounding is an independent error of at most u
    relative, zero mean.  A radix-2 level of a transform of length N = 2B adds at most 6 such errors to each output (the complex
    product by the twiddle: two roundings per component through fma; the twiddle's own rounding; the butterfly's add), and
    there are log2 N + 1 levels with the real (un)packing, so each transform's error has rms <= sqrt(6 (log2 N + 1)) u times
    the rms of its output; the spectral
    product and the P-term accumulate add 2 + P more, the float32 emitter gain, clip gain and envelope 8.  The inverse transform
    (1/N) sum_k dY_k e^(...) spreads the spectral error evenly: the error of one sample has standard deviation
        sigma <= u sqrt((18 (log2 N + 1) + P + 10 + (2 log2 N)^2) / N) * sum_p ||x window|| ||h_p||,
    where the (2 log2 N)^2 is the twiddle table's share: every transform reads the same table, so its rounding (<= u per entry,
    correctly rounded: run_twiddles) does not average out between a forward and the inverse transform, and is counted in
    amplitude over the 2 log2 N passes of the pair (without it, delta IRs at B = 16384 on gfx950 reach 1.33x the bound).  It
    is a sum of thousands of independent terms, so it is normal to a good approximation; 8 sigma is exceeded with
    probability 1e-15 per sample.  The P partitions' products come from different signal windows and different IR transforms,
    so their errors are independent too and add in quadrature: sum_p ||x window|| ||h_p|| becomes
    max ||x window|| (sum_p ||h_p||^2)^(1/2), and the streams of a moving event (other windows, other IRs) in quadrature as well.
    Bound: 8 sigma."""
    N = 2 * B
    return 8.0 * U * np.sqrt((18 * (np.log2(N) + 1) + P + 10 + (2 * np.log2(N)) ** 2) / N) * scale


def prepare(r, pl, clips, irs, layout="plain", guards=True, normalize=True):
    batch = r.prepare(pl, clips, irs, normalize_irs=normalize)
    for desc in batch.descs:
        desc.flags = layout_flags(desc, layout)
    if guards:
        sentinel_spatial(r, batch)
    return batch


def check_render(r, batch, clips, irs, family, partials=True):
    """Raw ``spatial`` of every event against ``render64``; guard bands; exact zeros from valid_len on; the partial statistics
    per (event, capsule, block) against float64 statistics of the kernel's own output.  Returns the float64 renders."""
    pl = batch.plan
    B, C = pl.block, pl.n_capsules
    res = batch.result()
    sp = check_guards(r, batch)
    gains = download(r, batch.bufs["emitter_gain"], max(pl.n_emitters, 1)).astype(np.float64)
    base = spatial_base(pl)
    outs = []
    for i in range(len(pl.events)):
        ev = pl.events[i]
        n, valid = int(ev["len"]), int(ev["valid_len"])
        got = sp[int(ev["out_off"]) - base: int(ev["out_off"]) - base + C * n].reshape(C, n)
        want, scale, term = render64(pl, i, clips[i], irs, gains)
        assert np.isfinite(got).all(), (family, i)
        if valid < n:       # pad_or_truncate_audio's zeros: +0.0, bit for bit
            assert not bits(got[:, valid:]).any(), (family, i, "padding is not +0.0")
        peak = float(np.abs(want).max())
        if int(ev["n_streams"]) == 0:
            np.testing.assert_array_equal(got, want.astype(np.float32), err_msg=str((family, i)))
        elif peak > 1e-9 * float(scale.max()):     # below that: float64 noise of an exactly silent result
            err = np.abs(got.astype(np.float64) - want)
            bound = render_bound(B, pl.n_partitions, scale)[:, None]
            # a tenth of the contract, asserted on the error itself: 1e-5 of the peak -- of the largest single product where the
            # output only catches the edge of the signal (a delay that keeps two samples of a long clip has a small peak).  The
            # model bound is per sample and position-aware, but for 21..26 flat partitions at B >= 4096 it reaches 1.7e-5 of
            # the peak, so it alone would not hold the kernels to the tenth.
            cap = max(peak, term)
            worst = int(np.argmax((err / bound).reshape(-1)))
            record(f"render {family} (err / bound)", float((err / bound).reshape(-1)[worst]), 1.0)
            record(f"render {family} (err / peak)", float(err.max()) / cap, 1e-5)
        else:               # an exactly silent result (a delta past the clip): only the transforms' rounding noise
            record(f"render {family} silent (err / bound)", float(np.max(np.abs(got) / render_bound(B, pl.n_partitions, scale)[:, None])), 1.0)
        if partials:
            K = int(ev["n_blocks"])
            pb = int(ev["part_base"])      # this event's entries alone: part_base may lie anywhere in a large buffer
            pp = download(r, batch.bufs["partials"][4 * pb: 4 * (pb + C * K)]).reshape(C, K, 4)
            x = np.abs(np.pad(got.astype(np.float64), ((0, 0), (0, K * B - n))).reshape(C, K, B))
            np.testing.assert_array_equal(pp[..., 1], x.max(axis=2).astype(np.float32), err_msg=f"{family} partial max, event {i}")
            s64 = x.sum(axis=2)
            g = gamma(sum_depth(B))
            sum_err = np.abs(pp[..., 0] - s64)
            record(f"partial sum|x| (err / gamma_d sum)", float(np.max(sum_err / np.maximum(g * s64, TINY64))), 1.0)
            assert not pp[..., 2].any(), (family, i, "non-finite count")
        outs.append(got)
    return res, outs


# ----------------------------------------------------------------------------- 2. IR energies and emitter gains
def gain_irs(ir_len, C, N, seed, edge=None):
    rng = np.random.default_rng(seed)
    h = rng.standard_normal((C, N, ir_len)).astype(np.float32)
    if edge == "all_zero":
        h[:] = 0
    elif edge == "some_zero":
        h[::2] = 0
    elif edge == "denormal":
        h = (np.sign(h) * np.float32(1e-41)).astype(np.float32)
    elif edge == "nan":
        h[C // 2, 0, ir_len // 2] = np.nan
    return h


def energy_batch(r, h, log2_block, flags=0):
    """One static event per IR column, one-sample clips: the batch the energy pass and the gains run on."""
    C, N, L = h.shape
    specs = [planning.EventSpec(n_samples=1, n_emitters=1, snr=10.0, emitter0=n) for n in range(N)]
    pl = planning.plan_batch(specs, C, L, SR, log2_block=log2_block)
    batch = r.prepare(pl, [np.ones(1, np.float32)] * N, h)
    for desc in batch.descs:
        desc.flags = layout_flags(desc, "plain") | flags
    return batch


def run_emitter_gains(r, log2_block, ir_len, C, N=2, edge=None, seed=0, layout="plain"):
    """ir_energy (al_ir_spectra) against float64 partition sums of h^2; emitter_gain (al_emitter_gains) against float64
    C / sum_c (sqrt(sum_p e_(c,p)) + tiny) of the kernel's own energies (<= 1 ulp: one rounding of a float64 value, whose
    summation order may differ) and against the float64 gains of h itself (relative gamma_d / 2 + 2u: sqrt halves the
    energies' relative error)."""
    B = 1 << log2_block
    h = gain_irs(ir_len, C, N, seed, edge)
    batch = energy_batch(r, h, log2_block)
    batch.descs[0].flags = layout_flags(batch.descs[0], layout)
    batch.run(stages=["al_ir_spectra", "al_emitter_gains"])
    P = batch.plan.n_partitions
    e = download(r, batch.bufs["ir_energy"], N * C * P).reshape(N, C, P).astype(np.float64)
    g = download(r, batch.bufs["emitter_gain"], N).astype(np.float64)
    h64 = h.astype(np.float64)
    hp = np.pad(h64, ((0, 0), (0, 0), (0, P * B - ir_len))).reshape(C, N, P, B)
    e64 = np.transpose(np.sum(hp * hp, axis=3), (1, 0, 2))
    if edge == "nan":
        assert np.isnan(g[0]) and not np.isnan(g[1:]).any(), g
        return
    if edge == "denormal":      # 1e-41 squared underflows float32: every energy exactly 0
        assert not e.any(), e[e != 0][:4]
        e64 = np.zeros_like(e64)
    rel = np.abs(e - e64) / np.maximum(e64, TINY64)
    ok = e64 > 0
    if ok.any():
        record("ir_energy (rel err / gamma_d)", float(rel[ok].max()) / gamma(sum_depth(B)), 1.0)
    assert not e[~ok].any()
    own = C / np.sum(np.sqrt(np.sum(e, axis=2)) + TINY64, axis=1)
    own32 = np.where(own <= FLT_MAX, own, 0.0).astype(np.float32)
    if edge in ("all_zero", "denormal"):
        assert not bits(g.astype(np.float32)).any(), (edge, g)     # gain exactly +0.0: zeros stay zeros
        return
    ul = float(np.max(np.abs(g - own32.astype(np.float64)) / np.spacing(own32).astype(np.float64)))
    record("emitter gain vs its own energies (ulp)", ul, 1.0)
    want = emitter_gains64(h)
    record("emitter gain vs float64 gains (rel err / bound)",
           float(np.max(np.abs(g - want) / want)) / (gamma(sum_depth(B)) / 2 + 2 * U), 1.0)
    assert np.isfinite(g).all()


def run_emitter_gains_flags(r, log2_block, ir_len, C):
    """AL_FLAG_NO_IR_NORM: every gain exactly 1, from both the single-GPU and the from-sums mode."""
    h = gain_irs(ir_len, C, 2, 5)
    batch = energy_batch(r, h, log2_block, flags=_hip.FLAG_NO_IR_NORM)
    batch.run(stages=["al_ir_spectra", "al_emitter_gains"])
    assert_bits_equal(download(r, batch.bufs["emitter_gain"], 2), np.ones(2, np.float32), "NO_IR_NORM")
    batch.run(stages=["al_ir_spectra", "al_emitter_norm_sums"])
    r.lib.call("al_emitter_gains_from_sums", ct.byref(batch.descs[0]), C, r.mem.stream())
    assert_bits_equal(download(r, batch.bufs["emitter_gain"], 2), np.ones(2, np.float32), "NO_IR_NORM from sums")


def run_emitter_gains_sharded(r, log2_block, ir_len, C, split, edge=None):
    """The capsule-sharded path: capsules [0, split) and [split, C) as two batches, al_emitter_norm_sums on each (mode 1: the
    float32 sum of float64-accumulated norms), the two sums added on the host in float32 (the all-reduce), then
    al_emitter_gains_from_sums with total_capsules = C (mode 2).  Against float64 C / sum_c(||h_c|| + tiny): three float32
    roundings (two shard sums, their sum) plus the final one, and sqrt's half of the energies' gamma_d."""
    B = 1 << log2_block
    h = gain_irs(ir_len, C, 2, 11, edge)
    sums = []
    for lo, hi in ((0, split), (split, C)):
        b = energy_batch(r, np.ascontiguousarray(h[lo:hi]), log2_block)
        b.run(stages=["al_ir_spectra", "al_emitter_norm_sums"])
        sums.append(download(r, b.bufs["emitter_gain"], 2).astype(np.float32))
    total = (sums[0] + sums[1]).astype(np.float32)
    put(r, b.bufs["emitter_gain"], total)
    r.lib.call("al_emitter_gains_from_sums", ct.byref(b.descs[0]), C, r.mem.stream())
    g = download(r, b.bufs["emitter_gain"], 2).astype(np.float64)
    if edge in ("all_zero", "denormal"):
        assert not bits(g.astype(np.float32)).any(), g
        return
    try:
        r.lib.call("al_emitter_gains_from_sums", ct.byref(b.descs[0]), hi - lo - 1, r.mem.stream())
    except _hip.HipError as exc:
        assert "total_capsules" in str(exc)
    else:
        raise AssertionError("al_emitter_gains_from_sums accepted total_capsules < n_capsules")
    want = emitter_gains64(h)
    record("sharded emitter gain (rel err / bound)", float(np.max(np.abs(g - want) / want)) / (gamma(sum_depth(B)) / 2 + 4 * U), 1.0)


# ----------------------------------------------------------------------------- 3. spectra, plain layout
def packed_rfft(x, B):
    """float64 rfft of a 2B-sample window as the kernels store it: B complex, bin 0 = (DC, Nyquist)."""
    X = np.fft.rfft(x, n=2 * B)
    out = X[:B].copy()
    out[0] = complex(X[0].real, X[B].real)
    return out


def run_spectra(r, log2_block, C=2, seed=0):
    """hspec and xspec of a static event (clip gain and a device clip_scale folded in) and of a moving event's streams against
    float64 rfft of the zero-padded IR partition / the weighted signal window.  Bound per block: 2 (log2 2B + 1) eps of the
    block spectrum's peak (kernel_edges.py's FFT bound), plus the weighting's float32 roundings (gain x clip_scale x envelope:
    4 u of the window's l1 norm, which bounds the peak of the spectrum's perturbation)."""
    B = 1 << log2_block
    rng = np.random.default_rng(300 + log2_block + seed)
    Lir = 3 * B - 5
    La = 3 * B + 7
    a0 = rng.uniform(-1, 1, La).astype(np.float32)
    a1 = rng.uniform(-1, 1, La + 900).astype(np.float32)
    h = rng.standard_normal((C, 4, Lir)).astype(np.float32)
    specs = [planning.EventSpec(n_samples=La, n_emitters=1, snr=10.0, emitter0=0, gain=0.75),
             planning.EventSpec(n_samples=La + 900, n_emitters=3, snr=10.0, emitter0=1, is_moving=True, duration=(La + 900) / SR)]
    pl = planning.plan_batch(specs, C, Lir, SR, log2_block=log2_block)
    from audiblelight_amd import engine

    clips = [engine.ClipSource(host=a0, n=La, prescale=-1.5, normalize=True), a1]
    batch = r.prepare(pl, clips, h, emitter_parts=np.full(4, pl.n_partitions, np.int32))
    for desc in batch.descs:
        desc.flags = layout_flags(desc, "plain")
    batch.run(stages=["al_ir_spectra", "al_signal_spectra"])
    P = pl.n_partitions
    hs = download(r, batch.bufs["hspec"], 4 * C * P * 2 * B).astype(np.float64).reshape(4, C, P, B, 2)
    hs = hs[..., 0] + 1j * hs[..., 1]
    bound = 2 * (np.log2(2 * B) + 1) * EPS
    for n in range(4):
        for c in range(C):
            for p in range(P):
                want = packed_rfft(h[c, n, p * B:(p + 1) * B].astype(np.float64), B)
                record(f"hspec (err / peak)", peak_error(hs[n, c, p], want), bound)
    clip_scale = download(r, batch.bufs["clip_scale"], 2).astype(np.float64)
    want_cs = np.float32(-1.5) / (np.float32(1.5) * np.abs(a0).max() + np.finfo(np.float32).tiny)
    assert abs(clip_scale[0] - want_cs) <= abs(want_cs) * EPS, (clip_scale[0], want_cs)
    xs = download(r, batch.bufs["xspec"], pl.xspec_blocks * 2 * B).astype(np.float64).reshape(-1, B, 2)
    xs = xs[..., 0] + 1j * xs[..., 1]
    for s in range(len(pl.streams)):
        st = pl.streams[s]
        ev = int(st["event"])
        x = stream_signal(pl, s, clips[ev].host if ev == 0 else a1)
        if ev == 0:
            x = x * float(np.float32(clip_scale[0]))
        pad = np.concatenate([np.zeros(B), x, np.zeros(3 * B)])
        for jj in range(int(st["n_j"])):
            j = int(st["j_lo"]) + jj
            w = pad[j * B:(j + 2) * B]
            want = packed_rfft(w, B)
            got = xs[int(st["xspec_base"]) + jj]
            peak = float(np.abs(want).max())
            if peak == 0:
                assert not np.abs(got).any()
                continue
            err = float(np.abs(got - want).max())
            record("xspec (err / bound)", err / (bound * peak + 4 * U * float(np.abs(w).sum())), 1.0)


# ----------------------------------------------------------------------------- 4. render output
def delta_irs(C, N, Lir, delays):
    h = np.zeros((C, N, Lir), dtype=np.float32)
    for n, d in enumerate(delays):
        h[:, n, d] = 1.0
    return h


def run_delta_render(r, log2_block, P, delays, clip_lens, layout="plain", C=2, seed=0, odd=True):
    """h = delta at d on every capsule (||h_c|| = 1, emitter gain exactly 1): the exact output is the clip shifted by d,
    truncated to len.  One static event per (delay, clip length); guard bands around every (C, len) block."""
    B = 1 << log2_block
    Lir = P * B
    rng = np.random.default_rng(900 + seed)
    specs, clips, col = [], [], 0
    for d in delays:
        for n in clip_lens:
            a = rng.uniform(-1, 1, n).astype(np.float32)
            clips.append(a)
            specs.append(planning.EventSpec(n_samples=n, n_emitters=1, snr=10.0, emitter0=col))
            col += 1
    h = delta_irs(C, col, Lir, [d for d in delays for _ in clip_lens])
    pl = make_plan(specs, C, Lir, log2_block, guards=True, odd=odd)
    batch = prepare(r, pl, clips, h, layout)
    batch.run()
    gains = download(r, batch.bufs["emitter_gain"], col)
    assert_bits_equal(gains, np.ones(col, np.float32), "delta IR gains")
    _, outs = check_render(r, batch, clips, h, f"delta IR {layout}")
    i = 0
    for d in delays:
        for n in clip_lens:
            exact = np.zeros(n)
            if d < n:
                exact[d:] = clips[i][: n - d]
            # the same bound as check_render's, with ||h_p|| = 1 and ||x window|| <= sqrt(2B) (|x| <= 1)
            assert float(np.abs(outs[i] - exact[None, :]).max()) <= render_bound(B, P, np.sqrt(2.0 * B)), (d, n)
            i += 1
    return batch


def run_delta_clip(r, log2_block, P, C=2, layout="plain", seed=0):
    """The mirror case: clip = delta at block seams (0, B-1, B, B+1, 2B-1), random flat IR: the output is the IR shifted."""
    B = 1 << log2_block
    Lir = P * B - 3
    rng = np.random.default_rng(1200 + seed)
    seams = [0, B - 1, B, B + 1, 2 * B - 1]
    n = 3 * B + 5
    clips, specs = [], []
    for k, s in enumerate(seams):
        a = np.zeros(n, np.float32)
        a[s] = 1.0
        clips.append(a)
        specs.append(planning.EventSpec(n_samples=n, n_emitters=1, snr=10.0, emitter0=k))
    h = rng.uniform(-1, 1, (C, len(seams), Lir)).astype(np.float32)
    pl = make_plan(specs, C, Lir, log2_block, guards=True, odd=True)
    batch = prepare(r, pl, clips, h, layout)
    batch.run()
    check_render(r, batch, clips, h, f"delta clip {layout}")


def flat_scene(log2_block, P, C, seed, kinds, n_j=None):
    """Random clips and FLAT random IRs (no decay: the last partition weighs as much as the first).  kinds: 'static', 'dry',
    'moving' (cross-fade over 3 emitters; n_j picks a duration whose streams span that many signal blocks)."""
    B = 1 << log2_block
    rng = np.random.default_rng(4000 + 31 * seed + P)
    Lir = P * B - int(rng.integers(0, B // 2))
    specs, clips, col = [], [], 0
    for kind in kinds:
        if kind == "moving":
            n = int((n_j - 0.75) * B) if n_j else int(rng.integers(2 * B, 5 * B))    # n_j: the longest stream's blocks
            n = max(n, 700)
            specs.append(planning.EventSpec(n_samples=n, n_emitters=3, snr=float(rng.uniform(5, 30)), emitter0=col,
                                            is_moving=True, duration=n / SR))
            col += 3
        else:
            n = int(rng.integers(1, 4 * B))
            specs.append(planning.EventSpec(n_samples=n, n_emitters=1 if kind == "static" else 0, snr=float(rng.uniform(5, 30)),
                                            emitter0=col))
            col += 1 if kind == "static" else 0
        clips.append(rng.uniform(-1, 1, n).astype(np.float32))
    h = rng.uniform(-1, 1, (C, max(col, 1), Lir)).astype(np.float32)
    return specs, clips, h, Lir


def run_flat_render(r, log2_block, P, layout="plain", C=2, seed=0, kinds=("static", "moving", "dry", "static"), n_j=None):
    specs, clips, h, Lir = flat_scene(log2_block, P, C, seed, kinds, n_j)
    pl = make_plan(specs, C, Lir, log2_block, guards=True, odd=True)
    if n_j is not None:     # AL_SPARSE_MAX_NJ = 6 is the longest stream the sliding-window accumulate takes; 7 goes to the tile kernel
        mv = pl.events["n_streams"] > 1
        assert int(pl.streams["n_j"].max()) == n_j and bool((pl.events["reserved"][mv] == 1).all()) == (n_j <= 6), pl.streams
    batch = prepare(r, pl, clips, h, layout)
    batch.run()
    check_render(r, batch, clips, h, f"flat IR {layout}")
    return batch


def run_emitter_parts_boundary(r, log2_block, reach, layout="plain", C=2):
    """A sliding-window moving event whose streams carry a delta at partition p of their IR.  p is chosen so that partition p of
    the last stream reaches exactly the last kept block (j_lo + p == n_blocks - 1: the delta must show in that block) or one
    block past it (j_lo + p == n_blocks: the partition is trimmed from the transform and the block must not contain it)."""
    B = 1 << log2_block
    n = 4 * B + 300
    spec = planning.EventSpec(n_samples=n, n_emitters=2, snr=10.0, emitter0=0, is_moving=True, duration=n / SR)
    P = 6
    Lir = P * B
    pl0 = planning.plan_batch([spec], C, Lir, SR, log2_block=log2_block)
    ev = pl0.events[0]
    K = int(ev["n_blocks"])
    assert int(ev["reserved"]) == 1
    st = pl0.streams[int(ev["stream0"]) + 1]
    p = K - 1 - int(st["j_lo"]) + (0 if reach == "last" else 1)
    assert 0 <= p < P, p
    h = np.zeros((C, 2, Lir), np.float32)
    h[:, :, 0] = 1.0                    # both emitters: a delta at 0 (normalisation) ...
    h[:, 1, p * B + 5] = 0.5            # ... and the probe at partition p of the last stream's IR
    clip = np.random.default_rng(77).uniform(-1, 1, n).astype(np.float32)
    pl = make_plan([spec], C, Lir, log2_block, guards=True)
    parts = pl.emitter_parts()
    assert parts is not None and parts[1] == (p + 1 if reach == "last" else p), (parts, p)
    batch = prepare(r, pl, [clip], h, layout)
    batch.run()
    _, outs = check_render(r, batch, [clip], h, f"emitter_parts {reach}")
    # the probe's contribution to the last block, alone: render with and without it in float64
    gains = download(r, batch.bufs["emitter_gain"], 2).astype(np.float64)
    h0 = h.copy()
    h0[:, 1, p * B + 5] = 0.0
    want0, scale, _ = render64(pl, 0, clip, h0, gains)       # the same (kernel's) gains, the probe left out
    last = slice((K - 1) * B, min(K * B, int(ev["valid_len"])))
    probe = float(np.abs(outs[0][:, last] - want0[:, last]).max()) / float(render_bound(B, P, scale).max())
    if reach == "last":     # the probe's share of the last block is far above the rounding bound ...
        assert probe > 100, ("the partition that reaches the last kept block is missing", probe)
    else:                   # ... and, one partition further on, nothing but rounding
        assert probe <= 1, ("a partition past the last kept block leaked into it", probe)


# ----------------------------------------------------------------------------- 5. level law
def level_law64(sum_abs, mx, rows, n, snr, ref_db):
    """apply_snr o db_to_multiplier (synthesize.py:40-68, chained at :594-599) in float64: s1 = snr / max(max|x|, 1e-15), the
    mean |s1 x| over rows * len samples, s2 = 10^((ref_db + snr) / 20) / (mean + tiny); event_scale = s1 s2 as float32 saturated
    at +-FLT_MAX (NaN stays NaN)."""
    s1 = snr / max(mx, 1e-15)
    mean = abs(s1) * sum_abs / (rows * n)
    s2 = 10.0 ** ((ref_db + snr) / 20.0) / (mean + TINY64)
    with np.errstate(over="ignore"):
        v = s1 * s2
    return s2, (np.float32(np.clip(v, -FLT_MAX, FLT_MAX)) if v == v else np.float32(v))


def run_level_law(r, log2_block, C, n_samples, snrs, ref_dbs, silent=None, total_extra=0, layout="plain"):
    """Static events rendered through every stage; then event_stats and event_scale against the float64 law.

    The reductions: sum|x| against the float64 sum of the kernel's own output (gamma_d per block; the float64 sum of the float32
    block partials adds n 2^-53), max|x| exact, non-finite count 0.  The law: evaluated in float64 from the kernel's OWN stats
    (so only the law is under test here) and rounded once: <= 1 ulp of float32 (numpy's and the device's pow may differ by an
    ulp of float64).  silent: 'clip' (zero clip) or 'ir' (zero IRs): event_scale = FLT_MAX and the scaled output exactly 0.
    total_extra > 0: al_event_stats + al_event_levels_from_stats with total_capsules = C + total_extra."""
    B = 1 << log2_block
    rng = np.random.default_rng(500 + log2_block + C)
    specs, clips = [], []
    for k, (snr, ref_db) in enumerate(zip(snrs, ref_dbs)):
        n = n_samples
        specs.append(planning.EventSpec(n_samples=n, n_emitters=1, snr=snr, emitter0=k, ref_db=ref_db))
        a = rng.uniform(-1, 1, n).astype(np.float32)
        if silent == "clip" and k == 0:
            a[:] = 0
        clips.append(a)
    h = (rng.standard_normal((C, len(specs), B + 3)) * np.exp(-np.arange(B + 3) / B)).astype(np.float32)
    if silent == "ir":
        h[:, 0] = 0
    pl = make_plan(specs, C, B + 3, log2_block, guards=True)
    batch = prepare(r, pl, clips, h, layout)
    stages = ["al_forward_spectra", "al_emitter_gains", "al_spectral_mac", "al_block_synthesis"]
    total = C + total_extra
    if total_extra:
        batch.run(stages=stages + ["al_event_stats"])
        r.lib.call("al_event_levels_from_stats", ct.byref(batch.descs[0]), total, r.mem.stream())
    else:
        batch.run(stages=stages + ["al_event_levels"])
    res = batch.result()
    sp = check_guards(r, batch)
    stats = res.stats()
    scales = download(r, batch.bufs["event_scale"], len(specs))
    for i, ev in enumerate(pl.events):
        n = int(ev["len"])
        x = np.abs(sp[int(ev["out_off"]): int(ev["out_off"]) + C * n].astype(np.float64))
        s64 = float(x.sum())
        blocks = int(ev["n_blocks"])
        assert C * blocks == C * -(-n // B)
        assert stats[i, 1] == float(x.max()), (stats[i, 1], x.max())
        assert stats[i, 2] == 0
        bound = gamma(sum_depth(B)) * s64 + C * blocks * 2.0 ** -53 * s64
        if s64 > 0:
            record("event sum|x| (err / bound)", abs(stats[i, 0] - s64) / bound, 1.0)
        else:
            assert stats[i, 0] == 0
        s2, want = level_law64(stats[i, 0], stats[i, 1], total, n, float(np.float32(specs[i].snr)), float(np.float32(specs[i].ref_db)))
        got = scales[i]
        if silent and i == 0:
            assert got == np.float32(FLT_MAX) and want == np.float32(FLT_MAX), (got, want)
            scaled = res.spatial_audio(0, dtype=np.float32)
            assert not bits(scaled).any(), "silent event's scaled output is not exactly 0"
            continue
        record("event_scale (ulp)", float(abs(float(got) - float(want)) / float(np.spacing(np.abs(want)))), 1.0)
        assert abs(stats[i, 3] - s2) <= 4 * 2.0 ** -52 * abs(s2), (stats[i, 3], s2)


# ----------------------------------------------------------------------------- 6. mixdown
class MixCase:
    """Hand-built al_mix tables: slots (src, len, start, count, rows, event) in insertion order, tile lists from them."""

    def __init__(self, n_capsules, n_samples, tile=4096):
        self.C, self.T, self.tile = n_capsules, n_samples, tile
        self.slots = []

    def add(self, src, length, start, count, rows, event):
        self.slots.append((int(src), int(length), int(start), int(count), int(rows), int(event)))

    def tables(self):
        n_tiles = -(-self.T // self.tile)
        lists = [[] for _ in range(n_tiles)]
        for q, (_, _, start, count, _, _) in enumerate(self.slots):
            lo, hi = max(start, 0), min(start + count, self.T)
            for t in range(lo // self.tile, (hi - 1) // self.tile + 1) if hi > lo else ():
                lists[t].append(q)
        ptr = np.zeros(n_tiles + 1, np.int32)
        ptr[1:] = np.cumsum([len(x) for x in lists])
        ev = np.array([q for x in lists for q in x] or [0], np.int32)
        cols = list(zip(*self.slots)) if self.slots else [[0]] * 6
        return dict(tile_ptr=ptr, tile_events=ev, slot_src=np.array(cols[0], np.int64), slot_len=np.array(cols[1], np.int32),
                    slot_start=np.array(cols[2], np.int32), slot_count=np.array(cols[3], np.int32),
                    slot_rows=np.array(cols[4], np.int32), slot_event=np.array(cols[5], np.int32), n_tiles=n_tiles)


def mixdown64(tabs, C, T, spatial, scales, prefill=None, amb=None, amb_scale=None):
    """The scene in float64 and, per sample, the sum of |terms| and the number of additions (for the gamma bound)."""
    out = np.zeros((C, T)) if prefill is None else prefill.astype(np.float64).copy()
    mag = np.abs(out).copy()
    adds = np.zeros((C, T)) if prefill is None else np.ones((C, T))
    if amb is not None:
        term = (amb.astype(np.float64) * amb_scale.astype(np.float64)[:, None])
        out += term
        mag += np.abs(term)
        adds += 1
    for q in range(len(tabs["slot_start"])):
        start, count, rows, ln = int(tabs["slot_start"][q]), int(tabs["slot_count"][q]), int(tabs["slot_rows"][q]), int(tabs["slot_len"][q])
        if count <= 0:
            continue
        sc = float(scales[int(tabs["slot_event"][q])])
        i = np.arange(max(0, -start), min(count, T - start))
        for c in range(min(rows, C)):
            x = spatial[int(tabs["slot_src"][q]) + c * ln + i].astype(np.float64) * sc
            out[c, start + i] += x
            mag[c, start + i] += np.abs(x)
            adds[c, start + i] += 1
    return out, mag, adds


def run_mixdown(r, case, spatial, scales, accumulate=False, ambience=False, prefill_seed=None, family="mixdown"):
    C, T = case.C, case.T
    tabs = case.tables()
    sp_dev = r.mem.upload(spatial.astype(np.float32))
    sc_dev = r.mem.upload(np.asarray(scales, np.float32))
    prefill = np.random.default_rng(prefill_seed or 1).uniform(-1, 1, (C, T)).astype(np.float32) if accumulate else None
    scene = Guarded(r, C * T, init=prefill if accumulate else None)
    amb = amb_scale = None
    keep = []
    if ambience:
        amb = np.random.default_rng(3).standard_normal((C, T)).astype(np.float32)
        amb_scale = np.linspace(0.25, 2.0, C).astype(np.float32)
        keep += [r.mem.upload(amb), r.mem.upload(amb_scale)]
    dev = {k: r.mem.upload(v) for k, v in tabs.items() if k != "n_tiles"}
    p = r.mem.ptr
    desc = _hip.AlMix(n_capsules=C, n_samples=T, tile=case.tile, n_tiles=tabs["n_tiles"], accumulate=1 if accumulate else 0,
                      tile_ptr=p(dev["tile_ptr"]), tile_events=p(dev["tile_events"]), slot_src=p(dev["slot_src"]),
                      slot_len=p(dev["slot_len"]), slot_start=p(dev["slot_start"]), slot_count=p(dev["slot_count"]),
                      slot_rows=p(dev["slot_rows"]), slot_event=p(dev["slot_event"]), spatial=p(sp_dev), event_scale=p(sc_dev),
                      scene=scene.ptr, ambience=p(keep[0]) if ambience else None, ambience_scale=p(keep[1]) if ambience else None)
    r.lib.call("al_mixdown", ct.byref(desc), r.mem.stream())
    got = scene.get().reshape(C, T).astype(np.float64)
    want, mag, adds = mixdown64(tabs, C, T, spatial, np.asarray(scales, np.float32), prefill, amb, amb_scale)
    # each term is one float32 product (u relative) and each addition one rounding: |err| <= gamma_(adds + 1) sum|terms|
    bound = gamma(adds + 1) * mag
    err = np.abs(got - want)
    assert (err <= bound).all(), (family, float(np.max(err - bound)), np.unravel_index(np.argmax(err - bound), err.shape))
    nz = bound > 0
    record(f"{family} (err / gamma bound)", float(np.max(err[nz] / bound[nz])) if nz.any() else 0.0, 1.0)
    untouched = ~nz & (adds == 0)
    assert not bits(got[untouched].astype(np.float32)).any() if not accumulate else True
    return got, desc, dev, keep, sp_dev, sc_dev, scene


def mix_spatial(n_events, C, length, seed):
    """Back-to-back (C, len) event blocks at ODD offsets inside one spatial buffer."""
    rng = np.random.default_rng(seed)
    offs, off = [], 1
    for _ in range(n_events):
        offs.append(off)
        off += C * length + 3            # odd + even: the next block starts at an odd offset again... alternately
    sp = rng.uniform(-1, 1, off + 8).astype(np.float32)
    return sp, offs


def run_mixdown_slots(r, T, C=2, seed=0, accumulate=False, ambience=False, rows_cut=False):
    """Slots at 0, at tile seams +-1..3, ending at T and running past it, count < len, counts 0..5, 40+ slots over one tile
    (insertion order), odd sources; rows_cut: slot_rows < C for every other slot (rows >= slot_rows untouched by that slot)."""
    rng = np.random.default_rng(600 + seed)
    L = 700
    n_ev = 60
    sp, offs = mix_spatial(n_ev, C, L, seed)
    scales = rng.uniform(0.1, 3.0, n_ev).astype(np.float32)
    case = MixCase(C, T)
    starts = [0, T - 1, T - L, T - L // 2]
    for seam in range(4096, T, 4096):
        starts += [seam + d for d in (-3, -2, -1, 1, 2, 3)]
        if len(starts) > 40:
            break
    q = 0
    for s in starts:
        if 0 <= s < T:
            count = min(T - s, L) if q % 3 else min(T - s + 5, L)          # some run past T (the kernel must clip them)
            count = min(count, L)
            case.add(offs[q % n_ev], L, s, count if q % 4 else max(count - 17, 0), C - 1 if rows_cut and q % 2 else C, q % n_ev)
            q += 1
    for k in range(6):                     # counts 0..5 at an unaligned start
        case.add(offs[k] + 2, L, min(37 + 5 * k, T - 1), min(k, T - min(37 + 5 * k, T - 1)), C, k)
    for k in range(42):                    # more than 40 slots over one tile, in insertion order
        s = min(100 + 13 * k, max(T - 1, 0))
        case.add(offs[k % n_ev] + (k % 3), L, s, min(L - 3, T - s), C, (k * 7) % n_ev)
    return run_mixdown(r, case, sp, scales, accumulate, ambience, family=f"mixdown T={T}")


def run_mixdown_planned(r, T, C=2, seed=0):
    """Tables from al_plan_mixdown, with scene times that start before 0 (clamped by the planner), at 0 and past the end."""
    rng = np.random.default_rng(700 + seed)
    L = 1500
    n_ev = 8
    sp, offs = mix_spatial(n_ev, C, L, seed)
    dur = T / SR
    starts = [-0.01, 0.0, dur - 0.005, 4096 / SR + 1 / SR, dur / 2, dur / 3 + 0.5 / SR, dur - 1 / SR, 0.003]
    ends = [s + L / SR for s in starts]
    mp = planning.plan_mixdown(starts, ends, [L] * n_ev, [C] * n_ev, offs, list(range(n_ev)), dur, SR, C)
    case = MixCase(C, mp.n_samples)
    for q in range(len(mp.slot_start)):
        if q < len(mp.slot_start) and (mp.slot_count[q] > 0 or len(mp.slot_start) > 1):
            case.add(mp.slot_src[q], mp.slot_len[q], mp.slot_start[q], mp.slot_count[q], mp.slot_rows[q], mp.slot_event[q])
    tabs = case.tables()
    np.testing.assert_array_equal(tabs["tile_ptr"], mp.tile_ptr)        # the planner's tile lists are the hand-built ones
    scales = rng.uniform(0.1, 3.0, n_ev).astype(np.float32)
    return run_mixdown(r, case, sp, scales, family="mixdown planned")


def run_mixdown_refusals(r):
    C, T = 2, 5000
    case = MixCase(C, T)
    sp, offs = mix_spatial(1, C, 10, 0)
    case.add(offs[0], 10, 0, 10, C, 0)
    _, desc, dev, keep, sp_dev, sc_dev, scene = run_mixdown(r, case, sp, [1.0])

    def refused(what, **changes):
        d = type(desc).from_buffer_copy(desc)
        for k, v in changes.items():
            setattr(d, k, v)
        try:
            r.lib.call("al_mixdown", ct.byref(d), r.mem.stream())
        except _hip.HipError as exc:
            assert what in str(exc), (what, str(exc))
        else:
            raise AssertionError(f"al_mixdown accepted {changes}")

    refused("tile must be 4096", tile=2048, n_tiles=3)
    refused("n_tiles", n_tiles=1)
    refused("16-byte aligned", scene=scene.ptr + 4)
    amb = r.mem.upload(np.zeros(C * T, np.float32))
    amb_s = r.mem.upload(np.ones(C, np.float32))
    refused("fused ambience", accumulate=1, ambience=r.mem.ptr(amb), ambience_scale=r.mem.ptr(amb_s))
    scene.get()            # the refusals wrote nothing
