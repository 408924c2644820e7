"""Standalone shake families: every barrier kernel that no rendered batch launches, called through the C ABI from any build of the library
(TEST INFRASTRUCTURE; tests/test_gpu_shake_standalone.py runs them through the product library and tests/shake.py's variants).

tests/test_gpu_shake.py's eleven FAMILIES render batches, so they reach the transforms, the accumulate kernels, the level kernels and
the mixdown.  The kernels below are only ever launched by a direct call of their entry point: the FX scans (k_fx_sos, k_fx_delay,
k_fx_chorus_fb, k_fx_phaser, k_fx_deemph), the block reductions (k_row_stats, k_peak_scale, k_clip_scales, k_ambience_scales) and the
LDS transpose of k_encode_frames.  Each family is a function ``(renderer) -> Outputs`` (a dict name -> ndarray) that calls the
scenario runners of tests/kernel_edges.py, tests/filter_fx_cases.py and tests/delay_mod_fx_cases.py: every launch writes into a
Guarded buffer and is compared with its float64 restatement there, so on EVERY library a family runs on it has met its reference
bound and left its guard bands intact before two libraries are compared with each other.

``Outputs.eps[name]`` is the absolute form of the bound the runner has just asserted, as far as it can be known from the output itself
(the runner keeps its reference to itself): a runner that asserts max|got - ref| <= rel * max|ref| implies max|ref| <= max|got| / (1 -
rel), hence |got - ref| <= rel * max|got| / (1 - rel) =: eps.  Two libraries that both passed differ by at most eps_a + eps_b.

Shapes: chosen from the kernels so that every barrier site executes, with ragged ends; the comment beside each row restates the
launch geometry.  Sizes: under AL_SHAKE=3 wave 0 sleeps ~10 us after every barrier, so every launch stays far below 50 000 barriers
(the largest here: k_fx_chorus_fb at fs = 16000, 2 * ceil(9605 / 16) = 1202; k_fx_sos with 16 sections, 1 + 4 * (2 + 3 * 16) + 22 * 16 = 553).
"""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np

from audiblelight_amd import _hip
from tests import delay_mod_fx_cases as dmc
from tests import filter_fx_cases as ffc
from tests import kernel_edges as ke
from tests import mac_regimes as mr

# ----------------------------------------------------------------------------- the barrier inventory
# Every __global__ kernel of the product library whose code object executes a workgroup barrier (any instantiation of a template
# holds an `s_barrier`), and the shake family that launches it: a row of tests/test_gpu_shake.py's FAMILIES (render stage) or one of
# FAMILIES below.  tests/test_host_logic.py::test_every_barrier_kernel_has_a_shake_family builds the left column from the
# disassembly of the built library and fails on any kernel that is not here.
BARRIER_KERNELS = {
    # render stage: one-transform layout (B = 1024), split layout (B = 8192), quad layout (B = 16384).  A render's al_forward_spectra
    # launches k_forward_spectra_{split,quad16} in those two layouts (kernel traces of the eleven families); the separate IR / signal
    # kernels run only when a host calls al_ir_spectra and al_signal_spectra itself: the separate_spectra family below
    "k_ir_spectra": "static_lds_ring_B10",
    "k_signal_spectra": "static_lds_ring_B10",
    "k_block_synthesis": "static_lds_ring_B10",
    "k_ir_spectra_split": "separate_spectra",
    "k_signal_spectra_split": "separate_spectra",
    "k_forward_spectra_split": "moving_window_split_B13",
    "k_block_synthesis_split": "static_regs_split_B13",
    "k_ir_spectra_quad16": "separate_spectra",
    "k_signal_spectra_quad16": "separate_spectra",
    "k_forward_spectra_quad16": "quad16_moving_trimmed",
    "k_block_synthesis_quad16": "quad16_static",
    # render stage: accumulate
    "k_spectral_mac_static": "static_regs_split_B13",
    "k_spectral_mac_static_lds": "static_lds_ring_B10",
    "k_spectral_mac_static_glds": "static_lds_dma_B10",
    "k_spectral_mac_moving": "moving_window_B10_P13",
    # standalone
    "k_fx_sos": "fx_sos",
    "k_fx_delay": "fx_delay",
    "k_fx_chorus_fb": "fx_chorus",
    "k_fx_phaser": "fx_phaser",
    "k_fx_deemph": "fx_deemph",
    "k_row_stats": "stats",
    "k_peak_scale": "stats",
    "k_clip_scales": "stats",
    "k_encode_frames": "encode",
}
# __syncthreads() in the source, no s_barrier in the code object: the workgroup is ONE wave (__launch_bounds__(64)), for which hipcc
# drops the instruction -- there is no second wave to be out of step with.  Launched by its family all the same.
ONE_WAVE_BARRIER_KERNELS = {"k_ambience_scales": "stats"}
# No barrier and no LDS: a schedule perturbation cannot change them, so no family has to launch them.
NO_BARRIER_NO_LDS = ("k_mixdown", "k_big_pass", "k_noise_pack", "k_noise_unpack", "k_blue_pre", "k_blue_kernel", "k_blue_mul",
                     "k_blue_post", "k_stft_pack", "k_stft_take_half", "k_tv_stft_mac", "k_istft_pack", "k_istft_ola",
                     "k_resample_poly", "k_pack_irs", "k_pack_ragged", "k_fx_pointwise", "k_fx_chorus_ff", "k_frame_shuffle",
                     "k_wrap_copy")

LLVM_BIN = "/opt/rocm/llvm/bin"


def kernel_inventory(lib_path=None):
    """{kernel base name: (instantiations with an s_barrier, instantiations, largest static LDS bytes)} of the gfx950 code objects
    embedded in the library, from `llvm-objdump --offloading` (extraction), `llvm-objdump -d` and `llvm-readelf --notes`."""
    lib_path = lib_path or _hip.DEFAULT_LIB
    inventory = {}
    with tempfile.TemporaryDirectory() as tmp:
        copy = os.path.join(tmp, "lib.so")        # llvm-objdump writes the extracted bundles beside its input
        shutil.copy(lib_path, copy)
        subprocess.check_call([os.path.join(LLVM_BIN, "llvm-objdump"), "--offloading", copy], stdout=subprocess.DEVNULL)
        objects = [os.path.join(tmp, f) for f in sorted(os.listdir(tmp)) if "amdgcn" in f]
        assert objects, "no gfx950 code object in " + lib_path
        for obj in objects:
            barrier, current = {}, None
            for line in subprocess.check_output([os.path.join(LLVM_BIN, "llvm-objdump"), "-d", obj]).decode().splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    current = m.group(1)
                    barrier[current] = False
                elif current and re.search(r"\bs_barrier\b", line):
                    barrier[current] = True
            lds, pending = {}, None
            for line in subprocess.check_output([os.path.join(LLVM_BIN, "llvm-readelf"), "--notes", obj]).decode().splitlines():
                m = re.search(r"\.group_segment_fixed_size:\s*(\d+)", line)
                if m:
                    pending = int(m.group(1))
                m = re.search(r"\.name:\s*(\S+)", line)
                if m and pending is not None:
                    lds[m.group(1)], pending = pending, None
            kernels = sorted(lds)                  # the metadata names exactly the __global__ functions
            assert kernels and all(k in barrier for k in kernels), "disassembly and metadata disagree on the kernels"
            stray = [sym for sym, has in barrier.items() if has and sym not in lds]
            assert not stray, f"a barrier in a device function that was not inlined into its kernels: {stray}"
            names = subprocess.check_output(["c++filt"] + kernels).decode().splitlines()
            for sym, name in zip(kernels, names):
                base = re.sub(r"^void ", "", name).split("<")[0].split("(")[0].split("::")[-1]
                had = inventory.get(base, (0, 0, 0))
                inventory[base] = (had[0] + barrier[sym], had[1] + 1, max(had[2], lds[sym]))
    return inventory


# ----------------------------------------------------------------------------- outputs and their bounds
class Outputs(dict):
    """name -> ndarray, with eps[name]: the elementwise absolute bound the runner asserted against its reference (see the module)."""

    def __init__(self):
        super().__init__()
        self.eps = {}

    def peak(self, name, got, rel):
        """the runner asserted max|got - ref| <= rel * max|ref|"""
        self[name] = got
        self.eps[name] = rel * float(np.max(np.abs(got.astype(np.float64)))) / (1.0 - rel)

    def relative(self, name, got, rel):
        """the runner asserted |got - ref| <= rel * |ref| per element"""
        self[name] = got
        self.eps[name] = rel * np.abs(got.astype(np.float64)) / (1.0 - rel)

    def ulp(self, name, got, n_ulp):
        """the runner asserted |got - ref| <= n_ulp (<= 1) float32 spacings at |ref|; ref is then within one spacing of got, so its
        spacing is at most twice got's"""
        self[name] = got
        with np.errstate(over="ignore"):       # a scale clamped to FLT_MAX: its spacing overflows to inf
            self.eps[name] = n_ulp * 2.0 * np.spacing(np.abs(got)).astype(np.float64)

    def roundings(self, name, got):
        """a render output, whose runner asserts bits against another launch sequence of the SAME library, not a float64 bound: between
        two builds the render stage's own bound holds, tests/test_gpu_shake.py within_roundings (2e-6 of the peak, half of it here)"""
        self[name] = got
        self.eps[name] = 1e-6 * float(np.max(np.abs(got.astype(np.float64))))

    def exact(self, name, got):
        """the runner asserted equality with its reference"""
        self[name] = got
        self.eps[name] = 0.0


# ----------------------------------------------------------------------------- the families
def sos_geometry(n):
    """(tiles per sweep, live runs) of k_fx_sos, restating sos_run_length (csrc/al_sos.h)."""
    run = -(-(-(-n // 1024)) // 16) * 16
    return -(-min(run, n) // 16), -(-n // run)


# (n, sections, in place, interior shift).  Sections: 1 = no fused next section (sos_sweep's nxt == nullptr on the only write sweep),
# 3, 16 = the cap of one launch.  Barriers: 1 + tiles * (2 + 3 K) + 22 K.
SOS_ROWS = [
    (50001, 1, False, 0),     # run 64: 4 tiles per sweep, 782 live runs (run 781 has 17 samples), threads 782.. own nothing
    (50001, 3, True, 0),      #   the same in place: every tile read completely before any of it is written back
    (50001, 16, False, 1),    #   16 sections, interior one element off alignment
    (50001, 16, True, 0),
    (1025, 1, True, 1),       # run 16: 1 tile, 65 live runs (run 64 has 1 sample), in place and off alignment
    (1025, 3, False, 0),
    (1025, 16, False, 0),
]


def fx_sos(r):
    out = Outputs()
    for n, k, in_place, shift in SOS_ROWS:
        got = ffc.run_sos_edges(r, n, k, shift=shift, in_place=in_place)
        out.peak(f"n{n}_k{k}_{'in' if in_place else 'out'}_shift{shift}", got, 1e-6 * k)
    return out


def delay_geometry(n, D):
    """(G, P, workgroups) of k_fx_delay, restating delay_plan (csrc/al_delayfx.h)."""
    pow2 = lambda v: 1 << max(int(v) - 1, 0).bit_length()
    K = (n - 1) // D if 1 <= D < n else 0
    if K == 0:
        return 1024, 1, -(-n // 1024)
    G = pow2(D) if D < 64 else 64
    P = min(pow2(-(-K // 16)), 1024 // G)
    return G, P, -(-D // G)


# (n, D, shift, (G, P, workgroups)): G residues x P runs per workgroup; the scan takes log2 P steps of two barriers + one.
DELAY_ROWS = [
    (20011, 1, 0, (1, 1024, 1)),        # K = 20010: P at its cap, ten scan steps, every read of carry[tid - d] with d >= 64 crosses waves
    (20011, 3, 1, (4, 256, 1)),         # K = 6670: eight steps; residue 3 of the 4 does not exist (threads with g = 3 idle)
    (20011, 63, 0, (64, 16, 1)),        # K = 317: four steps, each wave one run; residue 63 does not exist
    (20011, 64, 1, (64, 16, 1)),        # K = 312: G = 64 exactly
    (624147, 4801, 0, (64, 16, 76)),    # K = 130: P at its cap, 76 workgroups, the last with 1 residue of 64
    (5000, 5000, 1, (1024, 1, 5)),      # D >= n, K = 0: no chain, no scan step, the one barrier
]


def fx_delay(r):
    out = Outputs()
    for n, D, shift, geometry in DELAY_ROWS:
        assert delay_geometry(n, D) == geometry, (n, D, delay_geometry(n, D))
        out.peak(f"n{n}_D{D}", dmc.run_delay_edges(r, n, D, fb=0.7, mix=0.4, shift=shift), dmc.TOL)
    return out


def chorus_block(fs, depth, centre_ms):
    """B of k_fx_chorus_fb, restating al_fx_chorus."""
    tau_max = float(np.ceil(110.0 * fs / 1000.0))
    lowest = min(max(1.0, centre_ms - 10.0 * depth) * fs / 1000.0, tau_max)
    return int(min(max(np.floor(lowest) - 1.0, np.floor(fs / 1000.0)), 1024, 16384 - tau_max - 2.0))


# (n, fs, rate, depth, centre ms, feedback, mix, shift, B).  k_fx_chorus_fb walks ceil(n / B) blocks, two barriers each.
CHORUS_ROWS = [
    (9605, 16000, 6.0, 0.8, 1.5, 0.5, 0.5, 1, 16),       # the smallest block: 601 blocks, the last of 5; tau between the 1 ms floor and 9.5 ms
    (9605, 48000, 3.0, 1.0, 5.0, 0.6, 0.5, 0, 48),       # 10 depth lfo + centre spans -5 .. 15 ms: reaches the 1 ms floor and leaves it
    (20003, 48000, 2.0, 0.5, 20.0, 0.9, 0.4, 1, 719),    # a block wider than eleven waves: 28 blocks, the last of 590
    (20003, 48000, 2.0, 1.0, 105.0, 0.7, 0.6, 0, 1024),  # B at its cap; tau reaches the 110 ms clamp
    (9605, 48000, 3.0, 1.0, 5.0, 0.0, 0.5, 1, 48),       # feedback 0: k_fx_chorus_ff, no barrier -- must stay bit-identical
]


def fx_chorus(r):
    out = Outputs()
    for n, fs, rate, depth, centre, fb, mix, shift, block in CHORUS_ROWS:
        assert chorus_block(fs, depth, centre) == block and n % block, (fs, depth, centre, chorus_block(fs, depth, centre))
        got = dmc.run_chorus_case(r, n, fs, rate, depth, centre, fb, mix, shift=shift)
        out.peak(f"n{n}_fs{fs}_B{block}_fb{fb}", got, dmc.TOL)
    return out


# (n, feedback).  512 runs of a multiple of 4 samples; four batches of 128 maps, three barriers each, whatever n.
PHASER_ROWS = [
    (511, 0.0),               # run 4: 128 live runs (the last of 3 samples), batches 1..3 hold identity maps only
    (511, 0.7),
    (4 * 512 * 3 + 2, 0.0),   # run 16 (ceil(6146 / 512) = 13 rounded up to 4s): 385 live runs, the last of 2 samples
    (4 * 512 * 3 + 2, 0.7),
]


def fx_phaser(r):
    out = Outputs()
    for n, fb in PHASER_ROWS:
        out.peak(f"n{n}_fb{fb}", dmc.run_phaser_case(r, n, 48000, 8.0, 0.9, 900.0, fb, 0.6, shift=n % 2), dmc.TOL)
    return out


def fx_deemph(r):
    """1024 runs of ceil(n / 1024) samples, thread 0 chains the carries between the kernel's two barriers.  n = 1 never reaches the
    kernel: al_fx_apply refuses an emphasis filter on fewer than two samples (the extrapolation term needs x[1]), on every build --
    asserted, and the smallest clip that launches, n = 2 (two live runs of one sample), runs in its place; then n = 1025 (run 2:
    513 live runs, the last of 1 sample) and 60000 (run 59: 1017 live runs)."""
    out = Outputs()
    c = 0.97
    one = ke.Guarded(r, 1)
    try:
        ke.fx(r, _hip.FX_DEEMPH, r.mem.ptr(ke.dev(r, np.ones(1, np.float32))), one.ptr, 1, c)
    except _hip.HipError as exc:
        assert "n >= 2" in str(exc), exc
    else:
        raise AssertionError("al_fx_apply ran a de-emphasis on one sample")
    out.exact("n1_refused_untouched", one.get())
    for n in (2, 1025, 60000):
        out.peak(f"n{n}", ke.run_fx_deemphasis(r, n, c, shift=n % 2), 2.0 * ke.EPS / (1.0 - float(np.float32(c))))
    return out


def stats(r):
    """k_row_stats (two block_reduce3 over one `red`, a barrier between): 3 rows x 3 chunks, the last chunk of 5 samples, so 251 of its
    256 threads reduce zeros; k_peak_scale / k_clip_scales (1024 threads, 16 waves into `red`) on ragged lengths; k_ambience_scales."""
    out = Outputs()
    got = ke.run_row_stats(r, 3, 2 * 16384 + 5)
    out.relative("row_stats_sums", got[:, [0, 3]], 40.0 * ke.EPS)
    out.exact("row_stats_max_count", got[:, [1, 2]])
    for n in (1023, 4097):
        out.ulp(f"peak_scale_n{n}", ke.run_peak_scale(r, n), 0.5 + 1e-6)
    out.ulp("clip_scales", ke.run_clip_scales(r, [2, 1023, 1024, 1025, 5, 4097, 33333]), 0.5 + 1e-6)
    for rows in (3, 65):
        out.ulp(f"ambience_scales_rows{rows}", ke.run_ambience_scales(r, rows, 4801), 1.0)
    return out


# (capsules, format, store path); T = 64 * 3 + 7: three full tiles of 64 samples and one of 7
ENCODE_ROWS = [
    (8, _hip.FRAMES_PCM16, "16-byte stores of 8 int16"),
    (4, _hip.FRAMES_F32, "float4 stores"),
    (5, _hip.FRAMES_PCM16, "scalar stores"),
    (5, _hip.FRAMES_F32, "scalar stores"),
]


def encode(r):
    out = Outputs()
    for capsules, fmt, _ in ENCODE_ROWS:
        out.exact(f"C{capsules}_fmt{fmt}", ke.run_encode(r, capsules, 64 * 3 + 7, fmt, shift=0 if capsules in (4, 8) else 1))
    return out


def separate_spectra(r):
    """The one render-stage family here: al_ir_spectra + al_signal_spectra as two launches (k_ir_spectra_split / k_signal_spectra_split
    at B = 8192, k_ir_spectra_quad16 / k_signal_spectra_quad16 at B = 16384), which no batch of tests/test_gpu_shake.py reaches; the
    runner holds the event audio bit for bit against the merged launch of the same library."""
    out = Outputs()
    for log2_block in (13, 14):
        out.roundings(f"B{1 << log2_block}", mr.run_separate_forward_launches(r, log2_block))
    return out


FAMILIES = {"separate_spectra": separate_spectra, "fx_sos": fx_sos, "fx_delay": fx_delay, "fx_chorus": fx_chorus, "fx_phaser": fx_phaser, "fx_deemph": fx_deemph,
            "stats": stats, "encode": encode}

# Families whose shaken builds were observed to render the product library's bits (profiles/r08_shake_standalone.txt): asserted
# equal from then on, so a later one-ulp drift between the builds is seen.  The others may differ by FMA contraction (the sleep loops
# split basic blocks; profiles/r06_shake_diag.txt) and are held to the sum of their reference bounds.
BIT_IDENTICAL_TO_PRODUCT = ("fx_sos", "fx_delay", "fx_chorus", "fx_phaser", "fx_deemph", "stats", "encode")


def same(a, b):
    return all(np.array_equal(ke.bits(a[k]), ke.bits(b[k])) for k in a) and a.keys() == b.keys()


def worst_ratio(a, b):
    """max over outputs of |a - b| / (eps_a + eps_b); 0 where both are equal (eps may be 0 there), inf where they differ and eps is 0."""
    worst = 0.0
    for k in a:
        with np.errstate(invalid="ignore"):    # Inf - Inf
            diff = np.abs(a[k].astype(np.float64) - b[k].astype(np.float64))
        diff = np.where(ke.bits(a[k]) == ke.bits(b[k]), 0.0, diff)       # NaN / Inf that agree bit for bit
        bound = np.broadcast_to(np.asarray(a.eps[k] + b.eps[k], dtype=np.float64), diff.shape)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(diff == 0.0, 0.0, diff / bound)
        worst = max(worst, float(np.max(ratio)) if ratio.size else 0.0)
    return worst
