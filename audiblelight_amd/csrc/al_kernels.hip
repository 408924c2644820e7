// C ABI of the MI355X synthesis path (gfx950 only): every extern "C" entry point of include/audiblelight_hip.h that launches
// device code, each one argument validation plus launch.  No kernel and no launch planning lives here: kernels, their device
// helpers and the host-side choice of instantiation and grid are in the per-domain headers included below (al_mac.h accumulate,
// al_levels.h level scalars, al_mixdown.h, al_rows.h, al_clipfx.h / al_sos.h / al_delayfx.h / al_dynfx.h / al_stretchfx.h FX, al_ingest.h, al_ism.h, al_bigfft.h, al_stft.h);
// the FFT kernels of the pipeline are the other translation unit, al_transforms.hip.  See DESIGN.md for the data layout and
// per-kernel rooflines.
//
// Pipeline per batch of events (uniformly partitioned overlap-save, block B = M = 2^LOG2M):
//   k_ir_spectra      H[n,c,p]  = rFFT_2B([h[pB:(p+1)B], 0])        + partial sum of h^2
//   k_emitter_gains   g[n]      = 1 / mean_c(||h_{n,c}|| + tiny)      (normalize_irs)
//   k_signal_spectra  X[s,j]    = rFFT_2B(gain * env_s * a[(j-1)B:(j+1)B])
//   k_spectral_mac    Y[e,c,k]  = sum_s g[n_s] sum_p X[s,k-p] * H[n_s,c,p]
//   k_block_synthesis x[e,c,kB:(k+1)B] = irFFT_2B(Y[e,c,k])[B:2B]    + partial |x| statistics
//   k_event_levels    scale[e]  = apply_snr o db_to_multiplier from sum|x|, max|x|
//   k_mixdown         scene[c,t] (+)= sum_e scale[e] * x[e,c,t-start_e]
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "al_common.h"
#include "al_bigfft.h"
#include "al_clipfx.h"
#include "al_delayfx.h"
#include "al_dynfx.h"
#include "al_fft.h"
#include "al_ingest.h"
#include "al_ism.h"
#include "al_levels.h"
#include "al_mac.h"
#include "al_mixdown.h"
#include "al_rows.h"
#include "al_sos.h"
#include "al_stft.h"
#include "al_stretchfx.h"

// ====================================================================== C ABI
namespace {
thread_local char g_err[256] = "";

int fail(int code, const char *msg) {
  snprintf(g_err, sizeof(g_err), "%s", msg);
  return code;
}

int check_error(hipError_t e, const char *what) {
  if (e != hipSuccess) {
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return AL_E_HIP;
  }
  return AL_OK;
}

int check_launch(const char *what) { return check_error(hipGetLastError(), what); }

int check_batch(const al_batch *b) {
  if (!b) return fail(AL_E_BADARG, "null batch");
  if (b->struct_size != (int32_t)sizeof(al_batch) || b->abi_version != AL_ABI_VERSION)
    return fail(AL_E_BADARG, "al_batch was built against another version of audiblelight_hip.h (struct_size / abi_version)");
  if (b->log2_block < AL_MIN_LOG2_BLOCK || b->log2_block > AL_MAX_LOG2_BLOCK)
    return fail(AL_E_UNSUPPORTED, "log2_block must be in [10, 14]");
  if (b->n_capsules <= 0 || b->n_events < 0 || b->n_streams < 0) return fail(AL_E_BADARG, "bad batch sizes");
  if ((b->ir_stride_c & 3) || (b->ir_stride_n & 3)) return fail(AL_E_BADARG, "IR strides must be multiples of 4 floats");
  if (((uintptr_t)b->ir & 15) != 0) return fail(AL_E_BADARG, "IR base must be 16-byte aligned");
  if (b->n_emitters > 0 && b->n_partitions != ((b->ir_len + (1 << b->log2_block) - 1) >> b->log2_block))
    return fail(AL_E_BADARG, "n_partitions != ceil(ir_len / B)");
  if (b->hop <= 0) return fail(AL_E_BADARG, "hop must be positive");
  return AL_OK;
}

}  // namespace

extern "C" {

const char *al_last_error(void) { return g_err; }
int al_abi_version(void) { return AL_ABI_VERSION; }

int64_t al_twiddle_bytes(int log2_block) {
  if (log2_block < AL_MIN_LOG2_BLOCK || log2_block > AL_MAX_LOG2_BLOCK) return -1;
  return (int64_t)sizeof(float) * 2 * ((int64_t)1 << log2_block);
}

int al_twiddle_init(float *twiddle, int log2_block, al_stream_t stream) {
  if (!twiddle || al_twiddle_bytes(log2_block) < 0) return fail(AL_E_BADARG, "bad twiddle arguments");
  const int m = 1 << log2_block;
  hipLaunchKernelGGL(al::k_twiddle_init, dim3((m + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<float2 *>(twiddle), m);
  return check_launch("k_twiddle_init");
}

int al_ir_spectra(const al_batch *b, al_stream_t stream) {
  if (int rc = check_batch(b)) return rc;
  if (b->n_emitters <= 0) return AL_OK;
  return check_error(al::launch_ir_spectra(b, (hipStream_t)stream), "k_ir_spectra");
}

int al_emitter_gains(const al_batch *b, al_stream_t stream) {
  if (int rc = check_batch(b)) return rc;
  if (b->n_emitters <= 0) return AL_OK;
  hipLaunchKernelGGL(al::k_emitter_gains, dim3(b->n_emitters), dim3(64), 0, (hipStream_t)stream, *b, 0, 0);
  return check_launch("k_emitter_gains");
}

int al_emitter_norm_sums(const al_batch *b, al_stream_t stream) {
  if (int rc = check_batch(b)) return rc;
  if (b->n_emitters <= 0) return AL_OK;
  hipLaunchKernelGGL(al::k_emitter_gains, dim3(b->n_emitters), dim3(64), 0, (hipStream_t)stream, *b, 1, 0);
  return check_launch("k_emitter_gains(sums)");
}

int al_emitter_gains_from_sums(const al_batch *b, int32_t total_capsules, al_stream_t stream) {
  if (int rc = check_batch(b)) return rc;
  if (total_capsules < b->n_capsules) return fail(AL_E_BADARG, "total_capsules < n_capsules");
  if (b->n_emitters <= 0) return AL_OK;
  hipLaunchKernelGGL(al::k_emitter_gains, dim3(b->n_emitters), dim3(64), 0, (hipStream_t)stream, *b, 2, total_capsules);
  return check_launch("k_emitter_gains(from sums)");
}

int al_forward_spectra(const al_batch *b, al_stream_t stream) {
  if (int rc = check_batch(b)) return rc;
  return check_error(al::launch_forward_spectra(b, (hipStream_t)stream), "k_forward_spectra");
}

int al_signal_spectra(const al_batch *b, al_stream_t stream) {
  if (int rc = check_batch(b)) return rc;
  if (b->n_streams <= 0 || b->max_nj <= 0) return AL_OK;
  return check_error(al::launch_signal_spectra(b, (hipStream_t)stream), "k_signal_spectra");
}

int al_spectral_mac_variant(const al_batch *b, int32_t *static_code, int32_t *moving_code) {
  if (int rc = check_batch(b)) return rc;
  if (!static_code || !moving_code) return fail(AL_E_BADARG, "null output");
  const al::MacPlan m = al::plan_mac(b);
  *static_code = m.static_code;
  *moving_code = m.moving ? m.moving->code : 0;
  return AL_OK;
}

int al_spectral_mac(const al_batch *b, al_stream_t stream_) {
  if (int rc = check_batch(b)) return rc;
  if (b->n_events <= 0 || b->n_emitters <= 0) return AL_OK;
  hipStream_t stream = (hipStream_t)stream_;
  const al::MacPlan m = al::plan_mac(b);
  if (al::static_mac_active(*b)) {
    if (!m.statics) return fail(AL_E_BADARG, "capsule-loop accumulate: bad partition tile");
    hipLaunchKernelGGL(m.statics->kernel, m.static_grid, dim3(m.statics->threads), 0, stream, *b);
    if (int rc = check_launch("k_spectral_mac_static")) return rc;
  }
  if (m.tile) {   // (not under AL_FLAG_ONLY_STATIC: every event went through the capsule loop)
    hipLaunchKernelGGL(m.tile->kernel, m.tile_grid, dim3(m.tile->threads), 0, stream, *b);
    if (int rc = check_launch("k_spectral_mac")) return rc;
  }
  if (m.moving) {
    hipLaunchKernelGGL(m.moving->kernel, m.moving_grid, dim3(m.moving->threads), 0, stream, *b);
    return check_launch("k_spectral_mac_moving");
  }
  return AL_OK;
}

int al_block_synthesis(const al_batch *b, al_stream_t stream) {
  if (int rc = check_batch(b)) return rc;
  if (b->n_events <= 0 || b->max_blocks <= 0) return AL_OK;
  return check_error(al::launch_block_synthesis(b, (hipStream_t)stream), "k_block_synthesis");
}

int al_event_levels(const al_batch *b, al_stream_t stream) {
  if (int rc = check_batch(b)) return rc;
  if (b->n_events <= 0) return AL_OK;
  hipLaunchKernelGGL(al::k_event_levels, dim3(b->n_events), dim3(64), 0, (hipStream_t)stream, *b, 0, 0);
  return check_launch("k_event_levels");
}

int al_event_stats(const al_batch *b, al_stream_t stream) {
  if (int rc = check_batch(b)) return rc;
  if (b->n_events <= 0) return AL_OK;
  hipLaunchKernelGGL(al::k_event_levels, dim3(b->n_events), dim3(64), 0, (hipStream_t)stream, *b, 1, 0);
  return check_launch("k_event_levels(stats)");
}

int al_event_levels_from_stats(const al_batch *b, int32_t total_capsules, al_stream_t stream) {
  if (int rc = check_batch(b)) return rc;
  if (total_capsules < b->n_capsules) return fail(AL_E_BADARG, "total_capsules < n_capsules");
  if (b->n_events <= 0) return AL_OK;
  hipLaunchKernelGGL(al::k_event_levels, dim3(b->n_events), dim3(64), 0, (hipStream_t)stream, *b, 2, total_capsules);
  return check_launch("k_event_levels(law)");
}

int al_render_batch(const al_batch *b, al_stream_t stream) {
  int rc;
  if ((rc = al_forward_spectra(b, stream))) return rc;
  if ((rc = al_emitter_gains(b, stream))) return rc;
  if ((rc = al_spectral_mac(b, stream))) return rc;
  if ((rc = al_block_synthesis(b, stream))) return rc;
  return al_event_levels(b, stream);
}

int al_mixdown(const al_mix *m, al_stream_t stream) {
  if (!m) return fail(AL_E_BADARG, "null mixdown descriptor");
  if (m->struct_size != (int32_t)sizeof(al_mix) || m->abi_version != AL_ABI_VERSION)
    return fail(AL_E_BADARG, "al_mix was built against another version of audiblelight_hip.h (struct_size / abi_version)");
  if (m->n_capsules <= 0 || m->n_samples <= 0 || m->tile <= 0) return fail(AL_E_BADARG, "bad mixdown arguments");
  if (m->tile != 4096) return fail(AL_E_BADARG, "mixdown tile must be 4096 samples");
  if (m->n_tiles != (m->n_samples + m->tile - 1) / m->tile) return fail(AL_E_BADARG, "n_tiles != ceil(n_samples / tile)");
  if (((uintptr_t)m->scene & 15) != 0) return fail(AL_E_BADARG, "scene buffer must be 16-byte aligned");
  if (m->ambience && (!m->ambience_scale || m->accumulate || ((uintptr_t)m->ambience & 15) != 0))
    return fail(AL_E_BADARG, "fused ambience needs ambience_scale, accumulate == 0 and a 16-byte aligned buffer");
  hipLaunchKernelGGL(al::k_mixdown, dim3(m->n_tiles, m->n_capsules), dim3(256), 0, (hipStream_t)stream, *m);
  return check_launch("k_mixdown");
}

int al_scale_rows(float *x, int64_t n, const float *scale, al_stream_t stream) {
  if (!x || !scale || n < 0) return fail(AL_E_BADARG, "bad scale arguments");
  if (n == 0) return AL_OK;
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(al::k_scale, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, (hipStream_t)stream, x, n, scale);
  return check_launch("k_scale");
}

int al_scale_rows_f64(float *x, int64_t n, const double *scale, al_stream_t stream) {
  if (!x || !scale || n < 0) return fail(AL_E_BADARG, "bad scale arguments");
  if (n == 0) return AL_OK;
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(al::k_scale_d, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, (hipStream_t)stream, x, n, scale);
  return check_launch("k_scale_d");
}

int al_clip_scales(const al_batch *b, const float *prescale, const int32_t *mode, al_stream_t stream) {
  if (int rc = check_batch(b)) return rc;
  if (!prescale || !mode || !b->clip_scale) return fail(AL_E_BADARG, "clip_scales needs prescale, mode and al_batch.clip_scale");
  if (b->n_events <= 0) return AL_OK;
  hipLaunchKernelGGL(al::k_clip_scales, dim3(b->n_events), dim3(1024), 0, (hipStream_t)stream, *b, prescale, mode,
                     const_cast<float *>(b->clip_scale));
  return check_launch("k_clip_scales");
}

int al_peak_scale(const float *x, int64_t n, float prescale, float *scale_out, al_stream_t stream) {
  if (!x || !scale_out || n <= 0) return fail(AL_E_BADARG, "bad peak_scale arguments");
  hipLaunchKernelGGL(al::k_peak_scale, dim3(1), dim3(1024), 0, (hipStream_t)stream, x, n, prescale, scale_out);
  return check_launch("k_peak_scale");
}

int al_axpy(float *y, const float *x, const float *a_dev, int64_t n, al_stream_t stream) {
  if (!x || !y || !a_dev || n < 0) return fail(AL_E_BADARG, "bad axpy arguments");
  if (n == 0) return AL_OK;
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(al::k_axpy, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, (hipStream_t)stream, y, x, a_dev, n);
  return check_launch("k_axpy");
}

int64_t al_row_stats_partials(int32_t rows, int64_t cols) {
  if (rows <= 0 || cols <= 0) return 0;
  return 4 * (int64_t)rows * ((cols + al::ROW_CHUNK - 1) / al::ROW_CHUNK);
}

int al_row_stats(const float *x, int32_t rows, int64_t cols, float *partials, double *out, al_stream_t stream) {
  if (!x || !partials || !out || rows <= 0 || cols <= 0) return fail(AL_E_BADARG, "bad row_stats arguments");
  const int nchunks = (int)((cols + al::ROW_CHUNK - 1) / al::ROW_CHUNK);
  if ((int64_t)nchunks * rows > 0x7fffffff) return fail(AL_E_BADARG, "row_stats: too many (row, chunk) pairs");
  hipLaunchKernelGGL(al::k_row_stats, dim3((unsigned)(nchunks * rows)), dim3(256), 0, (hipStream_t)stream, x, cols, partials);
  if (int rc = check_launch("k_row_stats")) return rc;
  hipLaunchKernelGGL(al::k_row_stats_final, dim3(rows), dim3(64), 0, (hipStream_t)stream, partials, nchunks, out);
  return check_launch("k_row_stats_final");
}

// ---- FX: the checks and derivations of every entry whose kernel a batched launch can run, shared by the single-clip entries and
// al_fx_batch_pack.  Each returns 0 with *job filled, or the error of the first bad argument.
namespace {
bool fx_ranges_overlap(const float *a, int64_t na, const float *b, int64_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + (uintptr_t)nb * sizeof(float) && pb < pa + (uintptr_t)na * sizeof(float);
}

bool fx_overlap(const float *a, const float *b, int64_t n) { return fx_ranges_overlap(a, n, b, n); }

// 0, or the error for the first bad argument
int fx_check(const char *fn, const float *src, const float *dst, int64_t n, const char *const *names, const double *vals,
             int count) {
  char msg[200];
  if (!src || !dst) {
    snprintf(msg, sizeof(msg), "%s: null pointer", fn);
    return fail(AL_E_BADARG, msg);
  }
  if (n < 1) {
    snprintf(msg, sizeof(msg), "%s: n must be >= 1", fn);
    return fail(AL_E_BADARG, msg);
  }
  if (fx_overlap(src, dst, n)) {
    snprintf(msg, sizeof(msg), "%s: dst overlaps src (out of place only)", fn);
    return fail(AL_E_BADARG, msg);
  }
  for (int i = 0; i < count; ++i) {
    if (!isfinite(vals[i]) || vals[i] < 0.0) {
      snprintf(msg, sizeof(msg), "%s: %s must be finite and >= 0", fn, names[i]);
      return fail(AL_E_BADARG, msg);
    }
    if (!strcmp(names[i], "feedback") && vals[i] >= 1.0) {
      snprintf(msg, sizeof(msg), "%s: feedback must be < 1 (unstable loop)", fn);
      return fail(AL_E_BADARG, msg);
    }
  }
  return AL_OK;
}

// al_fx_apply's checks of its clip arguments
int fx_apply_check(int op, const float *src, const float *dst, int64_t n) {
  if (!src || !dst || n <= 0) return fail(AL_E_BADARG, "bad fx arguments");
  if (op < AL_FX_GAIN || op > AL_FX_DEEMPH) return fail(AL_E_UNSUPPORTED, "unknown fx op");
  const bool out_of_place = (op == AL_FX_REVERSE || op == AL_FX_PREEMPH || op == AL_FX_DEEMPH);
  if (out_of_place && src == dst) return fail(AL_E_BADARG, "this fx op needs dst != src");
  if ((op == AL_FX_PREEMPH || op == AL_FX_DEEMPH) && n < 2) return fail(AL_E_BADARG, "emphasis filters need n >= 2");
  return AL_OK;
}

int deemph_prepare(const float *src, float *dst, int64_t n, float c, al::DeemphJob *job) {
  if (int rc = fx_apply_check(AL_FX_DEEMPH, src, dst, n)) return rc;
  *job = al::DeemphJob{src, dst, n, c};
  return AL_OK;
}

int sos_prepare(const float *src, float *dst, int64_t n, const double *sos, int32_t n_sections, al::SosJob *job) {
  if (!src || !dst || !sos) return fail(AL_E_BADARG, "al_fx_sos: null pointer");
  if (n < 1) return fail(AL_E_BADARG, "al_fx_sos: n must be >= 1");
  if (n_sections < 1 || n_sections > AL_SOS_MAX_SECTIONS)
    return fail(AL_E_BADARG, "al_fx_sos: n_sections must be in 1..AL_SOS_MAX_SECTIONS (16); split longer cascades");
  const int64_t run = al::sos_run_length(n);
  memset(job, 0, sizeof(*job));
  job->src = src;
  job->dst = dst;
  job->n = n;
  job->run = run;
  al::SosArgs &a = job->a;
  a.n_sections = n_sections;
  char msg[160];
  for (int k = 0; k < n_sections; ++k) {
    const double *row = sos + 6 * k;
    for (int i = 0; i < 6; ++i)
      if (!isfinite(row[i])) {
        snprintf(msg, sizeof(msg), "al_fx_sos: section %d has a non-finite coefficient", k);
        return fail(AL_E_BADARG, msg);
      }
    if (row[3] == 0.0) {
      snprintf(msg, sizeof(msg), "al_fx_sos: section %d has a0 == 0", k);
      return fail(AL_E_BADARG, msg);
    }
    const double c[5] = {row[0] / row[3], row[1] / row[3], row[2] / row[3], row[4] / row[3], row[5] / row[3]};
    for (int i = 0; i < 5; ++i)
      if (!isfinite(c[i])) {
        snprintf(msg, sizeof(msg), "al_fx_sos: section %d has a non-finite coefficient after division by a0", k);
        return fail(AL_E_BADARG, msg);
      }
    // both roots of z^2 + a1 z + a2 inside the unit circle (Jury): |a2| < 1 and |a1| < 1 + a2
    if (!(fabs(c[4]) < 1.0 && fabs(c[3]) < 1.0 + c[4])) {
      snprintf(msg, sizeof(msg), "al_fx_sos: section %d has a pole of magnitude >= 1 (unstable filter)", k);
      return fail(AL_E_BADARG, msg);
    }
    for (int i = 0; i < 5; ++i) a.c[k][i] = c[i];
    al::sos_transition_power(c[3], c[4], run, a.phi[k]);
  }
  return AL_OK;
}

// delay and modulation FX: out of place, every parameter finite and >= 0, feedback < 1
int chorus_prepare(const float *src, float *dst, int64_t n, double fs, double rate_hz, double depth, double centre_delay_ms,
                   double feedback, double mix, al::ChorusJob *job) {
  static const char *const names[] = {"fs", "rate_hz", "depth", "centre_delay_ms", "feedback", "mix"};
  const double vals[] = {fs, rate_hz, depth, centre_delay_ms, feedback, mix};
  if (int e = fx_check("al_fx_chorus", src, dst, n, names, vals, 6)) return e;
  const double tau_max = ceil(110.0 * fs / 1000.0);
  const double b_min = floor(fs / 1000.0);   // tau >= fs / 1000: the 1 ms floor of the delay
  if (!(b_min >= 1.0) || tau_max + b_min + 2.0 > (double)al::CHO_RING)
    return fail(AL_E_BADARG, "al_fx_chorus: fs out of range (1000 <= fs and ceil(0.11 fs) + floor(fs / 1000) + 2 <= 16384)");
  job->src = src;
  job->dst = dst;
  job->n = n;
  al::ChorusArgs &a = job->a;
  a.fs = fs;
  a.rate = rate_hz;
  a.depth10 = 10.0 * depth;
  a.centre_ms = centre_delay_ms;
  a.tau_max = tau_max;
  a.fb = feedback;
  const double m = mix < 1.0 ? mix : 1.0;   // JUCE's DryWetMixer clamps the proportion
  a.dry = 1.0 - m;
  a.wet = m;
  // B = floor of a lower bound of every tau_t, one sample short of it against rounding, never below the 1 ms floor
  const double lowest = fmin(fmax(1.0, centre_delay_ms - 10.0 * depth) * fs / 1000.0, tau_max);
  double b = floor(lowest) - 1.0;
  b = b > b_min ? b : b_min;
  b = b < (double)al::CHO_MAX_BLOCK ? b : (double)al::CHO_MAX_BLOCK;
  b = b < (double)al::CHO_RING - tau_max - 2.0 ? b : (double)al::CHO_RING - tau_max - 2.0;
  a.block = (int64_t)b;
  return AL_OK;
}

int phaser_prepare(const float *src, float *dst, int64_t n, double fs, double rate_hz, double depth, double centre_frequency_hz,
                   double feedback, double mix, al::PhaserJob *job) {
  static const char *const names[] = {"fs", "rate_hz", "depth", "centre_frequency_hz", "feedback", "mix"};
  const double vals[] = {fs, rate_hz, depth, centre_frequency_hz, feedback, mix};
  if (int e = fx_check("al_fx_phaser", src, dst, n, names, vals, 6)) return e;
  if (!(0.49 * fs > 20.0)) return fail(AL_E_BADARG, "al_fx_phaser: fs out of range (0.49 fs must exceed 20 Hz)");
  const double fmax_hz = fmin(20000.0, 0.49 * fs);
  job->src = src;
  job->dst = dst;
  job->n = n;
  job->run = al::phaser_run_length(n);
  al::PhaserArgs &a = job->a;
  a.fs = fs;
  a.rate = rate_hz;
  a.half_depth = 0.5 * depth;
  a.c = log10(centre_frequency_hz / 20.0) / log10(fmax_hz / 20.0);   // -inf at fc = 0: the LFO clamps it to 0
  a.log_ratio = log(fmax_hz / 20.0);
  a.fb = feedback;
  const double m = mix < 1.0 ? mix : 1.0;
  a.dry = 1.0 - m;
  a.wet = m;
  return AL_OK;
}
// dynamics FX: out of place; the checks both entries share, then the stages
constexpr double DYN_TWO_PI = 6.283185307179586476925286766559;

// cte(ms): the one-pole coefficient of a time constant, 0 below a microsecond (JUCE's BallisticsFilter)
double dyn_cte(double ms, double fs) { return ms < 1e-3 ? 0.0 : exp(-DYN_TWO_PI * 1000.0 / (ms * fs)); }

al::DynStage dyn_stage(double threshold_db, double ratio, double cA, double cR) {
  const double T = pow(10.0, threshold_db / 20.0);
  return al::DynStage{T, 1.0 / T, 1.0 / ratio - 1.0, cA, cR};
}

int dyn_check(const char *fn, const float *src, const float *dst, int64_t n, double fs, double threshold_db, bool limiter,
              double ratio, double attack_ms, double release_ms) {
  if (int e = fx_check(fn, src, dst, n, nullptr, nullptr, 0)) return e;
  char msg[200];
  const char *why = nullptr;
  if (!isfinite(fs) || !(fs > 0.0)) why = "fs must be finite and > 0";
  else if (!isfinite(threshold_db) || !(threshold_db > -200.0)) why = "threshold_db must be finite and > -200";
  else if (limiter && !(threshold_db < 100.0)) why = "threshold_db must be < 100";
  else if (!isfinite(ratio) || !(ratio >= 1.0)) why = "ratio must be finite and >= 1";
  else if (!isfinite(attack_ms) || attack_ms < 0.0) why = "attack_ms must be finite and >= 0";
  else if (!isfinite(release_ms) || release_ms < 0.0) why = "release_ms must be finite and >= 0";
  if (!why) return AL_OK;
  snprintf(msg, sizeof(msg), "%s: %s", fn, why);
  return fail(AL_E_BADARG, msg);
}

int compressor_prepare(const float *src, float *dst, int64_t n, double fs, double threshold_db, double ratio, double attack_ms,
                       double release_ms, al::DynJob *job) {
  if (int e = dyn_check("al_fx_compressor", src, dst, n, fs, threshold_db, false, ratio, attack_ms, release_ms)) return e;
  memset(job, 0, sizeof(*job));
  job->src = src;
  job->dst = dst;
  job->n = n;
  job->n_stages = 1;
  job->st[0] = dyn_stage(threshold_db, ratio, dyn_cte(attack_ms, fs), dyn_cte(release_ms, fs));
  job->st[1] = job->st[0];   // not walked
  job->out_gain = 1.0;
  job->ceiling = INFINITY;
  return AL_OK;
}

// JUCE's dsp::Limiter: a fixed first compressor, the caller's second one (attack 0.001 ms: cA = 0), the make-up gain, the clamp
int limiter_prepare(const float *src, float *dst, int64_t n, double fs, double threshold_db, double release_ms, al::DynJob *job) {
  if (int e = dyn_check("al_fx_limiter", src, dst, n, fs, threshold_db, true, 1000.0, 0.0, release_ms)) return e;
  memset(job, 0, sizeof(*job));
  job->src = src;
  job->dst = dst;
  job->n = n;
  job->n_stages = 2;
  job->st[0] = dyn_stage(-10.0, 4.0, dyn_cte(2.0, fs), dyn_cte(200.0, fs));
  job->st[1] = dyn_stage(threshold_db, 1000.0, 0.0, dyn_cte(release_ms, fs));
  job->out_gain = pow(10.0, 10.0 * (1.0 - 1.0 / 4.0) / 40.0) * pow(10.0, -threshold_db / 20.0);
  job->ceiling = 1.0;
  return AL_OK;
}
}  // namespace

int al_fx_apply(int op, const float *src, float *dst, int64_t n, const float *params, const int32_t *iparams,
                al_stream_t stream) {
  if (int rc = fx_apply_check(op, src, dst, n)) return rc;
  al::FxArgs a{op, params ? params[0] : 0.f, 0, 0, AL_FADE_NONE, AL_FADE_NONE};
  if (op == AL_FX_FADE) {
    if (!iparams) return fail(AL_E_BADARG, "fade needs iparams");
    a.n_in = iparams[0]; a.n_out = iparams[1]; a.shape_in = iparams[2]; a.shape_out = iparams[3];
  }
  if (op == AL_FX_DEEMPH) {
    al::DeemphJob job;
    if (int rc = deemph_prepare(src, dst, n, a.p0, &job)) return rc;
    hipLaunchKernelGGL(al::k_fx_deemph, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const al::DeemphJob *)nullptr, job);
    return check_launch("k_fx_deemph");
  }
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(al::k_fx_pointwise, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0,
                     (hipStream_t)stream, src, dst, n, a);
  return check_launch("k_fx_pointwise");
}

int al_fx_frame_shuffle(const float *src, float *dst, int64_t n, int32_t frame_len, int32_t row_len,
                        const int32_t *rows, int32_t n_rows, al_stream_t stream) {
  if (!src || !dst || !rows || n <= 0 || frame_len <= 0 || row_len <= 0 || n_rows <= 0 || src == dst)
    return fail(AL_E_BADARG, "bad frame_shuffle arguments");
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(al::k_frame_shuffle, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0,
                     (hipStream_t)stream, src, dst, n, frame_len, row_len, rows, n_rows);
  return check_launch("k_frame_shuffle");
}

int al_fx_sos(const float *src, float *dst, int64_t n, const double *sos, int32_t n_sections, al_stream_t stream) {
  al::SosJob job;
  if (int rc = sos_prepare(src, dst, n, sos, n_sections, &job)) return rc;
  hipLaunchKernelGGL(al::k_fx_sos, dim3(1), dim3(al::SOS_THREADS), 0, (hipStream_t)stream, (const al::SosJob *)nullptr, job);
  return check_launch("k_fx_sos");
}

int al_fx_delay(const float *src, float *dst, int64_t n, int64_t delay_samples, float feedback, float mix, al_stream_t stream) {
  static const char *const names[] = {"feedback", "mix"};
  const double vals[] = {feedback, mix};
  if (int e = fx_check("al_fx_delay", src, dst, n, names, vals, 2)) return e;
  if (delay_samples < 0) return fail(AL_E_BADARG, "al_fx_delay: delay_samples must be >= 0");
  const al::DelayPlan pl = al::delay_plan(n, delay_samples, (double)feedback);
  const int64_t grid = (pl.residues + pl.G - 1) / pl.G;
  hipLaunchKernelGGL(al::k_fx_delay, dim3((unsigned)grid), dim3(pl.G * pl.P), 0, (hipStream_t)stream, src, dst, n, pl,
                     (double)feedback, 1.0 - (double)mix, (double)mix);
  return check_launch("k_fx_delay");
}

int al_fx_chorus(const float *src, float *dst, int64_t n, double fs, double rate_hz, double depth, double centre_delay_ms,
                 double feedback, double mix, al_stream_t stream) {
  al::ChorusJob job;
  if (int rc = chorus_prepare(src, dst, n, fs, rate_hz, depth, centre_delay_ms, feedback, mix, &job)) return rc;
  if (feedback == 0.0) {
    const int64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(al::k_fx_chorus_ff, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0,
                       (hipStream_t)stream, src, dst, n, job.a);
    return check_launch("k_fx_chorus_ff");
  }
  hipLaunchKernelGGL(al::k_fx_chorus_fb, dim3(1), dim3(al::CHO_THREADS), 0, (hipStream_t)stream, (const al::ChorusJob *)nullptr, job);
  return check_launch("k_fx_chorus_fb");
}

int al_fx_phaser(const float *src, float *dst, int64_t n, double fs, double rate_hz, double depth, double centre_frequency_hz,
                 double feedback, double mix, al_stream_t stream) {
  al::PhaserJob job;
  if (int rc = phaser_prepare(src, dst, n, fs, rate_hz, depth, centre_frequency_hz, feedback, mix, &job)) return rc;
  hipLaunchKernelGGL(al::k_fx_phaser, dim3(1), dim3(al::PH_THREADS), 0, (hipStream_t)stream, (const al::PhaserJob *)nullptr, job);
  return check_launch("k_fx_phaser");
}

int al_fx_compressor(const float *src, float *dst, int64_t n, double fs, double threshold_db, double ratio, double attack_ms,
                     double release_ms, al_stream_t stream) {
  al::DynJob job;
  if (int rc = compressor_prepare(src, dst, n, fs, threshold_db, ratio, attack_ms, release_ms, &job)) return rc;
  hipLaunchKernelGGL(al::k_fx_dynamics, dim3(1), dim3(al::DYN_LANES), 0, (hipStream_t)stream, (const al::DynJob *)nullptr, job);
  return check_launch("k_fx_dynamics");
}

int al_fx_limiter(const float *src, float *dst, int64_t n, double fs, double threshold_db, double release_ms, al_stream_t stream) {
  al::DynJob job;
  if (int rc = limiter_prepare(src, dst, n, fs, threshold_db, release_ms, &job)) return rc;
  hipLaunchKernelGGL(al::k_fx_dynamics, dim3(1), dim3(al::DYN_LANES), 0, (hipStream_t)stream, (const al::DynJob *)nullptr, job);
  return check_launch("k_fx_dynamics");
}

// ---- time-stretch FX (phase vocoder, Kaiser-windowed sinc resampler): DESIGN.md "Time-stretch FX"
namespace {
// 0, or the error of the first bad pointer or length; src of n samples, dst of n_out
int stretch_check(const char *fn, const float *src, int64_t n, const float *dst, int64_t n_out, const char *n_name,
                  const char *n_out_name, const void *workspace, bool needs_workspace) {
  char msg[200];
  if (!src || !dst || (needs_workspace && !workspace)) snprintf(msg, sizeof(msg), "%s: null pointer", fn);
  else if (n < 1) snprintf(msg, sizeof(msg), "%s: %s must be >= 1", fn, n_name);
  else if (n_out < 1) snprintf(msg, sizeof(msg), "%s: %s must be >= 1", fn, n_out_name);
  else return AL_OK;
  return fail(AL_E_BADARG, msg);
}

int stretch_overlap_check(const char *fn, const float *src, int64_t n, const float *dst, int64_t n_out) {
  if (!fx_ranges_overlap(src, n, dst, n_out)) return AL_OK;
  char msg[200];
  snprintf(msg, sizeof(msg), "%s: dst overlaps src (out of place only)", fn);
  return fail(AL_E_BADARG, msg);
}

// 0, or the error of a bad (n, rate, n_fft): the geometry both time-stretch entries derive
int stretch_geometry_check(const char *fn, int64_t n, double rate, int32_t n_fft) {
  char msg[200];
  const char *why = nullptr;
  if (!al::pv_fft_ok(n_fft)) why = "n_fft must be a power of two in [64, 4096]";
  else if (!isfinite(rate) || rate < 0.25 || rate > 4.0) why = "rate must be finite and in [0.25, 4]";
  else if (al::pv_frames_in(n, n_fft) > al::PV_MAX_FRAMES) why = "too many analysis frames (F = 1 + n / hop must be <= 2^30)";
  else if (al::pv_frames_out(al::pv_frames_in(n, n_fft), rate) > al::PV_MAX_FRAMES) why = "too many output frames (T must be <= 2^30)";
  if (!why) return AL_OK;
  snprintf(msg, sizeof(msg), "%s: %s", fn, why);
  return fail(AL_E_BADARG, msg);
}
}  // namespace

int64_t al_fx_time_stretch_workspace_floats(int64_t n, double rate, int32_t n_fft) {
  if (n < 1 || stretch_geometry_check("al_fx_time_stretch_workspace_floats", n, rate, n_fft)) return 0;
  return al::pv_plan(n, rate, n_fft).floats;
}

int al_fx_time_stretch(const float *src, int64_t n, float *dst, int64_t n_out, double rate, int32_t n_fft, float *workspace,
                       al_stream_t stream) {
  if (int rc = stretch_check("al_fx_time_stretch", src, n, dst, n_out, "n", "n_out", workspace, true)) return rc;
  if (int rc = stretch_geometry_check("al_fx_time_stretch", n, rate, n_fft)) return rc;   // before the ranges: it bounds n
  if (int rc = stretch_overlap_check("al_fx_time_stretch", src, n, dst, n_out)) return rc;
  if (((uintptr_t)workspace & 15) != 0) return fail(AL_E_BADARG, "al_fx_time_stretch: workspace must be 16-byte aligned");
  al::launch_time_stretch(src, n, dst, n_out, rate, n_fft, workspace, (hipStream_t)stream);
  return check_launch("al_fx_time_stretch");  // hipGetLastError keeps the first failure of the sequence until it is read
}

int al_fx_resample_sinc(const float *src, int64_t m, float *dst, int64_t n, al_stream_t stream) {
  if (int rc = stretch_check("al_fx_resample_sinc", src, m, dst, n, "m", "n", nullptr, false)) return rc;
  if (m > 0x7fffffff || n > 0x7fffffff) return fail(AL_E_BADARG, "al_fx_resample_sinc: m and n must be below 2^31");
  if (int rc = stretch_overlap_check("al_fx_resample_sinc", src, m, dst, n)) return rc;
  al::launch_resample_sinc(src, m, dst, n, (hipStream_t)stream);
  return check_launch("k_resample_sinc");
}

// ---- batched FX launches: one workgroup per job, the jobs of one kind in one grid
namespace {
int64_t fxb_desc_bytes(int32_t kind) {
  switch (kind) {
    case AL_FXB_SOS: return (int64_t)sizeof(al::SosJob);
    case AL_FXB_CHORUS: return (int64_t)sizeof(al::ChorusJob);
    case AL_FXB_PHASER: return (int64_t)sizeof(al::PhaserJob);
    case AL_FXB_DEEMPH: return (int64_t)sizeof(al::DeemphJob);
    case AL_FXB_COMPRESSOR:
    case AL_FXB_LIMITER: return (int64_t)sizeof(al::DynJob);
    default: return -1;
  }
}

// the last error, with the job it belongs to in front
int fail_job(int rc, int32_t job) {
  char msg[sizeof(g_err)];
  snprintf(msg, sizeof(msg), "al_fx_batch_pack: job %d: %.200s", job, g_err);
  return fail(rc, msg);
}

struct FxRange {
  const float *src, *dst;
  int64_t n;
};
}  // namespace

int64_t al_fx_batch_desc_bytes(int32_t kind) { return fxb_desc_bytes(kind); }

int al_fx_batch_pack(int32_t kind, const void *jobs, int32_t count, void *host_table) {
  if (fxb_desc_bytes(kind) < 0) return fail(AL_E_BADARG, "al_fx_batch_pack: unknown kind");
  if (!jobs || !host_table) return fail(AL_E_BADARG, "al_fx_batch_pack: null pointer");
  if (count < 1) return fail(AL_E_BADARG, "al_fx_batch_pack: count must be >= 1");
  for (int32_t i = 0; i < count; ++i) {
    int rc = AL_OK;
    if (kind == AL_FXB_SOS) {
      const al_fx_sos_job &j = static_cast<const al_fx_sos_job *>(jobs)[i];
      rc = sos_prepare(j.src, j.dst, j.n, j.sos, j.n_sections, static_cast<al::SosJob *>(host_table) + i);
    } else if (kind == AL_FXB_DEEMPH) {
      const al_fx_deemph_job &j = static_cast<const al_fx_deemph_job *>(jobs)[i];
      rc = deemph_prepare(j.src, j.dst, j.n, j.coef, static_cast<al::DeemphJob *>(host_table) + i);
    } else if (kind == AL_FXB_COMPRESSOR) {
      const al_fx_compressor_job &j = static_cast<const al_fx_compressor_job *>(jobs)[i];
      rc = compressor_prepare(j.src, j.dst, j.n, j.fs, j.threshold_db, j.ratio, j.attack_ms, j.release_ms,
                              static_cast<al::DynJob *>(host_table) + i);
    } else if (kind == AL_FXB_LIMITER) {
      const al_fx_limiter_job &j = static_cast<const al_fx_limiter_job *>(jobs)[i];
      rc = limiter_prepare(j.src, j.dst, j.n, j.fs, j.threshold_db, j.release_ms, static_cast<al::DynJob *>(host_table) + i);
    } else {
      const al_fx_mod_job &j = static_cast<const al_fx_mod_job *>(jobs)[i];
      if (kind == AL_FXB_CHORUS) {
        rc = chorus_prepare(j.src, j.dst, j.n, j.fs, j.rate_hz, j.depth, j.centre, j.feedback, j.mix,
                            static_cast<al::ChorusJob *>(host_table) + i);
        if (!rc && j.feedback == 0.0)
          rc = fail(AL_E_BADARG, "al_fx_chorus: feedback == 0 runs grid-wide (k_fx_chorus_ff): not a batch job");
      } else {
        rc = phaser_prepare(j.src, j.dst, j.n, j.fs, j.rate_hz, j.depth, j.centre, j.feedback, j.mix,
                            static_cast<al::PhaserJob *>(host_table) + i);
      }
    }
    if (rc) return fail_job(rc, i);
  }
  // the workgroups run concurrently: no job may write where another reads or writes (src, dst, n lead every job struct)
  const size_t stride = kind == AL_FXB_SOS          ? sizeof(al_fx_sos_job)
                        : kind == AL_FXB_DEEMPH     ? sizeof(al_fx_deemph_job)
                        : kind == AL_FXB_COMPRESSOR ? sizeof(al_fx_compressor_job)
                        : kind == AL_FXB_LIMITER    ? sizeof(al_fx_limiter_job)
                                                    : sizeof(al_fx_mod_job);
  auto range = [&](int32_t i) { return reinterpret_cast<const FxRange *>(static_cast<const char *>(jobs) + stride * i); };
  for (int32_t i = 0; i < count; ++i)
    for (int32_t k = 0; k < count; ++k) {
      const FxRange *a = range(i), *b = range(k);
      if (k == i || !(fx_ranges_overlap(a->dst, a->n, b->src, b->n) || fx_ranges_overlap(a->dst, a->n, b->dst, b->n))) continue;
      char msg[160];
      snprintf(msg, sizeof(msg), "al_fx_batch_pack: job %d: dst overlaps src or dst of job %d (the jobs run concurrently)", i, k);
      return fail(AL_E_BADARG, msg);
    }
  return AL_OK;
}

int al_fx_batch_launch(int32_t kind, const void *device_table, int32_t count, al_stream_t stream) {
  if (fxb_desc_bytes(kind) < 0) return fail(AL_E_BADARG, "al_fx_batch_launch: unknown kind");
  if (!device_table || count < 1) return fail(AL_E_BADARG, "al_fx_batch_launch: needs a table and count >= 1");
  switch (kind) {
    case AL_FXB_SOS:
      hipLaunchKernelGGL(al::k_fx_sos, dim3((unsigned)count), dim3(al::SOS_THREADS), 0, (hipStream_t)stream, static_cast<const al::SosJob *>(device_table), al::SosJob{});
      return check_launch("k_fx_sos");
    case AL_FXB_CHORUS:
      hipLaunchKernelGGL(al::k_fx_chorus_fb, dim3((unsigned)count), dim3(al::CHO_THREADS), 0, (hipStream_t)stream, static_cast<const al::ChorusJob *>(device_table), al::ChorusJob{});
      return check_launch("k_fx_chorus_fb");
    case AL_FXB_PHASER:
      hipLaunchKernelGGL(al::k_fx_phaser, dim3((unsigned)count), dim3(al::PH_THREADS), 0, (hipStream_t)stream, static_cast<const al::PhaserJob *>(device_table), al::PhaserJob{});
      return check_launch("k_fx_phaser");
    case AL_FXB_COMPRESSOR:
    case AL_FXB_LIMITER:
      hipLaunchKernelGGL(al::k_fx_dynamics, dim3((unsigned)count), dim3(al::DYN_LANES), 0, (hipStream_t)stream, static_cast<const al::DynJob *>(device_table), al::DynJob{});
      return check_launch("k_fx_dynamics");
    default:
      hipLaunchKernelGGL(al::k_fx_deemph, dim3((unsigned)count), dim3(1024), 0, (hipStream_t)stream, static_cast<const al::DeemphJob *>(device_table), al::DeemphJob{});
      return check_launch("k_fx_deemph");
  }
}

// ---- arbitrary-length inverse real FFT (ambience)
int64_t al_noise_workspace_floats(int32_t rows, int64_t n) {
  if (rows <= 0 || n <= 0) return 0;
  const al::BigPlan p = al::big_plan(n);
  const int64_t per = p.bluestein ? p.L : p.len;
  return 2 * (2 * (int64_t)rows * per) + (p.bluestein ? 2 * 2 * p.L + 2 * (int64_t)rows * p.len : 0);
}

int al_noise_irfft(const float *zr, const float *zi, const float *shape, int32_t rows, int64_t n, float inv_sigma,
                   float *out, float *workspace, al_stream_t stream) {
  if (!zr || !zi || !shape || !out || !workspace || rows <= 0 || n <= 0) return fail(AL_E_BADARG, "bad noise arguments");
  al::noise_irfft(zr, zi, 0, shape, rows, n, inv_sigma, out, workspace, (hipStream_t)stream);
  return check_launch("al_noise_irfft");  // hipGetLastError keeps the first failure of the sequence until it is read
}

int al_noise_irfft_seeded(uint64_t seed, const float *shape, int32_t rows, int64_t n, float inv_sigma, float *out,
                          float *workspace, al_stream_t stream) {
  if (!out || !workspace || rows <= 0 || n <= 0) return fail(AL_E_BADARG, "bad noise arguments");
  al::noise_irfft(nullptr, nullptr, seed, shape, rows, n, inv_sigma, out, workspace, (hipStream_t)stream);
  return check_launch("al_noise_irfft");
}

int al_normal_fill(float *out, int64_t n, uint64_t seed, uint32_t tag, float scale, al_stream_t stream) {
  if (!out || n <= 0) return fail(AL_E_BADARG, "bad normal_fill arguments");
  if (((uintptr_t)out & 15) != 0) return fail(AL_E_BADARG, "normal_fill: output must be 16-byte aligned");
  const int64_t blocks = (n / 4 + 256) / 256;
  hipLaunchKernelGGL(al::k_normal_fill, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, (hipStream_t)stream, out, n,
                     seed, tag, scale);
  return check_launch("k_normal_fill");
}

int al_philox4x32_10(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]) {
  if (!counter || !key || !out) return fail(AL_E_BADARG, "bad philox arguments");
  const al::Philox4 p = al::philox4x32_10(counter[0], counter[1], counter[2], counter[3], key[0], key[1]);
  out[0] = p.x; out[1] = p.y; out[2] = p.z; out[3] = p.w;
  return AL_OK;
}

int al_ambience_scales(const double *row_stats, int32_t rows, int64_t cols, float ref_db, int32_t normalize, float *scales,
                       al_stream_t stream) {
  if (!row_stats || !scales || rows <= 0 || rows > 1024 || cols <= 0) return fail(AL_E_BADARG, "bad ambience_scales arguments");
  hipLaunchKernelGGL(al::k_ambience_scales, dim3(1), dim3(64), 0, (hipStream_t)stream, row_stats, rows, cols, ref_db, normalize, scales);
  return check_launch("k_ambience_scales");
}

int al_axpy_rows(float *y, const float *x, const float *a_dev, int32_t rows, int64_t cols, al_stream_t stream) {
  if (!x || !y || !a_dev || rows <= 0 || rows > 65535 || cols <= 0) return fail(AL_E_BADARG, "bad axpy_rows arguments");
  const int64_t blocks = (cols + 255) / 256;
  hipLaunchKernelGGL(al::k_axpy_rows, dim3((unsigned)(blocks < 2048 ? blocks : 2048), rows), dim3(256), 0, (hipStream_t)stream, y, x,
                     a_dev, cols);
  return check_launch("k_axpy_rows");
}

// ---- STFT-domain intermediates of the moving path (A7), reference signatures kept in audiblelight_amd/synthesize.py
int64_t al_stft_workspace_floats(int64_t series, int32_t fft_size) {
  if (series <= 0 || fft_size <= 0) return 0;
  const int64_t group = series < al::MAX_GRID_ROWS ? series : al::MAX_GRID_ROWS;
  return 2 * 2 * group * (int64_t)fft_size + al::any_fft_tmp_floats(group, fft_size);  // ping-pong complex buffers for one launch group (+ Bluestein's)
}

int al_stft(const float *y, int64_t rows, int64_t n, int32_t fft_size, int32_t win_size, int32_t hop_size, float *spec,
            float *workspace, al_stream_t stream) {
  // fft_size < win_size is legal in the reference: rfft(frames, n=fft_size) crops every windowed frame to its first fft_size samples
  if (!y || !spec || !workspace || rows <= 0 || n <= 0 || win_size <= 0 || hop_size <= 0 || win_size < hop_size || fft_size <= 0)
    return fail(AL_E_BADARG, "bad stft arguments");
  hipStream_t st = (hipStream_t)stream;
  const int n_frames = 2 * (int)((n + 2 * (int64_t)hop_size - 1) / (2 * (int64_t)hop_size)) + 1;
  const int64_t series = rows * n_frames;
  const int64_t group = series < al::MAX_GRID_ROWS ? series : al::MAX_GRID_ROWS;
  float2 *a = reinterpret_cast<float2 *>(workspace);
  float2 *b = a + group * fft_size;
  float *tmp = reinterpret_cast<float *>(b + group * fft_size);
  for (int64_t s0 = 0; s0 < series; s0 += al::MAX_GRID_ROWS) {
    const int g = (int)(series - s0 < al::MAX_GRID_ROWS ? series - s0 : al::MAX_GRID_ROWS);
    const dim3 grid((unsigned)((fft_size + 255) / 256), g);
    hipLaunchKernelGGL(al::k_stft_pack, grid, dim3(256), 0, st, y, n, n_frames, fft_size, win_size, hop_size, s0, a);
    const float2 *z = al::any_fft(a, b, tmp, g, fft_size, -1, st);
    hipLaunchKernelGGL(al::k_stft_take_half, grid, dim3(256), 0, st, z, fft_size, s0, reinterpret_cast<float2 *>(spec));
  }
  return check_launch("al_stft");
}

int al_tv_stft_mac(const float *s_audio, const float *s_ir, const float *w_ir, int32_t n_frames, int32_t n_frames_ir,
                   int32_t n_freq, int32_t n_ch, int32_t n_irs, float *out, al_stream_t stream) {
  if (!s_audio || !s_ir || !w_ir || !out || n_frames <= 0 || n_frames_ir <= 0 || n_freq <= 0 || n_ch <= 0 || n_irs <= 0)
    return fail(AL_E_BADARG, "bad tv_stft_mac arguments");
  // one launch per al::MAX_GRID_ROWS output frames (grid.y limit): a clip of any length (hop 16 at 44.1 kHz passes 65 535 frames after 23 s)
  for (int32_t f0 = 0; f0 < n_frames; f0 += al::MAX_GRID_ROWS) {
    const int g = n_frames - f0 < al::MAX_GRID_ROWS ? n_frames - f0 : al::MAX_GRID_ROWS;
    const dim3 grid((unsigned)(((int64_t)n_freq * n_ch + 255) / 256), g);
    hipLaunchKernelGGL(al::k_tv_stft_mac, grid, dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float2 *>(s_audio),
                       reinterpret_cast<const float2 *>(s_ir), w_ir, f0, n_frames_ir, n_freq, n_ch, n_irs,
                       reinterpret_cast<float2 *>(out));
  }
  return check_launch("k_tv_stft_mac");
}

int64_t al_istft_workspace_floats(int32_t n_frames, int32_t n_ch, int32_t fft_size) {
  if (n_frames <= 0 || n_ch <= 0 || fft_size <= 0) return 0;
  const int64_t series = (int64_t)n_frames * n_ch;
  return 2 * 2 * series * fft_size + al::any_fft_tmp_floats(series < al::MAX_GRID_ROWS ? series : al::MAX_GRID_ROWS, fft_size);
}

int al_istft_ola(const float *spatial_stft, int32_t n_frames, int32_t n_freq, int32_t n_ch, int32_t fft_size,
                 int32_t win_size, int32_t hop_size, float *out, float *workspace, al_stream_t stream) {
  if (!spatial_stft || !out || !workspace || n_frames <= 0 || n_ch <= 0 || fft_size <= 0 || win_size <= 0 || hop_size <= 0)
    return fail(AL_E_BADARG, "bad istft arguments");
  if (n_freq != fft_size / 2 + 1) return fail(AL_E_BADARG, "istft: n_freq must be fft_size / 2 + 1");
  if ((int64_t)n_frames * hop_size <= win_size) return fail(AL_E_BADARG, "istft: no output samples");
  hipStream_t st = (hipStream_t)stream;
  const int64_t series = (int64_t)n_frames * n_ch;
  float2 *a = reinterpret_cast<float2 *>(workspace), *b = a + series * fft_size;
  float *tmp = reinterpret_cast<float *>(b + series * fft_size);
  const float2 *frames = nullptr;
  for (int64_t s0 = 0; s0 < series; s0 += al::MAX_GRID_ROWS) {
    const int g = (int)(series - s0 < al::MAX_GRID_ROWS ? series - s0 : al::MAX_GRID_ROWS);
    const dim3 grid((unsigned)((fft_size + 255) / 256), g);
    hipLaunchKernelGGL(al::k_istft_pack, grid, dim3(256), 0, st, reinterpret_cast<const float2 *>(spatial_stft), n_freq, n_ch,
                       fft_size, s0, a + s0 * fft_size);
    const float2 *z = al::any_fft(a + s0 * fft_size, b + s0 * fft_size, tmp, g, fft_size, +1, st);
    frames = (z == a + s0 * fft_size) ? a : b;  // every group ends in the same buffer (same pass count; Bluestein: always the second)
  }
  const int64_t total = ((int64_t)n_frames * hop_size - win_size) * n_ch;
  hipLaunchKernelGGL(al::k_istft_ola, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, frames, n_frames, n_ch, fft_size,
                     win_size, hop_size, out);
  return check_launch("al_istft_ola");
}

int al_scale_matrix_rows(float *x, int32_t rows, int64_t cols, const float *scale, al_stream_t stream) {
  if (!x || !scale || rows <= 0 || rows > 65535 || cols <= 0) return fail(AL_E_BADARG, "bad scale_matrix_rows arguments");
  const int64_t blocks = (cols + 255) / 256;
  hipLaunchKernelGGL(al::k_scale_matrix_rows, dim3((unsigned)(blocks < 2048 ? blocks : 2048), rows), dim3(256), 0,
                     (hipStream_t)stream, x, cols, scale);
  return check_launch("k_scale_matrix_rows");
}

int al_pack_irs_f64(const double *src, float *dst, int64_t rows, int32_t len, int32_t dst_pitch, al_stream_t stream) {
  if (!src || !dst || rows <= 0 || len <= 0 || dst_pitch < len || (dst_pitch & 3) || rows > 0x7fffffff)
    return fail(AL_E_BADARG, "bad pack_irs arguments");
  hipLaunchKernelGGL(al::k_pack_irs<double>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, src, dst, len, dst_pitch);
  return check_launch("k_pack_irs<double>");
}

int al_pack_irs_f32(const float *src, float *dst, int64_t rows, int32_t len, int32_t dst_pitch, al_stream_t stream) {
  if (!src || !dst || src == dst || rows <= 0 || len <= 0 || dst_pitch < len || (dst_pitch & 3) || rows > 0x7fffffff)
    return fail(AL_E_BADARG, "bad pack_irs arguments");
  hipLaunchKernelGGL(al::k_pack_irs<float>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, src, dst, len, dst_pitch);
  return check_launch("k_pack_irs<float>");
}

int al_pack_ragged_irs(const void *src, int32_t src_is_f64, const int64_t *offsets, const int32_t *lens, int64_t rows,
                       int32_t dst_pitch, float *dst, al_stream_t stream) {
  if (!src || !offsets || !lens || !dst || rows <= 0 || rows > 0x7fffffff || dst_pitch <= 0 || (dst_pitch & 3))
    return fail(AL_E_BADARG, "bad pack_ragged_irs arguments");
  if (src_is_f64)
    hipLaunchKernelGGL(al::k_pack_ragged<double>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const double *>(src), offsets, lens, dst, dst_pitch);
  else
    hipLaunchKernelGGL(al::k_pack_ragged<float>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const float *>(src), offsets, lens, dst, dst_pitch);
  return check_launch("k_pack_ragged");
}

// ---- shoebox room IRs (image-source method): DESIGN.md "Shoebox IRs"
int al_ism_shoebox(const double *sources, int32_t n_sources, const double *capsules, int32_t n_capsules, const double *L,
                   const double *beta, double c, double fs, int32_t max_order, int32_t ir_len, int32_t pitch, float *out,
                   al_stream_t stream) {
  if (!sources || !capsules || !L || !beta || !out) return fail(AL_E_BADARG, "al_ism_shoebox: null pointer");
  if (n_sources < 1 || n_capsules < 1) return fail(AL_E_BADARG, "al_ism_shoebox: n_sources and n_capsules must be >= 1");
  if (ir_len < 1) return fail(AL_E_BADARG, "al_ism_shoebox: ir_len must be >= 1");
  if (pitch < ir_len || (pitch & 3)) return fail(AL_E_BADARG, "al_ism_shoebox: pitch must be >= ir_len and a multiple of 4");
  if (max_order < -1) return fail(AL_E_BADARG, "al_ism_shoebox: max_order must be >= 0, or -1 for none");
  if (!isfinite(c) || !(c > 0.0) || !isfinite(fs) || !(fs > 0.0)) return fail(AL_E_BADARG, "al_ism_shoebox: c and fs must be finite and positive");
  al::IsmJob job;
  for (int i = 0; i < 3; ++i) {
    if (!isfinite(L[i]) || !(L[i] > 0.0)) return fail(AL_E_BADARG, "al_ism_shoebox: room dimensions must be finite and positive");
    if (!(c * ((double)ir_len + 42.0) / fs / L[i] + 2.0 <= al::ISM_MAX_HALF_WIDTH))
      return fail(AL_E_BADARG, "al_ism_shoebox: c (ir_len + 42) / fs spans more than 2^20 mirror cells of the room");
    job.L[i] = L[i];
  }
  for (int i = 0; i < 6; ++i) {
    if (!(beta[i] >= 0.0 && beta[i] <= 1.0)) return fail(AL_E_BADARG, "al_ism_shoebox: reflection coefficients must be in [0, 1]");
    job.beta_zero[i] = beta[i] == 0.0;
    job.ln_beta[i] = beta[i] == 0.0 ? 0.0 : log(beta[i]);
  }
  job.n_tiles = (pitch + al::ISM_TILE - 1) / al::ISM_TILE;
  if ((int64_t)job.n_tiles * n_sources * n_capsules > 0x7fffffff)
    return fail(AL_E_BADARG, "al_ism_shoebox: more than 2^31 - 1 workgroups (tiles of 256 samples x pairs): split the call");
  job.sources = sources;
  job.capsules = capsules;
  job.out = out;
  job.n_sources = n_sources;
  job.n_capsules = n_capsules;
  job.ir_len = ir_len;
  job.pitch = pitch;
  job.max_order = max_order;
  job.c = c;
  job.fs = fs;
  al::launch_ism_shoebox(job, (hipStream_t)stream);
  return check_launch("k_ism_shoebox");
}

int al_resample_poly(const float *x, int32_t rows, int64_t n_in, const float *taps, int32_t half_len, int32_t up, int32_t down,
                     float *out, int64_t n_out, int64_t out_pitch, al_stream_t stream) {
  if (!x || !taps || !out || rows <= 0 || rows > 65535 || n_in <= 0 || half_len < 0 || up <= 0 || down <= 0 || n_out <= 0 ||
      out_pitch < n_out)
    return fail(AL_E_BADARG, "bad resample_poly arguments");
  const int64_t blocks = (out_pitch + 255) / 256;
  hipLaunchKernelGGL(al::k_resample_poly, dim3((unsigned)(blocks < 4096 ? blocks : 4096), rows), dim3(256), 0, (hipStream_t)stream,
                     x, n_in, taps, half_len, up, down, out, n_out, out_pitch);
  return check_launch("k_resample_poly");
}

int al_encode_frames(const float *scene, int32_t n_capsules, int64_t n_samples, int32_t format, void *out, al_stream_t stream) {
  if (!scene || !out || n_capsules <= 0 || n_samples <= 0 || (format != AL_FRAMES_F32 && format != AL_FRAMES_PCM16))
    return fail(AL_E_BADARG, "bad encode_frames arguments");
  const bool vector_stores = format == AL_FRAMES_PCM16 ? (n_capsules & 7) == 0 : (n_capsules & 3) == 0;
  if (vector_stores && ((uintptr_t)out & 15) != 0) return fail(AL_E_BADARG, "encode_frames: output must be 16-byte aligned");
  const dim3 grid((unsigned)((n_samples + 63) / 64), (unsigned)((n_capsules + 31) / 32));
  if (format == AL_FRAMES_PCM16)
    hipLaunchKernelGGL((al::k_encode_frames<true>), grid, dim3(256), 0, (hipStream_t)stream, scene, n_capsules, n_samples, out);
  else
    hipLaunchKernelGGL((al::k_encode_frames<false>), grid, dim3(256), 0, (hipStream_t)stream, scene, n_capsules, n_samples, out);
  return check_launch("k_encode_frames");
}

int al_wrap_copy(const float *src, int64_t m, float *dst, int64_t n, al_stream_t stream) {
  if (!src || !dst || m <= 0 || n <= 0 || src == dst) return fail(AL_E_BADARG, "bad wrap_copy arguments");
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(al::k_wrap_copy, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0,
                     (hipStream_t)stream, src, m, dst, n);
  return check_launch("k_wrap_copy");
}

}  // extern "C"
