// C ABI of the MI355X synthesis path (gfx950 only): every extern "C" entry point of include/audiblelight_hip.h that launches
// device code.  No kernel, no launch planning and no definition of an effect lives here.  Each per-domain header included below
// owns its kernels, their device helpers and its host side: the choice of instantiation and grid (al_mac.h plan_mac, al_delayfx.h
// delay_plan, al_stretchfx.h pv_plan) and, for the FX, time-stretch and image-source entries, the checks and derivations that turn
// the caller's arguments into the kernel's job (the *_prepare and *_check functions of al_clipfx.h, al_sos.h, al_delayfx.h,
// al_dynfx.h, al_stretchfx.h, al_ism.h), refusing through al_status.h.  What is left to an entry is: prepare, launch, check_launch;
// the entries without a prepare check their few arguments in place.  The FX that a batched launch can run are ONE TABLE (FX_KINDS
// below): a row per batched kind, read by al_fx_batch_desc_bytes / _pack / _launch and by the single-clip entries alike.
// The FFT kernels of the pipeline are the other translation unit, al_transforms.hip.  See DESIGN.md for the data layout and
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
#include "al_irmetrics.h"
#include "al_ism.h"
#include "al_ism_bands.h"
#include "al_ism_sphere.h"
#include "al_levels.h"
#include "al_mac.h"
#include "al_mixdown.h"
#include "al_rows.h"
#include "al_sos.h"
#include "al_status.h"
#include "al_stft.h"
#include "al_stretchfx.h"

// ====================================================================== C ABI
namespace {
using al::check_error;
using al::check_launch;
using al::fail;
using al::grid_1d;

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

// ---- the FX a batched launch can run: one row per kind.  Job: the public job struct of audiblelight_hip.h; Desc: what
// Prepare derives from it, the packed descriptor that Kernel reads -- workgroup b from table[b], or `one` by value when the table
// is null (a single clip, grid of 1).  A new scan FX is one header with kernel, descriptor and prepare, one public job struct, and
// one row here.
struct FxKind {
  int32_t kind;
  size_t job_bytes, desc_bytes;
  int (*prepare)(const void *job, void *desc);   // 0, or the error of the job's first bad argument
  void (*launch)(const void *table, const void *one, unsigned count, hipStream_t stream);
  const char *kernel;                            // its name, for check_launch
  const float *(*src)(const void *job);
  const float *(*dst)(const void *job);
  int64_t (*n)(const void *job);
};

template <int32_t Kind, class JobT, class DescT, int (*Prepare)(const JobT &, DescT *), void (*Kernel)(const DescT *, DescT), int Threads>
struct FxRow {
  using Job = JobT;
  using Desc = DescT;
  static constexpr int32_t KIND = Kind;
  static int prepare(const void *job, void *desc) { return Prepare(*static_cast<const Job *>(job), static_cast<Desc *>(desc)); }
  static void launch(const void *table, const void *one, unsigned count, hipStream_t stream) {
    hipLaunchKernelGGL(Kernel, dim3(count), dim3(Threads), 0, stream, static_cast<const Desc *>(table),
                       one ? *static_cast<const Desc *>(one) : Desc{});
  }
  // by name: a job struct without src, dst and n does not compile
  static const float *src(const void *job) { return static_cast<const Job *>(job)->src; }
  static const float *dst(const void *job) { return static_cast<const Job *>(job)->dst; }
  static int64_t n(const void *job) { return static_cast<const Job *>(job)->n; }
  static constexpr FxKind row(const char *kernel) { return {Kind, sizeof(Job), sizeof(Desc), prepare, launch, kernel, src, dst, n}; }
};

using SosRow = FxRow<AL_FXB_SOS, al_fx_sos_job, al::SosJob, al::sos_prepare, al::k_fx_sos, al::SOS_THREADS>;
using ChorusRow = FxRow<AL_FXB_CHORUS, al_fx_mod_job, al::ChorusJob, al::chorus_prepare, al::k_fx_chorus_fb, al::CHO_THREADS>;
using PhaserRow = FxRow<AL_FXB_PHASER, al_fx_mod_job, al::PhaserJob, al::phaser_prepare, al::k_fx_phaser, al::PH_THREADS>;
using DeemphRow = FxRow<AL_FXB_DEEMPH, al_fx_deemph_job, al::DeemphJob, al::deemph_prepare, al::k_fx_deemph, 1024>;
using CompressorRow = FxRow<AL_FXB_COMPRESSOR, al_fx_compressor_job, al::DynJob, al::compressor_prepare, al::k_fx_dynamics, al::DYN_LANES>;
using LimiterRow = FxRow<AL_FXB_LIMITER, al_fx_limiter_job, al::DynJob, al::limiter_prepare, al::k_fx_dynamics, al::DYN_LANES>;

const FxKind FX_KINDS[] = {SosRow::row("k_fx_sos"),       ChorusRow::row("k_fx_chorus_fb"),    PhaserRow::row("k_fx_phaser"),
                           DeemphRow::row("k_fx_deemph"), CompressorRow::row("k_fx_dynamics"), LimiterRow::row("k_fx_dynamics")};

const FxKind *fx_kind(int32_t kind) {
  for (const FxKind &row : FX_KINDS)
    if (row.kind == kind) return &row;
  return nullptr;
}

// one clip through its row, exactly as a batch of one job: the same prepare, the same kernel, the descriptor by value
template <class Row>
int fx_single(const typename Row::Job &in, al_stream_t stream) {
  const FxKind *row = fx_kind(Row::KIND);
  if (!row) return fail(AL_E_UNSUPPORTED, "fx_single: this kind has no row in FX_KINDS");
  typename Row::Desc desc;
  if (int rc = row->prepare(&in, &desc)) return rc;
  row->launch(nullptr, &desc, 1, (hipStream_t)stream);
  return check_launch(row->kernel);
}

}  // namespace

extern "C" {

const char *al_last_error(void) { return al::g_err; }
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
  hipLaunchKernelGGL(al::k_scale, dim3(grid_1d(n, 8192)), dim3(256), 0, (hipStream_t)stream, x, n, scale);
  return check_launch("k_scale");
}

int al_scale_rows_f64(float *x, int64_t n, const double *scale, al_stream_t stream) {
  if (!x || !scale || n < 0) return fail(AL_E_BADARG, "bad scale arguments");
  if (n == 0) return AL_OK;
  hipLaunchKernelGGL(al::k_scale_d, dim3(grid_1d(n, 8192)), dim3(256), 0, (hipStream_t)stream, x, n, scale);
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
  hipLaunchKernelGGL(al::k_axpy, dim3(grid_1d(n, 8192)), dim3(256), 0, (hipStream_t)stream, y, x, a_dev, n);
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

// ---- FX.  The scans and walks run through their row of FX_KINDS; the pointwise ops, the frame shuffle, the delay and the
// feed-forward chorus are grid-wide launches of their own.
int al_fx_apply(int op, const float *src, float *dst, int64_t n, const float *params, const int32_t *iparams,
                al_stream_t stream) {
  if (int rc = al::fx_apply_check(op, src, dst, n)) return rc;
  al::FxArgs a{op, params ? params[0] : 0.f, 0, 0, AL_FADE_NONE, AL_FADE_NONE};
  if (op == AL_FX_FADE) {
    if (!iparams) return fail(AL_E_BADARG, "fade needs iparams");
    a.n_in = iparams[0]; a.n_out = iparams[1]; a.shape_in = iparams[2]; a.shape_out = iparams[3];
  }
  if (op == AL_FX_DEEMPH) return fx_single<DeemphRow>(al_fx_deemph_job{src, dst, n, a.p0, 0}, stream);
  hipLaunchKernelGGL(al::k_fx_pointwise, dim3(grid_1d(n, 4096)), dim3(256), 0,
                     (hipStream_t)stream, src, dst, n, a);
  return check_launch("k_fx_pointwise");
}

int al_fx_frame_shuffle(const float *src, float *dst, int64_t n, int32_t frame_len, int32_t row_len,
                        const int32_t *rows, int32_t n_rows, al_stream_t stream) {
  if (!src || !dst || !rows || n <= 0 || frame_len <= 0 || row_len <= 0 || n_rows <= 0 || src == dst)
    return fail(AL_E_BADARG, "bad frame_shuffle arguments");
  hipLaunchKernelGGL(al::k_frame_shuffle, dim3(grid_1d(n, 4096)), dim3(256), 0,
                     (hipStream_t)stream, src, dst, n, frame_len, row_len, rows, n_rows);
  return check_launch("k_frame_shuffle");
}

int al_fx_sos(const float *src, float *dst, int64_t n, const double *sos, int32_t n_sections, al_stream_t stream) {
  return fx_single<SosRow>(al_fx_sos_job{src, dst, n, sos, n_sections, 0}, stream);
}

int al_fx_delay(const float *src, float *dst, int64_t n, int64_t delay_samples, float feedback, float mix, al_stream_t stream) {
  if (int rc = al::delay_check(src, dst, n, delay_samples, feedback, mix)) return rc;
  const al::DelayPlan pl = al::delay_plan(n, delay_samples, (double)feedback);
  const int64_t grid = (pl.residues + pl.G - 1) / pl.G;
  hipLaunchKernelGGL(al::k_fx_delay, dim3((unsigned)grid), dim3(pl.G * pl.P), 0, (hipStream_t)stream, src, dst, n, pl,
                     (double)feedback, 1.0 - (double)mix, (double)mix);
  return check_launch("k_fx_delay");
}

int al_fx_chorus(const float *src, float *dst, int64_t n, double fs, double rate_hz, double depth, double centre_delay_ms,
                 double feedback, double mix, al_stream_t stream) {
  const al_fx_mod_job in{src, dst, n, fs, rate_hz, depth, centre_delay_ms, feedback, mix};
  if (feedback != 0.0) return fx_single<ChorusRow>(in, stream);
  al::ChorusJob job;   // no feedback: the same prepare, then the gather runs grid-wide
  if (int rc = al::chorus_prepare(in, &job)) return rc;
  hipLaunchKernelGGL(al::k_fx_chorus_ff, dim3(grid_1d(n, 8192)), dim3(256), 0, (hipStream_t)stream, src, dst, n, job.a);
  return check_launch("k_fx_chorus_ff");
}

int al_fx_phaser(const float *src, float *dst, int64_t n, double fs, double rate_hz, double depth, double centre_frequency_hz,
                 double feedback, double mix, al_stream_t stream) {
  return fx_single<PhaserRow>(al_fx_mod_job{src, dst, n, fs, rate_hz, depth, centre_frequency_hz, feedback, mix}, stream);
}

int al_fx_compressor(const float *src, float *dst, int64_t n, double fs, double threshold_db, double ratio, double attack_ms,
                     double release_ms, al_stream_t stream) {
  return fx_single<CompressorRow>(al_fx_compressor_job{src, dst, n, fs, threshold_db, ratio, attack_ms, release_ms}, stream);
}

int al_fx_limiter(const float *src, float *dst, int64_t n, double fs, double threshold_db, double release_ms, al_stream_t stream) {
  return fx_single<LimiterRow>(al_fx_limiter_job{src, dst, n, fs, threshold_db, release_ms}, stream);
}

// ---- time-stretch FX (phase vocoder, Kaiser-windowed sinc resampler): DESIGN.md "Time-stretch FX"
int64_t al_fx_time_stretch_workspace_floats(int64_t n, double rate, int32_t n_fft) {
  if (n < 1 || al::stretch_geometry_check("al_fx_time_stretch_workspace_floats", n, rate, n_fft)) return 0;
  return al::pv_plan(n, rate, n_fft).floats;
}

int al_fx_time_stretch(const float *src, int64_t n, float *dst, int64_t n_out, double rate, int32_t n_fft, float *workspace,
                       al_stream_t stream) {
  if (int rc = al::stretch_check("al_fx_time_stretch", src, n, dst, n_out, "n", "n_out", workspace, true)) return rc;
  if (int rc = al::stretch_geometry_check("al_fx_time_stretch", n, rate, n_fft)) return rc;   // before the ranges: it bounds n
  if (int rc = al::stretch_overlap_check("al_fx_time_stretch", src, n, dst, n_out)) return rc;
  if (((uintptr_t)workspace & 15) != 0) return fail(AL_E_BADARG, "al_fx_time_stretch: workspace must be 16-byte aligned");
  al::launch_time_stretch(src, n, dst, n_out, rate, n_fft, workspace, (hipStream_t)stream);
  return check_launch("al_fx_time_stretch");  // hipGetLastError keeps the first failure of the sequence until it is read
}

int al_fx_resample_sinc(const float *src, int64_t m, float *dst, int64_t n, al_stream_t stream) {
  if (int rc = al::stretch_check("al_fx_resample_sinc", src, m, dst, n, "m", "n", nullptr, false)) return rc;
  if (m > 0x7fffffff || n > 0x7fffffff) return fail(AL_E_BADARG, "al_fx_resample_sinc: m and n must be below 2^31");
  if (int rc = al::stretch_overlap_check("al_fx_resample_sinc", src, m, dst, n)) return rc;
  al::launch_resample_sinc(src, m, dst, n, (hipStream_t)stream);
  return check_launch("k_resample_sinc");
}

// ---- batched FX launches: one workgroup per job, the jobs of one kind in one grid
int64_t al_fx_batch_desc_bytes(int32_t kind) {
  const FxKind *row = fx_kind(kind);
  return row ? (int64_t)row->desc_bytes : -1;
}

int al_fx_batch_pack(int32_t kind, const void *jobs, int32_t count, void *host_table) {
  const FxKind *row = fx_kind(kind);
  if (!row) return fail(AL_E_BADARG, "al_fx_batch_pack: unknown kind");
  if (!jobs || !host_table) return fail(AL_E_BADARG, "al_fx_batch_pack: null pointer");
  if (count < 1) return fail(AL_E_BADARG, "al_fx_batch_pack: count must be >= 1");
  auto job = [&](int32_t i) -> const void * { return static_cast<const char *>(jobs) + row->job_bytes * i; };
  for (int32_t i = 0; i < count; ++i) {
    int rc = row->prepare(job(i), static_cast<char *>(host_table) + row->desc_bytes * i);
    if (!rc && row->kind == ChorusRow::KIND && static_cast<const al_fx_mod_job *>(job(i))->feedback == 0.0)
      rc = fail(AL_E_BADARG, "al_fx_chorus: feedback == 0 runs grid-wide (k_fx_chorus_ff): not a batch job");
    if (rc) {   // the refusal, with the job it belongs to in front
      char msg[sizeof(al::g_err)];
      snprintf(msg, sizeof(msg), "al_fx_batch_pack: job %d: %.200s", i, al::g_err);
      return fail(rc, msg);
    }
  }
  // the workgroups run concurrently: no job may write where another reads or writes
  for (int32_t i = 0; i < count; ++i)
    for (int32_t k = 0; k < count; ++k) {
      const void *a = job(i), *b = job(k);
      if (k == i || !(al::fx_ranges_overlap(row->dst(a), row->n(a), row->src(b), row->n(b)) ||
                      al::fx_ranges_overlap(row->dst(a), row->n(a), row->dst(b), row->n(b)))) continue;
      char msg[160];
      snprintf(msg, sizeof(msg), "al_fx_batch_pack: job %d: dst overlaps src or dst of job %d (the jobs run concurrently)", i, k);
      return fail(AL_E_BADARG, msg);
    }
  return AL_OK;
}

int al_fx_batch_launch(int32_t kind, const void *device_table, int32_t count, al_stream_t stream) {
  const FxKind *row = fx_kind(kind);
  if (!row) return fail(AL_E_BADARG, "al_fx_batch_launch: unknown kind");
  if (!device_table || count < 1) return fail(AL_E_BADARG, "al_fx_batch_launch: needs a table and count >= 1");
  row->launch(device_table, nullptr, (unsigned)count, (hipStream_t)stream);
  return check_launch(row->kernel);
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
  hipLaunchKernelGGL(al::k_axpy_rows, dim3(grid_1d(cols, 2048), rows), dim3(256), 0, (hipStream_t)stream, y, x,
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
  hipLaunchKernelGGL(al::k_scale_matrix_rows, dim3(grid_1d(cols, 2048), rows), dim3(256), 0,
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

// ---- shoebox room IRs (image-source method): DESIGN.md "Shoebox IRs".  The five point-receiver entries share one prepare and one
// launch (al_ism.h); each hands over what it has (no patterns: one channel; no source side: null and 0; no tail: mix = -1; else the
// knot tables' strides from row to row and from source to source) and states what it requires
int al_ism_shoebox(const double *sources, int32_t n_sources, const double *capsules, int32_t n_capsules, const double *L,
                   const double *beta, double c, double fs, int32_t max_order, int32_t ir_len, int32_t pitch, float *out,
                   al_stream_t stream) {
  al::IsmDirJob job;
  if (int rc = al::ism_images_prepare(sources, n_sources, nullptr, capsules, n_capsules, nullptr, 1, L, beta, 0.0, c, fs, max_order, ir_len,
                                      pitch, -1, 0, 0, 0, 0, nullptr, 0, 0, 0, out, &job))
    return rc;
  al::launch_ism_images(job, false, false, (hipStream_t)stream);
  return check_launch("k_ism_shoebox");
}

int al_ism_shoebox_tail(const double *sources, int32_t n_sources, const double *capsules, int32_t n_capsules, const double *L,
                        const double *beta, double c, double fs, int32_t max_order, int32_t ir_len, int32_t pitch, int64_t mix,
                        int64_t fade, uint64_t seed, int64_t source_id0, int64_t capsule_id0, const double *ln_env, int32_t n_knots,
                        float *out, al_stream_t stream) {
  al::IsmDirJob job;
  if (mix < 0) return al::fail(AL_E_BADARG, "al_ism_shoebox_tail: mix must be >= 0");
  if (int rc = al::ism_images_prepare(sources, n_sources, nullptr, capsules, n_capsules, nullptr, 1, L, beta, 0.0, c, fs, max_order, ir_len,
                                      pitch, mix, fade, seed, source_id0, capsule_id0, ln_env, n_knots, 0, 0, out, &job))
    return rc;
  al::launch_ism_images(job, true, false, (hipStream_t)stream);
  return check_launch("k_ism_tail");
}

// ---- the same with first-order directional receivers: DESIGN.md "Shoebox IRs: directional receivers"
int al_ism_shoebox_dir(const double *sources, int32_t n_sources, const double *receivers, int32_t n_receivers, const double *patterns,
                       int32_t n_channels, const double *L, const double *beta, double c, double fs, int32_t max_order, int32_t ir_len,
                       int32_t pitch, float *out, al_stream_t stream) {
  al::IsmDirJob job;
  if (!patterns) return al::fail(AL_E_BADARG, "al_ism_shoebox_dir: null pattern table");
  if (int rc = al::ism_images_prepare(sources, n_sources, nullptr, receivers, n_receivers, patterns, n_channels, L, beta, 0.0, c, fs,
                                      max_order, ir_len, pitch, -1, 0, 0, 0, 0, nullptr, 0, 0, 0, out, &job))
    return rc;
  al::launch_ism_images(job, false, false, (hipStream_t)stream);
  return check_launch("k_ism_shoebox_dir");
}

int al_ism_shoebox_dir_tail(const double *sources, int32_t n_sources, const double *receivers, int32_t n_receivers,
                            const double *patterns, int32_t n_channels, const double *L, const double *beta, double c, double fs,
                            int32_t max_order, int32_t ir_len, int32_t pitch, int64_t mix, int64_t fade, uint64_t seed,
                            int64_t source_id0, int64_t capsule_id0, const double *ln_env, int32_t n_knots, float *out,
                            al_stream_t stream) {
  al::IsmDirJob job;
  if (mix < 0) return al::fail(AL_E_BADARG, "al_ism_shoebox_tail: mix must be >= 0");
  if (!patterns) return al::fail(AL_E_BADARG, "al_ism_shoebox_dir: null pattern table");
  if (int rc = al::ism_images_prepare(sources, n_sources, nullptr, receivers, n_receivers, patterns, n_channels, L, beta, 0.0, c, fs,
                                      max_order, ir_len, pitch, mix, fade, seed, source_id0, capsule_id0, ln_env, n_knots, n_knots, 0, out,
                                      &job))
    return rc;
  al::launch_ism_images(job, true, false, (hipStream_t)stream);
  return check_launch("k_ism_tail");
}

// ---- the same with frequency-dependent walls in bands: DESIGN.md "Shoebox IRs: frequency-dependent walls"
int64_t al_ism_shoebox_bands_workspace_bytes(int32_t n_bands, int32_t half, int32_t ir_len, int64_t mix, int64_t fade) {
  return al::ism_rows_workspace_bytes("al_ism_shoebox_bands", "n_bands", n_bands, al::ISM_MAX_BANDS, half, al::ISM_BAND_MAX_HALF, ir_len, mix,
                                      fade);
}

int al_ism_shoebox_bands(const double *sources, int32_t n_sources, const double *capsules, int32_t n_capsules, const double *L,
                         const double *beta, int32_t n_bands, const double *filters, int32_t half, double c, double fs,
                         int32_t max_order, int32_t ir_len, int32_t pitch, void *workspace, int64_t workspace_bytes, float *out,
                         al_stream_t stream) {
  al::IsmBandJob job;
  if (int rc = al::ism_bands_prepare(sources, n_sources, capsules, n_capsules, L, beta, n_bands, filters, half, c, fs, max_order, ir_len,
                                     pitch, -1, 0, 0, 0, 0, nullptr, 0, workspace, workspace_bytes, out, &job))
    return rc;
  al::launch_ism_shoebox_bands(job, false, false, (hipStream_t)stream);
  return check_launch("k_ism_band_combine");
}

int al_ism_shoebox_bands_tail(const double *sources, int32_t n_sources, const double *capsules, int32_t n_capsules, const double *L,
                              const double *beta, int32_t n_bands, const double *filters, int32_t half, double c, double fs,
                              int32_t max_order, int32_t ir_len, int32_t pitch, int64_t mix, int64_t fade, uint64_t seed,
                              int64_t source_id0, int64_t capsule_id0, const double *ln_env, int32_t n_knots, void *workspace,
                              int64_t workspace_bytes, float *out, al_stream_t stream) {
  al::IsmBandJob job;
  if (mix < 0) return al::fail(AL_E_BADARG, "al_ism_shoebox_tail: mix must be >= 0");
  if (int rc = al::ism_bands_prepare(sources, n_sources, capsules, n_capsules, L, beta, n_bands, filters, half, c, fs, max_order, ir_len,
                                     pitch, mix, fade, seed, source_id0, capsule_id0, ln_env, n_knots, workspace, workspace_bytes, out, &job))
    return rc;
  al::launch_ism_shoebox_bands(job, true, false, (hipStream_t)stream);
  return check_launch("k_ism_band_tail");
}

// ---- the same with directional sources and air absorption: DESIGN.md "Shoebox IRs: directional sources and air"
int al_ism_shoebox_src(const double *sources, int32_t n_sources, const double *source_patterns, const double *receivers,
                       int32_t n_receivers, const double *patterns, int32_t n_channels, const double *L, const double *beta, double air,
                       double c, double fs, int32_t max_order, int32_t ir_len, int32_t pitch, int64_t mix, int64_t fade, uint64_t seed,
                       int64_t source_id0, int64_t capsule_id0, const double *ln_env, int32_t n_knots, float *out, al_stream_t stream) {
  al::IsmDirJob job;   // ln_env: (rows, N, n_knots)
  if (int rc = al::ism_images_prepare(sources, n_sources, source_patterns, receivers, n_receivers, patterns, n_channels, L, beta, air, c, fs,
                                      max_order, ir_len, pitch, mix, fade, seed, source_id0, capsule_id0, ln_env, n_knots,
                                      (int64_t)n_knots * n_sources, n_knots, out, &job))
    return rc;
  al::launch_ism_images(job, mix >= 0, true, (hipStream_t)stream);
  return check_launch("k_ism_shoebox_src");
}

// ---- the same with a diffuse tail that is coherent between the rows of the call: DESIGN.md "Shoebox IRs: the coherent tail"
int al_ism_shoebox_coherent(const double *sources, int32_t n_sources, const double *source_patterns, const double *receivers,
                            int32_t n_receivers, const double *patterns, int32_t n_channels, const double *L, const double *beta,
                            double air, double c, double fs, int32_t max_order, int32_t ir_len, int32_t pitch, int64_t mix, int64_t fade,
                            uint64_t seed, int64_t source_id0, int64_t capsule_id0, const double *ln_env, int32_t n_knots,
                            const double *taps, const int32_t *delays, int32_t n_waves, int32_t n_taps, int64_t group_id, float *out,
                            al_stream_t stream) {
  al::IsmDirJob job;   // ln_env: (rows, N, n_knots), as al_ism_shoebox_src
  if (mix < 0) return al::fail(AL_E_BADARG, "al_ism_shoebox_coherent: mix must be >= 0");
  if (int rc = al::ism_images_prepare(sources, n_sources, source_patterns, receivers, n_receivers, patterns, n_channels, L, beta, air, c, fs,
                                      max_order, ir_len, pitch, mix, fade, seed, source_id0, capsule_id0, ln_env, n_knots,
                                      (int64_t)n_knots * n_sources, n_knots, out, &job))
    return rc;
  if (int rc = al::ism_coherent_prepare(taps, delays, n_waves, n_taps, group_id, &job.base)) return rc;
  al::launch_ism_coherent(job, (hipStream_t)stream);
  return check_launch("k_ism_ctail");
}

int al_ism_shoebox_bands_src(const double *sources, int32_t n_sources, const double *source_patterns, const double *capsules,
                             int32_t n_capsules, const double *L, const double *beta, int32_t n_bands, const double *filters,
                             int32_t half, const double *air, double c, double fs, int32_t max_order, int32_t ir_len, int32_t pitch,
                             int64_t mix, int64_t fade, uint64_t seed, int64_t source_id0, int64_t capsule_id0, const double *ln_env,
                             int32_t n_knots, void *workspace, int64_t workspace_bytes, float *out, al_stream_t stream) {
  al::IsmBandJob job;
  if (int rc = al::ism_bands_prepare(sources, n_sources, capsules, n_capsules, L, beta, n_bands, filters, half, c, fs, max_order, ir_len,
                                     pitch, mix, fade, seed, source_id0, capsule_id0, ln_env, n_knots, workspace, workspace_bytes, out, &job))
    return rc;
  if (int rc = al::ism_bands_source_prepare(source_patterns, air, mix >= 0, &job)) return rc;
  al::launch_ism_shoebox_bands(job, mix >= 0, true, (hipStream_t)stream);
  return check_launch("k_ism_bands_src");
}

// ---- capsules on a rigid sphere (arrays, a spherical head): DESIGN.md "Shoebox IRs: rigid-sphere receivers"
int64_t al_ism_shoebox_sphere_workspace_bytes(int32_t n_orders, int32_t half, int32_t ir_len, int64_t mix, int64_t fade) {
  return al::ism_rows_workspace_bytes("al_ism_shoebox_sphere", "n_orders", n_orders, al::ISM_SPHERE_MAX_ORDERS, half, al::ISM_SPHERE_MAX_HALF,
                                      ir_len, mix, fade);
}

int al_ism_shoebox_sphere(const double *sources, int32_t n_sources, const double *source_patterns, const double *centre,
                          const double *directions, int32_t n_capsules, const double *L, const double *beta, double air,
                          const double *filters, int32_t n_orders, int32_t half, const double *diffuse, double c, double fs,
                          int32_t max_order, int32_t ir_len, int32_t pitch, int64_t mix, int64_t fade, uint64_t seed, int64_t source_id0,
                          int64_t capsule_id0, const double *ln_env, int32_t n_knots, void *workspace, int64_t workspace_bytes, float *out,
                          al_stream_t stream) {
  al::IsmSphereJob job;
  if (int rc = al::ism_sphere_prepare(sources, n_sources, source_patterns, centre, directions, n_capsules, L, beta, air, filters, n_orders,
                                      half, diffuse, c, fs, max_order, ir_len, pitch, mix, fade, seed, source_id0, capsule_id0, ln_env,
                                      n_knots, workspace, workspace_bytes, out, &job))
    return rc;
  al::launch_ism_shoebox_sphere(job, mix >= 0, (hipStream_t)stream);
  return check_launch("k_ism_sphere");
}

// ---- room-acoustic metrics of an IR tensor where it lies: DESIGN.md "IR metrics"
int64_t al_ir_metrics_workspace_bytes(int32_t n_capsules, int32_t n_sources, int32_t ir_len) {
  if (n_capsules < 1 || n_sources < 1 || ir_len < 1) return 0;
  return al::irm_workspace_bytes((int64_t)n_capsules * n_sources, ir_len);
}

int al_ir_metrics(const float *irs, int32_t n_capsules, int32_t n_sources, int64_t stride_c, int64_t pitch, int32_t ir_len, double fs,
                  void *workspace, int64_t workspace_bytes, double *out, double *edc, al_stream_t stream) {
  al::IrmJob job;
  if (int rc = al::irm_prepare(irs, n_capsules, n_sources, stride_c, pitch, ir_len, fs, workspace, workspace_bytes, out, edc, &job)) return rc;
  al::launch_ir_metrics(job, (int64_t)n_capsules * n_sources, (hipStream_t)stream);
  return check_launch("k_irm_columns");
}

// ---- the same per octave band, a device band split in front: DESIGN.md "IR metrics: octave bands"
int al_ir_band_split(const float *irs, int32_t n_capsules, int32_t n_sources, int64_t stride_c, int64_t pitch, int32_t ir_len,
                     const double *filters, int32_t n_bands, int32_t half, float *out, int64_t out_pitch, al_stream_t stream) {
  al::IrbJob job;
  if (int rc = al::irb_split_prepare(irs, n_capsules, n_sources, stride_c, pitch, ir_len, filters, n_bands, half, out, out_pitch, &job))
    return rc;
  al::launch_ir_band_split(job, (int64_t)n_capsules * n_sources, (hipStream_t)stream);
  return check_launch("k_ir_band_split");
}

int64_t al_ir_band_metrics_workspace_bytes(int32_t n_bands, int32_t ir_len) { return al::irb_metrics_workspace_bytes(n_bands, ir_len); }

int al_ir_band_metrics(const float *irs, int32_t n_capsules, int32_t n_sources, int64_t stride_c, int64_t pitch, int32_t ir_len,
                       double fs, const double *filters, int32_t n_bands, int32_t half, void *workspace, int64_t workspace_bytes,
                       double *out, double *edc, al_stream_t stream) {
  al::IrbMetricsJob job;
  if (int rc = al::irb_metrics_prepare(irs, n_capsules, n_sources, stride_c, pitch, ir_len, fs, filters, n_bands, half, workspace,
                                       workspace_bytes, out, edc, &job))
    return rc;
  if (int rc = al::launch_ir_band_metrics(job, (hipStream_t)stream)) return rc;
  return check_launch("k_irm_columns");
}

// ---- pairs of rows (IACC, ITD, ILD): DESIGN.md "IR metrics: channel pairs"
int64_t al_ir_pair_metrics_workspace_bytes(int32_t n_pairs, int32_t n_sources, int32_t ir_len, int32_t max_lag) {
  return al::irp_workspace_bytes(n_pairs, n_sources, ir_len, max_lag);
}

int al_ir_pair_metrics(const float *irs, int32_t n_capsules, int32_t n_sources, int64_t stride_c, int64_t pitch, int32_t ir_len, double fs,
                       const double *rows, const int32_t *pairs, int32_t n_pairs, int32_t max_lag, void *workspace,
                       int64_t workspace_bytes, double *out, double *xcorr, al_stream_t stream) {
  al::IrpJob job;
  if (int rc = al::irp_prepare(irs, n_capsules, n_sources, stride_c, pitch, ir_len, fs, rows, pairs, n_pairs, max_lag, workspace,
                               workspace_bytes, out, xcorr, &job))
    return rc;
  al::launch_ir_pair_metrics(job, (hipStream_t)stream);
  return check_launch("k_irp_columns");
}

int al_resample_poly(const float *x, int32_t rows, int64_t n_in, const float *taps, int32_t half_len, int32_t up, int32_t down,
                     float *out, int64_t n_out, int64_t out_pitch, al_stream_t stream) {
  if (!x || !taps || !out || rows <= 0 || rows > 65535 || n_in <= 0 || half_len < 0 || up <= 0 || down <= 0 || n_out <= 0 ||
      out_pitch < n_out)
    return fail(AL_E_BADARG, "bad resample_poly arguments");
  hipLaunchKernelGGL(al::k_resample_poly, dim3(grid_1d(out_pitch, 4096), rows), dim3(256), 0, (hipStream_t)stream,
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
  hipLaunchKernelGGL(al::k_wrap_copy, dim3(grid_1d(n, 4096)), dim3(256), 0,
                     (hipStream_t)stream, src, m, dst, n);
  return check_launch("k_wrap_copy");
}

}  // extern "C"
