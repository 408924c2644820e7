/*
 * audiblelight_hip.h -- C ABI of the MI355X (gfx950) spatial-audio synthesis path.
 *
 * Drop-in boundary for the hot path of AudibleLight's audiblelight/synthesize.py (reference paths
 * below are relative to the AudibleLight repository).  The reference has no FFI of its own: its
 * boundary is a set of Python functions that mutate Scene/Event objects.  The
 * Python mirror of those functions lives in audiblelight_amd/synthesize.py and calls ONLY the entry
 * points declared here (ctypes).  Every pointer marked "device" is a HIP device pointer to
 * contiguous memory owned by the caller; the library never allocates, never frees, keeps no
 * global state and never synchronises: every call only enqueues kernels on `stream`.
 *
 * Error convention: 0 = success, negative = AL_E_*; al_last_error() returns a thread-local string.
 *
 * Algorithm: uniformly partitioned overlap-save convolution with block size
 * B = 2^log2_block.  Spectra of real 2B-sample windows are stored as B complex floats: bin 0
 * packs (DC, Nyquist) in (re, im), bins 1..B-1 are ordinary.
 */
#ifndef AUDIBLELIGHT_HIP_H
#define AUDIBLELIGHT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS header's struct layouts and entry points.  al_abi_version() returns the value the library was built
 * with; a host must compare it with the AL_ABI_VERSION it was compiled against before passing any struct (al_batch and
 * al_mix grew fields in version 2: clip_scale, xspec/hspec_zero_block, ambience, ambience_scale; version 3 puts
 * struct_size + abi_version at the head of both, so a descriptor built against another header is refused, not misread;
 * version 4 appends al_batch.emitter_parts; version 5 adds the host-side planner (al_plan_*, al_workspace_bytes,
 * al_plan_mixdown) and the AL_FLAG_QUAD_SPECTRA / AL_FLAG_FUSED_MOVING path: no struct changed; version 6 adds
 * al_plan_batch_flags -- the dispatch policy (layout + accumulate flags per chunk) moves from the hosts into the library --
 * and al_scale_rows_f64; the opt-in fused kernels of versions 2-5 (AL_FLAG_FUSED_STATIC / _FUSED_MOVING / _FUSED_NJ5,
 * al_mac_synthesis, al_fused_supported, al_moving_fused_supported, the quad layout at B = 8192, the fused_moving argument of
 * al_plan_emitter_parts) are gone: measured 20-35 % slower than the stored-spectra path, profiles/r05c_fused_ab.txt).  The
 * batched FX entries (al_fx_batch_*) were added within version 6: new entry points only, no struct or entry changed. */
#define AL_ABI_VERSION 6

#define AL_OK 0
#define AL_E_BADARG (-1)
#define AL_E_HIP (-2)
#define AL_E_UNSUPPORTED (-3)

/* al_batch.flags */
#define AL_FLAG_NO_IR_NORM 1 /* IRs are already normalised: emitter_gain := 1 (time_invariant_convolution,
                                 time_variant_convolution called directly, synthesize.py:71,277) */

#define AL_FLAG_SPLIT_SPECTRA 32 /* spectra in the split layout of csrc/al_split.h (even bins | odd bins, every window transformed
                                    as two half-size FFTs); all of al_ir_spectra / al_signal_spectra / al_block_synthesis must
                                    see the same setting; the accumulate does not care.  B >= 2048 */
#define AL_FLAG_STATIC_MAC 64   /* al_spectral_mac: static (one-emitter) events of batches with at most 21 partitions through k_spectral_mac_static (one workgroup per
                                   (event, k-tile, bin tile) looping over the capsules); the tile kernels skip them */
#define AL_FLAG_ONLY_STATIC 128 /* with AL_FLAG_STATIC_MAC: the batch has no multi-emitter event, so the other accumulate
                                   kernels are not launched at all (the host knows the event table, the library does not) */
#define AL_FLAG_QUAD_SPECTRA 256 /* with AL_FLAG_SPLIT_SPECTRA at B = 16384: the four-tile layout of csrc/al_quad16.h (every window as
                                    four 4096-point transforms) -- set both there: the one- / two-transform kernels are 15-20 %
                                    slower per scene at that block size.  Ignored at other block sizes.  al_plan_batch_flags sets
                                    the layout flags for the plan's block size */
#define AL_FLAG_NARROW_FFT 4 /* A/B switch: 16 complex values per thread at every block size (default: 32 from
                               B = 8192 up, see csrc/al_fft.h) */
/* A/B switches of the capsule-loop accumulate (AL_FLAG_STATIC_MAC); the default of each is the faster path where both exist
   (profiles/r02_mac.txt, profiles/r03_p24_ab.txt).  The result is the same to rounding; al_spectral_mac_variant reports the choice. */
#define AL_FLAG_MAC_ONE_KTILE (1 << 12)   /* one k-tile of 12 blocks per workgroup (default: two from 13 blocks up) */
#define AL_FLAG_MAC_NO_LDS_RING (1 << 13) /* clips of more than 24 blocks through the register kernel k_spectral_mac_static<12,P,2>
                                             too (default there: the partition spectra staged through LDS, k_spectral_mac_static_lds) */
#define AL_FLAG_MAC_LDS_DMA (1 << 14)     /* at most 12 partitions through the LDS-DMA kernel k_spectral_mac_static_glds too, from 13
                                             blocks up (default: only 13..21 partitions go through it) */
#define AL_FLAG_SYNTH_RUN(n) (((n) & 0xff) << 16) /* al_block_synthesis: n consecutive blocks per workgroup (0 = 1) */
#define AL_FLAG_IR_RUN(n) (((n) & 0x7f) << 24)    /* al_ir_spectra: n consecutive partitions per workgroup (0 = 1; the B = 16384 quad-tile
                                                     kernels: 0 = chosen per batch, equal runs, csrc/al_quad16.h) */

#define AL_SPARSE_MAX_NJ 6          /* longest stream (in blocks) the sliding-window accumulate accepts */
#define AL_SPARSE_MAX_PARTITIONS 24 /* most IR partitions it accepts */
#define AL_STATIC_MAC_MAX_PARTITIONS 21 /* most IR partitions the capsule-loop accumulate (AL_FLAG_STATIC_MAC) takes */

#define AL_MIN_LOG2_BLOCK 10
#define AL_MAX_LOG2_BLOCK 14

typedef void *al_stream_t; /* hipStream_t */

/* One event as render_event_audio sees it (synthesize.py:507-608; attribute list SURVEY 8a A15). */
typedef struct {
  int64_t audio_off;  /* first sample of the mono clip inside `audio` */
  int64_t out_off;    /* first element of this event's (C, len) block inside `spatial` */
  int32_t len;        /* clip samples La = output samples per capsule (synthesize.py:553,590) */
  int32_t valid_len;  /* convolution samples kept before zero padding: La for static events,
                         min(La, n_frames*hop - win) for moving ones (synthesize.py:274,590) */
  int32_t n_blocks;   /* K = ceil(len / B) output blocks */
  int32_t stream0;    /* first entry of this event in the stream table */
  int32_t n_streams;  /* emitters: 1 static, >1 moving (synthesize.py:564-587), 0 = tiled dry clip */
  int32_t yspec_base; /* block index of (c=0,k=0) inside yspec; layout [c][k] */
  int32_t part_base;  /* index of (c=0,k=0) inside the partial-statistics array; layout [c][k] */
  float snr;          /* Event.snr */
  float ref_db;       /* Scene.ref_db (synthesize.py:598) */
  int32_t reserved;   /* 1: moving event whose streams all have n_j <= AL_SPARSE_MAX_NJ (sliding-window accumulate) */
} al_event;

/* One (event, emitter) source stream: the clip weighted by that emitter's cross-fade envelope
 * (time_variant_convolution, synthesize.py:277-310, in the envelope form of SURVEY 8a A7). */
typedef struct {
  int32_t event;    /* owning event */
  int32_t emitter;  /* column of the IR tensor (synthesize.py:662) */
  int32_t j_lo;     /* first non-zero signal block */
  int32_t n_j;      /* number of non-zero signal blocks */
  int32_t xspec_base; /* block index of block j_lo inside xspec */
  int32_t w_off;    /* offset of this stream's frame weights W[:, l] in `wtab`, -1 = static (env == 1) */
  int32_t w_len;    /* number of frames n_frames = min(F_a, W.shape[0]) (synthesize.py:208-210) */
  float gain;       /* clip gain folded into the spectrum (peak normalisation event.py:535-536,
                       sample-wise FX gain/polarity, x fft_size for moving events) */
} al_stream;

/* Everything one launch sequence needs.  All pointers are device pointers unless noted. */
typedef struct {
  int32_t struct_size;  /* sizeof(al_batch) as the CALLER compiled it, and the AL_ABI_VERSION it was compiled against: every */
  int32_t abi_version;  /* entry point refuses a descriptor whose two fields differ from the library's own (AL_E_BADARG) */
  int32_t log2_block;   /* B = 1 << log2_block */
  int32_t n_capsules;   /* C */
  int32_t n_events;     /* E */
  int32_t n_streams;    /* S */
  int32_t n_emitters;   /* columns of the IR tensor used by this batch: [emitter0, emitter0 + n_emitters) */
  int32_t ir_len;       /* Lir samples per IR row */
  int64_t ir_stride_c;  /* elements between capsules  (multiple of 4) */
  int64_t ir_stride_n;  /* elements between emitters (multiple of 4) */
  int32_t n_partitions; /* P = ceil(ir_len / B) */
  int32_t max_blocks;   /* max over events of n_blocks */
  int32_t max_nj;       /* max over streams of n_j */
  int32_t hop;          /* STFT hop of the moving path (config.py:11), 128 */
  /* Chunking.  A long scene is run as several batches ("chunks") over ONE set of global tables: a chunk
   * covers events [event0, event0+n_events), streams [stream0, stream0+n_streams) and IR columns
   * [emitter0, emitter0+n_emitters).  hspec/xspec/yspec are chunk-local workspaces that every chunk reuses
   * (so they stay in the 256 MiB Infinity Cache instead of round-tripping through HBM): global block
   * indices from the tables are rebased by xspec_block0 / yspec_block0 / emitter0.  ir_energy,
   * emitter_gain, partials, spatial, event_stats and event_scale are indexed globally. */
  int32_t event0;
  int32_t stream0;
  int32_t emitter0;
  int32_t xspec_block0;
  int32_t yspec_block0;
  int32_t flags;        /* AL_FLAG_* */

  const float *twiddle;   /* al_twiddle_init output, B complex */
  const float *audio;     /* mono clips, float32 */
  const float *ir;        /* IR tensor (C, N, Lir) float32: WorldState.get_irs() layout (worldstate.py:2183-2255) */
  const float *wtab;      /* frame weights of moving streams */
  const al_event *events;   /* E entries */
  const al_stream *streams; /* S entries */

  float *ir_energy;  /* workspace: n_emitters * C * P partial sums of ir^2 */
  float *emitter_gain; /* workspace/out: n_emitters, 1 / mean_c ||ir||  (normalize_irs, synthesize.py:404-428); 0 for an emitter whose
                          IRs are all zeros (the reference divides zeros by tiny and keeps zeros) */
  float *hspec;      /* workspace: n_emitters * C * P blocks of B complex, [n - emitter0][c][p] */
  float *xspec;      /* workspace: sum(n_j) blocks of B complex */
  float *yspec;      /* workspace: sum(C * n_blocks) blocks of B complex */
  float *spatial;    /* out: per event (C, len) float32, UNSCALED convolution truncated/padded to len */
  float *partials;   /* workspace: 4 floats per (event, c, k): sum|x|, max|x|, non-finite count, pad */
  double *event_stats; /* out: 4 doubles per event: sum|x|, max|x|, non-finite count, total scale */
  float *event_scale;  /* out: per event multiplier = apply_snr o db_to_multiplier (synthesize.py:594-599), saturated at +-FLT_MAX:
                          a silent render (all-zero clip or IRs) has 10^(dB/20) / tiny here, which the reference multiplies its
                          zeros by in float64 -- silence stays silence, never inf * 0 */
  const float *clip_scale; /* optional (NULL = 1): per event scalar applied to the clip on top of al_stream.gain; written on
                              the device by al_clip_scales (peak normalisation + folded Gain/Invert, event.py:529-536), so
                              the clip's peak never travels to the host.  Indexed globally like event_scale. */
  int32_t xspec_zero_block; /* index of an all-zero block inside xspec / hspec (-1: none): the LDS-DMA accumulate reads the rows past */
  int32_t hspec_zero_block; /* an odd partition count from it instead of masking per lane (13..21 partitions need hspec_zero_block). */
  const int32_t *emitter_parts; /* optional (NULL = n_partitions everywhere), indexed globally by IR column: how many leading
                                   partitions of that IR can reach a block some event keeps.  pad_or_truncate_audio
                                   (synthesize.py:590) drops everything from block n_blocks on, and partition p of an IR whose
                                   signal starts at block j_lo only feeds blocks >= j_lo + p; al_forward_spectra / al_ir_spectra
                                   still read the later partitions (normalize_irs needs their energy) but neither transform nor
                                   store them, and the sliding-window accumulate never reads them.  Must be n_partitions for
                                   the IR of every event that is not a sliding-window (al_event.reserved == 1) event; ignored when n_partitions >
                                   AL_SPARSE_MAX_PARTITIONS (those events then go through the tile accumulate). */
} al_batch;

/* Mixdown of one microphone (generate_scene_audio_from_events, synthesize.py:314-401). */
typedef struct {
  int32_t struct_size;    /* sizeof(al_mix) and AL_ABI_VERSION as the caller compiled them (checked like al_batch's) */
  int32_t abi_version;
  int32_t n_capsules;     /* rows of the scene buffer */
  int32_t n_samples;      /* round(scene.duration * sample_rate) (synthesize.py:331) */
  int32_t tile;           /* samples per time tile: 4096 */
  int32_t n_tiles;        /* ceil(n_samples / tile) */
  int32_t accumulate;     /* 0: scene is overwritten, 1: scene already holds ambience (synthesize.py:335-356) */
  int32_t reserved;
  const int32_t *tile_ptr;  /* n_tiles + 1 */
  const int32_t *tile_events; /* indices into the slot arrays, insertion order inside a tile */
  const int64_t *slot_src;  /* per slot: offset of the event's (C, len) block inside `spatial` */
  const int32_t *slot_len;  /* per slot: event len (row stride) */
  const int32_t *slot_start; /* per slot: max(0, round(scene_start*sr)) (synthesize.py:361) */
  const int32_t *slot_count; /* per slot: samples added = min(end-start, len) (synthesize.py:372-378) */
  const int32_t *slot_rows;  /* per slot: capsules of that event */
  const int32_t *slot_event; /* per slot: index into event_scale */
  const float *spatial;
  const float *event_scale;
  float *scene;             /* (C, n_samples) float32 */
  const float *ambience;       /* optional (NULL = none): (C, n_samples) noise, added as ambience_scale[c] * noise[c] in the */
  const float *ambience_scale; /* same pass that mixes the events (synthesize.py:350-356 fused with :358-383): the scene is */
                               /* written once instead of zeroed and read-modify-written twice.  n_capsules floats: the */
                               /* noise-floor multiplier, times 1/peak of the channel when the noise is handed over */
                               /* un-normalised (al_ambience_scales) */
} al_mix;

const char *al_last_error(void);
int al_abi_version(void);

/* Bytes of the twiddle table for block 2^log2_block; al_twiddle_init fills it (device). */
int64_t al_twiddle_bytes(int log2_block);
int al_twiddle_init(float *twiddle, int log2_block, al_stream_t stream);

/* Stage entry points (each only enqueues).  al_render_batch = stages 1-6 in order. */
int al_ir_spectra(const al_batch *b, al_stream_t stream);      /* A1 energy partials + IR partition spectra */
int al_emitter_gains(const al_batch *b, al_stream_t stream);   /* A1 normalize_irs scalar per emitter */
int al_signal_spectra(const al_batch *b, al_stream_t stream);  /* A13 gain + A7 envelope + block spectra */
int al_forward_spectra(const al_batch *b, al_stream_t stream); /* al_ir_spectra + al_signal_spectra (independent of each other):
                                                                  one launch in the split layout, else the two in turn */
int al_spectral_mac(const al_batch *b, al_stream_t stream);    /* A2/A7 frequency-domain accumulate */
/* Which kernel instantiations al_spectral_mac launches for this batch (no launch; the launcher and this call read the
 * SAME descriptor, so the parity tests' assertion of the regime they cover cannot drift).  *static_code = the kernel that
 * takes one-emitter events: 1000000*KSPLIT + 10000*KT + 100*PT + VB (k-tile, partition tile, bins per thread of the tile
 * kernel k_spectral_mac), or 3120000 + 100*P + D for the capsule-loop kernels (AL_FLAG_STATIC_MAC, P <= 21 partitions):
 * D = 1: k_spectral_mac_static<12,P,1> (clips of at most 12 blocks), 2: <12,P,2> (13..24 blocks), 3: the partition spectra
 * staged through LDS by registers, k_spectral_mac_static_lds<12,P> (more than 24 blocks) or <12,ceil(P/2),2> (13..16
 * partitions without hspec_zero_block), 4: staged by LDS-DMA, k_spectral_mac_static_glds (13..21 partitions as two or three
 * units per capsule, any clip length; needs hspec_zero_block >= 0); *moving_code = 100*NJW + PT of the sliding-window kernel for moving events,
 * 0 = not launched. */
int al_spectral_mac_variant(const al_batch *b, int32_t *static_code, int32_t *moving_code);
int al_block_synthesis(const al_batch *b, al_stream_t stream); /* inverse FFT, A3 truncate/pad, A4/A5 statistics */
int al_event_levels(const al_batch *b, al_stream_t stream);    /* A9 composite level law -> event_scale */
/* The two halves of al_event_levels, for a scene whose capsules are sharded over several GPUs: every rank reduces
 * its own capsules into event_stats[e] = {sum|x|, max|x|, non-finite count, -}, the ranks all-reduce those E triples
 * (SUM, MAX, SUM), then every rank evaluates the level law with the TOTAL capsule count. */
int al_event_stats(const al_batch *b, al_stream_t stream);
/* The same split for normalize_irs (synthesize.py:404-428), whose mean runs over ALL capsules of the microphone:
 * al_emitter_norm_sums leaves sum_c ||h_{n,c}|| over this rank's capsules in emitter_gain[n]; the ranks all-reduce (SUM)
 * that device array; al_emitter_gains_from_sums turns it into total_capsules / sum in place.  No host round trip. */
int al_emitter_norm_sums(const al_batch *b, al_stream_t stream);
int al_emitter_gains_from_sums(const al_batch *b, int32_t total_capsules, al_stream_t stream);
int al_event_levels_from_stats(const al_batch *b, int32_t total_capsules, al_stream_t stream);
int al_render_batch(const al_batch *b, al_stream_t stream);

/* A11 mixdown and helpers. */
int al_mixdown(const al_mix *m, al_stream_t stream);
/* x[r, :] *= scale[r_index] for a (rows, cols) block: scales an event's spatial audio in place
 * (event.spatial_audio, synthesize.py:599,606). scale is a device pointer to ONE float. */
int al_scale_rows(float *x, int64_t n, const float *scale, al_stream_t stream);
/* The same with the scalar read from a DOUBLE on the device (rounded to float32 once): al_batch.event_stats[4 e + 3], the
 * noise-floor multiplier db_to_multiplier(ref_db + snr, mean|x|) alone, which scales the dry render (synthesize.py:598,608 ->
 * :432-504) -- event_scale[e] also carries the apply_snr factor and is not the reference's `event_scale`. */
int al_scale_rows_f64(float *x, int64_t n, const double *scale, al_stream_t stream);
/* A13 on the device, without a host round trip.  al_clip_scales: for every event of the batch, clip_scale[e] =
 * prescale[e] (mode[e] == 0) or prescale[e] / (|prescale[e]| * max|clip_e| + tiny(float32)) (mode[e] == 1): the
 * peak normalisation `a / max(|a| + tiny)` of event.py:535-536 applied to the clip prescale[e] * clip_e, i.e. behind a
 * chain of pure scalar FX (Gain: 10^(dB/20), Invert: -1; augmentation.py:1105-1136,1557-1580).  prescale (float32[E]) and
 * mode (int32[E]) are device arrays indexed like al_batch.events.  al_peak_scale: the same scalar for one buffer. */
int al_clip_scales(const al_batch *b, const float *prescale, const int32_t *mode, al_stream_t stream);
int al_peak_scale(const float *x, int64_t n, float prescale, float *scale_out, al_stream_t stream);
/* y += a * x over n floats; a = *a_dev (ambience add, synthesize.py:350-356). */
int al_axpy(float *y, const float *x, const float *a_dev, int64_t n, al_stream_t stream);
/* Row statistics of a (rows, cols) float32 matrix: out[r] = {sum|x|, max|x|, non-finite count, sum x^2} (doubles). */
int al_row_stats(const float *x, int32_t rows, int64_t cols, float *partials, double *out, al_stream_t stream);
int64_t al_row_stats_partials(int32_t rows, int64_t cols); /* floats needed in `partials` */

/* ---- Sample-wise clip operations (A13 peak normalisation, A14 stateless FX; audiblelight/augmentation.py).
 * All work on float32 device buffers of n samples; ops marked (o) are out-of-place (dst != src).
 * `params` / `iparams` are HOST pointers (scalars copied into the kernel arguments). */
#define AL_FX_GAIN 1      /* x *= p[0]                      Gain (augmentation.py:1105-1136), p[0] = 10^(gain_db/20) */
#define AL_FX_INVERT 2    /* x = -x                         Invert (1557-1580) */
#define AL_FX_REVERSE 3   /* (o) dst[t] = src[n-1-t]        Reverse (1583-1601) */
#define AL_FX_FADE 4      /* x *= fade_in(t) * fade_out(t)  Fade (1403-1554): ip = {n_in, n_out, shape_in, shape_out} */
#define AL_FX_CLIP 5      /* clamp(x, -p[0], p[0])          Clipping (832-868), p[0] = 10^(threshold_db/20) */
#define AL_FX_TANH 6      /* tanh(p[0] * x)                 Distortion (927-960), p[0] = 10^(drive_db/20) */
#define AL_FX_BITCRUSH 7  /* rint(x * p[0]) / p[0]          Bitcrush (266-300), p[0] = 2^bit_depth */
#define AL_FX_PREEMPH 8   /* (o) y[n] = x[n] - c x[n-1], y[0] = x[0] + (2x[0] - x[1])   Preemphasis (1350-1385) */
#define AL_FX_DEEMPH 9    /* (o) inverse of PREEMPH (IIR + extrapolation correction)    Deemphasis (1388-1400) */
#define AL_FADE_LINEAR 0
#define AL_FADE_EXPONENTIAL 1
#define AL_FADE_LOGARITHMIC 2
#define AL_FADE_QUARTER_SINE 3
#define AL_FADE_HALF_SINE 4
#define AL_FADE_NONE 5
int al_fx_apply(int op, const float *src, float *dst, int64_t n, const float *params, const int32_t *iparams,
                al_stream_t stream);
/* TimeWarp* (augmentation.py:1604-1790): dst[t] for t < n is taken from the concatenation of `n_rows` rows of
 * `row_len` samples, row q = {src row r = rows[2q], mode = rows[2q+1]: 0 copy, 1 zeros, 2 reversed}, where src row r
 * is src[r + frame_len * j], j < row_len (the reference iterates librosa.util.frame's (frame_len, n_frames) matrix
 * by rows); the concatenation is wrap-extended to n samples (Augmentation.process, augmentation.py:117-123). */
int al_fx_frame_shuffle(const float *src, float *dst, int64_t n, int32_t frame_len, int32_t row_len,
                        const int32_t *rows, int32_t n_rows, al_stream_t stream);
/* Linear time-invariant filter FX (LowpassFilter, HighpassFilter, LowShelfFilter, HighShelfFilter, MultibandEqualizer;
 * augmentation.py:303-660): dst = the float32 clip src of n samples filtered through n_sections second-order sections in
 * series, every section starting from zero state (scipy.signal.sosfilt with zi=None).  `sos` is a HOST array of n_sections
 * rows {b0, b1, b2, a0, a1, a2} (scipy's sos layout); the library divides each row by its a0.  Coefficients and recursion
 * state are float64, only src and dst are float32.  One launch per call; longer cascades are split over several calls
 * (up to AL_SOS_MAX_SECTIONS sections each).  In place (dst == src) is allowed.
 * AL_E_BADARG for n < 1, n_sections outside 1..AL_SOS_MAX_SECTIONS, a0 == 0, a non-finite coefficient, or a section with a
 * pole of magnitude >= 1; al_last_error() names the reason and the section. */
#define AL_SOS_MAX_SECTIONS 16
int al_fx_sos(const float *src, float *dst, int64_t n, const double *sos, int32_t n_sections, al_stream_t stream);
/* Delay and modulation FX (Delay, Chorus, Phaser; augmentation.py:746-829, 963-1043, 1046-1102).  pedalboard is not vendored:
 * these restate pedalboard 0.9.17's Delay and JUCE's dsp::Chorus / dsp::Phaser as this project reads them, unchecked against
 * a running pedalboard (DESIGN.md "Delay and modulation FX").  src / dst: float32 clips of n samples; every state starts at
 * zero; out of place only (dst must not overlap src).  Recursion state is float64; the LFO phase is exact (float64).
 * AL_E_BADARG, with al_last_error() naming the parameter, for a null pointer, overlap, n < 1, a non-finite or negative
 * parameter, feedback >= 1 (an unstable loop) or fs out of range.
 *
 * al_fx_delay: D = delay_samples (the caller truncates delay_seconds * fs and clamps it to 30 fs); with w[m] = 0 for m < 0,
 *   d[t] = w[t - D], w[t] = x[t] + feedback d[t], y = (1 - mix) x + mix d.  The line is read before it is written, so D = 0
 *   (and D >= n) gives d = 0.  mix is used as given.  (delay_seconds == 0 is the identity: the caller makes no call.)
 * al_fx_chorus: lfo_t = sin(2 pi rate_hz t / fs - pi); tau_t = clamp(max(1, 10 depth lfo_t + centre_delay_ms) fs / 1000, 0,
 *   ceil(110 fs / 1000)) = i_t + f_t; with u[m] = 0 for m < 0: u[t] = x[t] - feedback v[t-1],
 *   v[t] = u[t - i_t] + f_t (u[t - i_t - 1] - u[t - i_t]); y = (1 - m) x + m v, m = min(mix, 1).
 *   fs must satisfy 1000 <= fs and ceil(0.11 fs) + floor(fs / 1000) + 2 <= 16384 (the u history lives in LDS).
 * al_fx_phaser: fmax = min(20000, 0.49 fs), c = log10(fc / 20) / log10(fmax / 20); the LFO ticks at t = 4k:
 *   lfo_k = clamp(0.5 depth sin(2 pi rate_hz 4k / fs - pi) + c, 0, 1), f_k = 20 (fmax / 20)^lfo_k, g = tan(pi f_k / fs),
 *   G = g / (1 + g) for samples 4k .. 4k + 3.  Per sample: in = x - L, six TPT all-passes {v = G (in - s), lp = v + s,
 *   s = lp + v, in = 2 lp - in}, wet = in, L = feedback wet; y = (1 - m) x + m wet, m = min(mix, 1).  0.49 fs must exceed 20. */
int al_fx_delay(const float *src, float *dst, int64_t n, int64_t delay_samples, float feedback, float mix, al_stream_t stream);
int al_fx_chorus(const float *src, float *dst, int64_t n, double fs, double rate_hz, double depth, double centre_delay_ms,
                 double feedback, double mix, al_stream_t stream);
int al_fx_phaser(const float *src, float *dst, int64_t n, double fs, double rate_hz, double depth, double centre_frequency_hz,
                 double feedback, double mix, al_stream_t stream);
/* Dynamics FX (Compressor, Limiter; augmentation.py:663-743, 871-924).  pedalboard is not vendored: these restate JUCE's
 * dsp::Compressor, dsp::BallisticsFilter (peak mode) and dsp::Limiter as pedalboard 0.9.17 wraps them and as this project reads
 * them, unchecked against a running pedalboard (DESIGN.md "Dynamics FX").  src / dst: float32 clips of n samples; every state
 * starts at zero; out of place only (dst must not overlap src).  All arithmetic and state are float64 (JUCE: float32).
 *
 * Coefficients: cte(ms) = 0 when ms < 1e-3, else exp(-2 pi 1000 / (ms fs)); cA = cte(attack_ms), cR = cte(release_ms).
 * A compressor stage (T_dB, ratio, attack_ms, release_ms), T = 10^(T_dB / 20), e[-1] = 0:
 *   a_t = |x_t|;  c_t = cA when a_t > e[t-1], else cR;  e_t = a_t + c_t (e[t-1] - a_t);
 *   g_t = 1 when e_t < T, else (e_t / T)^(1 / ratio - 1);  y_t = g_t x_t.
 * al_fx_compressor: one stage.
 * al_fx_limiter: stage 1 = (-10 dB, 4, 2 ms, 200 ms); stage 2 on its output = (threshold_db, 1000, cA = 0, release_ms) (JUCE's
 *   0.001 ms attack: exp(-2 pi 1e6 / fs) is 0 in any case); y = clamp(G y2, -1, 1), G = 10^(10 (1 - 1/4) / 40) 10^(-threshold_db / 20).
 *   JUCE's smoothed output gain starts at its target (no ramp).
 * The envelope's coefficient depends on its state, so the time axis is walked serially: one wave per clip (a batched launch,
 * below, runs a scene's clips side by side).
 * AL_E_BADARG, with al_last_error() naming the entry and the reason, for a null pointer, n < 1, dst overlapping src, fs not
 * finite or <= 0, threshold_db not finite or <= -200 (JUCE maps it to a zero threshold, whose inverse is infinite), for the
 * limiter threshold_db >= 100, ratio not finite or < 1, attack_ms / release_ms not finite or < 0. */
int al_fx_compressor(const float *src, float *dst, int64_t n, double fs, double threshold_db, double ratio, double attack_ms,
                     double release_ms, al_stream_t stream);
int al_fx_limiter(const float *src, float *dst, int64_t n, double fs, double threshold_db, double release_ms, al_stream_t stream);
/* Time-stretch FX (SpeedUp, PitchShift; augmentation.py:1232-1347).  The reference calls pedalboard.time_stretch (Rubber Band, not
 * vendored): these are pinned by the definition in DESIGN.md "Time-stretch FX" -- librosa 0.11's effects.time_stretch /
 * phase_vocoder restated, and a Kaiser-windowed sinc resampler -- unchecked against a running pedalboard or librosa.
 *
 * al_fx_time_stretch: dst[0 .. n_out) = stretch(src[0 .. n), rate, n_fft, n_out).  hop = n_fft / 4, w[t] = sin^2(pi t / n_fft).
 *   Analysis: x zero-padded by n_fft / 2 on both sides, F = 1 + n / hop frames, D[f] = rfft(w xpad[f hop ..]), D[F] = D[F+1] = 0.
 *   Steps: step_t = t rate (float64) for every t >= 0 with step_t < F (T of them), i_t = floor(step_t), a_t = step_t - i_t.
 *   mag[t][k] = (1 - a_t) |D[i_t][k]| + a_t |D[i_t + 1][k]|;  phi_k = pi hop k / (n_fft / 2);
 *   d = arg D[i_t + 1][k] - arg D[i_t][k] - phi_k, d <- d - 2 pi round(d / 2 pi), inc[t][k] = phi_k + d  (arg 0 = 0).
 *   acc[0][k] = arg D[0][k], acc[t + 1][k] = acc[t][k] + inc[t][k] (float64, reduced mod 2 pi at tile boundaries);
 *   S[t][k] = mag[t][k] e^{i acc[t][k]};  fr[t] = irfft(S[t], n_fft);  y[u] = sum_t w[u - t hop] fr[t][u - t hop],
 *   divided by sum_t w^2[u - t hop] where that exceeds FLT_MIN;  dst[j] = y[n_fft / 2 + j], zero from u = n_fft + hop (T - 1) on.
 *   The analysis transform runs in float64 (an error in arg D would add up over the frames), the synthesis in float32.
 *   Runs on `stream` without a host synchronisation; workspace: al_fx_time_stretch_workspace_floats(n, rate, n_fft) floats,
 *   16-byte aligned (0 for arguments the entry would refuse).
 * al_fx_resample_sinc: dst[0 .. n) from src[0 .. m): c = 0.95 min(1, n / m), H = 16 / c, beta = 8.6, p = t m / n (exact integer
 *   division, int64: i + rem / n), dst[t] = sum_{j in [0, m), |p - j| <= H} src[j] c sinc(c (p - j)) I0(beta sqrt(1 - ((p - j) / H)^2)) / I0(beta),
 *   float64 per output sample.  m == n is a low-pass (c = 0.95), not a copy.
 * AL_E_BADARG, with al_last_error() naming the entry and the reason, for a null pointer (the workspace included), n < 1,
 * n_out < 1, m < 1, dst overlapping src, n_fft not a power of two in [64, 4096], rate not finite or outside [0.25, 4], F or T
 * above 2^30, a workspace that is not 16-byte aligned, m or n of the resampler at or above 2^31. */
int64_t al_fx_time_stretch_workspace_floats(int64_t n, double rate, int32_t n_fft);
int al_fx_time_stretch(const float *src, int64_t n, float *dst, int64_t n_out, double rate, int32_t n_fft, float *workspace,
                       al_stream_t stream);
int al_fx_resample_sinc(const float *src, int64_t m, float *dst, int64_t n, al_stream_t stream);
/* Batched FX launches: the one-workgroup scans (al_fx_sos, al_fx_chorus with feedback > 0, al_fx_phaser, the AL_FX_DEEMPH op
 * of al_fx_apply) and the one-wave walks (al_fx_compressor, al_fx_limiter) on MANY clips in ONE launch, workgroup b running job b exactly as the single-clip entry would (the same
 * kernel, which a single-clip call launches with a grid of 1: the samples are bit-identical).  Three steps:
 *   1. al_fx_batch_pack, on the host, touching no device: checks every job with the checks of its single-clip entry, derives
 *      what that entry derives (run lengths, the transition powers of the sections, the Chorus block, the Phaser constants) and
 *      writes `count` packed descriptors of al_fx_batch_desc_bytes(kind) bytes each to the HOST buffer host_table;
 *   2. the caller copies host_table to device memory (stream-ordered before step 3);
 *   3. al_fx_batch_launch enqueues the one launch of `count` workgroups reading that device table.
 * The job structs: src / dst are device pointers to n float32 samples; the scalars are those of the single-clip entry
 * (al_fx_mod_job.centre: centre_delay_ms for AL_FXB_CHORUS, centre_frequency_hz for AL_FXB_PHASER); al_fx_sos_job.sos is a HOST
 * array of n_sections rows {b0, b1, b2, a0, a1, a2}, read by al_fx_batch_pack only.
 * al_fx_batch_pack returns AL_E_BADARG for an unknown kind, a null pointer or count < 1, and, with al_last_error() naming the
 * job ("al_fx_batch_pack: job 3: ..."), for anything the single-clip entry refuses, for an AL_FXB_CHORUS job with
 * feedback == 0 (that case runs grid-wide through al_fx_chorus) and for a job whose dst range overlaps the src or dst range of
 * ANOTHER job (the workgroups run concurrently; within a job dst == src stays allowed for AL_FXB_SOS, and only there).
 * al_fx_batch_desc_bytes returns -1 for an unknown kind.  The packed layout is private to the library build that wrote it. */
#define AL_FXB_SOS 1
#define AL_FXB_CHORUS 2
#define AL_FXB_PHASER 3
#define AL_FXB_DEEMPH 4
/* 5 is not a kind: it stays refused as unknown, as it was before the dynamics kinds */
#define AL_FXB_COMPRESSOR 6
#define AL_FXB_LIMITER 7
typedef struct al_fx_sos_job {
  const float *src;
  float *dst;
  int64_t n;
  const double *sos;
  int32_t n_sections;
  int32_t reserved;
} al_fx_sos_job;
typedef struct al_fx_mod_job {
  const float *src;
  float *dst;
  int64_t n;
  double fs, rate_hz, depth, centre, feedback, mix;
} al_fx_mod_job;
typedef struct al_fx_deemph_job {
  const float *src;
  float *dst;
  int64_t n;
  float coef;
  int32_t reserved;
} al_fx_deemph_job;
typedef struct al_fx_compressor_job {
  const float *src;
  float *dst;
  int64_t n;
  double fs, threshold_db, ratio, attack_ms, release_ms;
} al_fx_compressor_job;
typedef struct al_fx_limiter_job {
  const float *src;
  float *dst;
  int64_t n;
  double fs, threshold_db, release_ms;
} al_fx_limiter_job;
int64_t al_fx_batch_desc_bytes(int32_t kind);
int al_fx_batch_pack(int32_t kind, const void *jobs, int32_t count, void *host_table);
int al_fx_batch_launch(int32_t kind, const void *device_table, int32_t count, al_stream_t stream);
/* ---- Ambience (A12): Timmer-Koenig (1/f)^beta noise, audiblelight/ambience.py:271-375.
 * The host draws the two standard-normal sets with numpy's default_rng(seed) (PCG64 + ziggurat, ambience.py:351-356:
 * the reference's RNG stream is data-dependent and is not re-implemented on the device); everything after the draws
 * runs here: spectral shaping, DC/Nyquist fix-up, an inverse real FFT of ARBITRARY length n, the 1/sigma scale. */
/* floats of workspace al_noise_irfft needs for `rows` series of length n */
int64_t al_noise_workspace_floats(int32_t rows, int64_t n);
/* out[r, :] = irfft((zr + i zi) * shape)[r] / sigma ; zr, zi: (rows, n/2+1) float32 draws; shape: n/2+1 float32. */
int al_noise_irfft(const float *zr, const float *zi, const float *shape, int32_t rows, int64_t n, float inv_sigma,
                   float *out, float *workspace, al_stream_t stream);
/* The same with the draws made ON THE DEVICE (csrc/al_rng.h: Philox-4x32-10 counters + Box-Muller; (zr, zi) of bin f of row r
 * is a pure function of (seed, r, f)): nothing is drawn, cast or uploaded by the host.  The realisation differs from numpy's
 * for the same seed -- the reference's own tests of this function are statistical (tests/test_ambience.py:30-67) plus
 * fixed-seed reproducibility (:70-76), which this keeps.  shape == NULL: flat (white). */
int al_noise_irfft_seeded(uint64_t seed, const float *shape, int32_t rows, int64_t n, float inv_sigma, float *out,
                          float *workspace, al_stream_t stream);
/* out[i] = scale * N(0,1) for i < n, element i = normal (i % 4) of Philox counter block i / 4 under (seed, tag): "gaussian"
 * ambience (ambience.py:160-165) and white noise, whose Timmer-Koenig synthesis is iid Gaussian in time (flat spectrum). */
int al_normal_fill(float *out, int64_t n, uint64_t seed, uint32_t tag, float scale, al_stream_t stream);
/* Philox-4x32-10 on the HOST (the same function the kernels call), for known-answer tests: all arguments host pointers. */
int al_philox4x32_10(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]);
/* scales[c] = db_to_multiplier(ref_db, mean|normalised noise|) / (normalize ? max|noise_c| + tiny : 1) from al_row_stats'
 * output, on the device (ambience.py:211-214 + synthesize.py:350-356 as one scalar per channel; rows <= 1024).
 * normalize == 2: scales[c] = 1 / (max|noise_c| + tiny) alone (Ambience.load_ambience(normalize=True) without the floor). */
int al_ambience_scales(const double *row_stats, int32_t rows, int64_t cols, float ref_db, int32_t normalize, float *scales,
                       al_stream_t stream);
/* y[r, :] += a_dev[r] * x[r, :] over a (rows, cols) matrix: second and further ambiences of a scene. */
int al_axpy_rows(float *y, const float *x, const float *a_dev, int32_t rows, int64_t cols, al_stream_t stream);
/* x[r, :] *= scale[r]: per-channel peak normalisation (ambience.py:211-214) after al_row_stats. */
int al_scale_matrix_rows(float *x, int32_t rows, int64_t cols, const float *scale, al_stream_t stream);

/* ---- STFT-domain intermediates of the moving-source path (A7).  The render path evaluates the same result in the
 * envelope form (al_signal_spectra / al_spectral_mac); these three give the reference's public helper functions of the
 * same names a device implementation with the reference's array layouts (C order, complex64 as interleaved floats).
 * Any fft_size: Stockham passes of radix 2 / 3 / 4 / 5 / 7 where it factors into those, Bluestein's chirp-z on a power-of-two length
 * otherwise (numpy's rfft / irfft in the reference take any size, synthesize.py:135,263); the workspace functions account for it. */
/* stft (synthesize.py:109-145): y (rows, n) float32 -> spec (rows, n_frames, fft_size/2+1) complex64,
 * n_frames = 2*ceil(n / (2*hop)) + 1, window sin^2(pi t / win), left pad win-hop, rfft norm="backward". */
int64_t al_stft_workspace_floats(int64_t series /* rows * n_frames */, int32_t fft_size);
int al_stft(const float *y, int64_t rows, int64_t n, int32_t fft_size, int32_t win_size, int32_t hop_size, float *spec,
            float *workspace, al_stream_t stream);
/* perform_time_variant_convolution (synthesize.py:184-252): s_audio (F_a, n_freq), s_ir (F_ir, n_freq, n_ch, n_irs)
 * complex64, w_ir (F_w, n_irs) float32 -> out (n_frames, n_freq, n_ch) complex64, n_frames = min(F_a, F_w) (any count: launched in groups of frames). */
int al_tv_stft_mac(const float *s_audio, const float *s_ir, const float *w_ir, int32_t n_frames, int32_t n_frames_ir,
                   int32_t n_freq, int32_t n_ch, int32_t n_irs, float *out, al_stream_t stream);
/* istft_overlap_synthesis (synthesize.py:255-274): spatial_stft (n_frames, n_freq, n_ch) complex64 -> out
 * (n_frames*hop - win, n_ch) float32: irfft(n=fft_size, norm="forward"), overlap-add at i*hop, slice [win, n_frames*hop). */
int64_t al_istft_workspace_floats(int32_t n_frames, int32_t n_ch, int32_t fft_size);
int al_istft_ola(const float *spatial_stft, int32_t n_frames, int32_t n_freq, int32_t n_ch, int32_t fft_size,
                 int32_t win_size, int32_t hop_size, float *out, float *workspace, al_stream_t stream);

/* IR ingest: WorldState.get_irs() hands out float64 (C, N, L) (worldstate.py:2183-2255); this
 * converts to the float32 layout al_batch wants (row pitch `dst_pitch` >= L, multiple of 4, pad zeroed) on the device,
 * so the host never casts 1.6 GB per scene.  rows = C * N. */
int al_pack_irs_f64(const double *src, float *dst, int64_t rows, int32_t len, int32_t dst_pitch, al_stream_t stream);
/* The same re-pitching for float32 IRs whose length is not a multiple of 4 (ragged listeners padded to the longest IR,
 * worldstate.py:2236-2253): the caller's array goes to HBM as it is and is laid out on the device. */
int al_pack_irs_f32(const float *src, float *dst, int64_t rows, int32_t len, int32_t dst_pitch, al_stream_t stream);

/* Ragged ingest: the ray tracer hands out one 1-D IR per (capsule, source) of varying length, which the reference
 * zero-pads into (C, N, maxlen) with a four-deep Python loop run twice (worldstate.py:2196-2253).  Here the IRs are
 * concatenated once (`src`, float32 or float64) and laid out on the device: row r = src[offsets[r] : offsets[r]+lens[r]]
 * followed by zeros up to dst_pitch (multiple of 4).  offsets / lens are device arrays. */
int al_pack_ragged_irs(const void *src, int32_t src_is_f64, const int64_t *offsets, const int32_t *lens, int64_t rows,
                       int32_t dst_pitch, float *dst, al_stream_t stream);
/* Rational-ratio resampling of `rows` series (SOFA IRs at another sample rate, worldstate.py:2995-3006): polyphase FIR,
 * out[m] = sum_j x[j] * taps[m*down - j*up + half_len], m < n_out (zeros up to out_pitch): scipy.signal.resample_poly
 * semantics with the caller's `taps` (2*half_len+1 floats, already scaled by `up`).  The reference calls
 * librosa.resample (soxr), an un-vendored dependency: parity with IT is unpinned; this is pinned to resample_poly. */
int al_resample_poly(const float *x, int32_t rows, int64_t n_in, const float *taps, int32_t half_len, int32_t up, int32_t down,
                     float *out, int64_t n_out, int64_t out_pitch, al_stream_t stream);

/* Output encoding for the WAV writer: (C, T) float32 scene -> (T, C) interleaved frames as
 * soundfile.write(mic_audio.T, sr) stores them (core.py:1840-1847).  AL_FRAMES_PCM16 is soundfile's default subtype for
 * WAV: python-soundfile enables clipping on every file, so libsndfile's f2s_clip_array applies: int16 = lrintf(x * 32768)
 * saturated to [-32768, 32767]; AL_FRAMES_F32 keeps float32.
 * Done on the device so the D2H copy is already the file payload (half the bytes for PCM_16).  `out` may be page-locked host
 * memory; capsule counts that are multiples of 8 (PCM_16) / 4 (float32) are stored 16 bytes per lane and need a 16-byte
 * aligned `out`. */
#define AL_FRAMES_F32 0
#define AL_FRAMES_PCM16 1
int al_encode_frames(const float *scene, int32_t n_capsules, int64_t n_samples, int32_t format, void *out, al_stream_t stream);

/* ---- Planning (host side, no device call; csrc/al_plan.cpp).  Everything al_batch / al_mix point to is index arithmetic on
 * shapes: which signal blocks a moving event's cross-fade windows touch (generate_interpolation_matrix, synthesize.py:148-181),
 * where every event's spectra, statistics and audio live, which events overlap which mixdown tile (event slots with Python's
 * round-half-even, synthesize.py:361-362).  A host builds the tables here, copies them to the device and fills al_batch / al_mix
 * with the device pointers.  The plan owns its arrays; the accessors return HOST pointers valid until al_plan_destroy. */
typedef struct {
  int32_t n_samples;   /* clip length La */
  int32_t n_emitters;  /* len(event): 0 = clip tiled over the capsules, 1 = static, > 1 = moving (synthesize.py:564-587) */
  int32_t emitter0;    /* first IR column of this event (synthesize.py:662) */
  int32_t is_moving;
  float snr;           /* Event.snr */
  float ref_db;        /* Scene.ref_db */
  float gain;          /* scalar folded into the clip (peak normalisation, FX gain / polarity); 1 = none */
  int32_t stft_len;    /* samples the STFT frame count is taken from; 0 = n_samples */
  double duration;     /* Event.duration in seconds (moving events) */
} al_event_spec;

typedef struct {
  int32_t log2_block, n_capsules, ir_len, n_events, n_streams, n_emitters, n_partitions, hop, fft_size;
  int32_t max_blocks;       /* al_batch.max_blocks of the whole batch */
  int32_t max_nj;           /* al_batch.max_nj */
  int32_t max_nj_sliding;   /* longest stream of the sliding-window events */
  int32_t xspec_blocks, yspec_blocks, n_partials;   /* blocks of B complex / entries of 4 floats */
  int32_t reserved;
  int64_t hspec_blocks;     /* n_emitters * n_capsules * n_partitions */
  int64_t audio_floats, spatial_floats, wtab_floats;
} al_plan_info;

typedef struct al_plan al_plan;
typedef struct al_mix_plan al_mix_plan;

typedef struct {            /* what al_mix needs, as host arrays owned by the al_mix_plan */
  int32_t n_capsules, n_samples, tile, n_tiles, n_slots, n_tile_events, n_skipped, reserved;
  const int32_t *tile_ptr;     /* n_tiles + 1 */
  const int32_t *tile_events;  /* max(n_tile_events, 1) */
  const int64_t *slot_src;     /* max(n_slots, 1) entries each, as al_mix documents them */
  const int32_t *slot_len, *slot_start, *slot_count, *slot_rows, *slot_event;
  const int32_t *skipped;      /* n_skipped: events whose slot is empty after rounding (synthesize.py:364-370 warns and skips) */
} al_mix_tables;

typedef struct {            /* the al_batch fields of a chunk of consecutive events (al_plan_chunk) */
  int32_t event0, n_events, stream0, n_streams, emitter0, n_emitters, xspec_block0, xspec_blocks, yspec_block0, yspec_blocks;
  int32_t max_blocks, max_nj;
} al_chunk;

const char *al_plan_last_error(void);
/* The planner is plain host code: it is exported by libaudiblelight_hip.so AND by libaudiblelight_plan.so (csrc/al_plan.cpp alone,
 * no HIP dependency), for hosts that plan on a machine without ROCm; al_plan_abi_version() is what that library answers to. */
int al_plan_abi_version(void);
int32_t al_choose_log2_block(int32_t ir_len, int32_t max_clip);
int32_t al_stft_frame_count(int64_t n_samples, int32_t hop);                          /* synthesize.py:123 */
int32_t al_interpolation_rows(int32_t n_irs, double duration, double sample_rate, int32_t hop);
/* generate_interpolation_matrix (synthesize.py:148-181) for ir_times = linspace(0, duration, n_irs): rows x n_irs float64 */
int al_interpolation_matrix(int32_t n_irs, double duration, double sample_rate, int32_t hop, int32_t rows, double *weights);
/* log2_block <= 0: chosen from the lengths (al_choose_log2_block: 8192 from 4096 samples of IR and clip up), and 16384 in the two
 * situations it was measured to pay (csrc/al_plan.cpp): batches of at least 100 000 (capsule, block) rows of static events with
 * 17..24 partitions of 8192, and batches whose moving events are off the sliding-window accumulate at 8192 but on it at 16384.  Read
 * the choice back from al_plan_info.log2_block and set the layout flags for it (AL_FLAG_SPLIT_SPECTRA at 13, + AL_FLAG_QUAD_SPECTRA
 * at 14).  Errors carry the reference's messages ("Moving Event has only one emitter!", ...). */
int al_plan_create(const al_event_spec *specs, int32_t n_events, int32_t n_capsules, int32_t ir_len, double sample_rate,
                   int32_t log2_block, int32_t hop, int32_t win, int32_t fft_size, al_plan **out);
void al_plan_destroy(al_plan *plan);
int al_plan_get_info(const al_plan *plan, al_plan_info *info);
const al_event *al_plan_events(const al_plan *plan);          /* n_events */
const al_stream *al_plan_streams(const al_plan *plan);        /* n_streams */
const float *al_plan_wtab(const al_plan *plan);               /* wtab_floats */
const int64_t *al_plan_audio_offsets(const al_plan *plan);    /* n_events: where each clip goes inside `audio` */
/* A run of consecutive events as one al_batch over the plan's global tables (a scene too large for one spectra workspace is
 * rendered chunk by chunk over ONE reused workspace sized for the largest chunk; results are identical to one batch). */
int al_plan_chunk(const al_plan *plan, int32_t event0, int32_t n_events, al_chunk *out);
/* bytes of the spectra workspaces + statistics of the whole batch as ONE chunk (hspec, xspec, yspec, ir_energy, emitter_gain, partials) */
int64_t al_workspace_bytes(const al_plan *plan);
/* al_batch.emitter_parts: returns 1 and fills out[n_emitters] if the batch needs the table, 0 if every IR needs all partitions */
int al_plan_emitter_parts(const al_plan *plan, int32_t *out);
/* Dispatch policy: al_batch.flags for a chunk of the plan (chunk == NULL: the whole plan as one batch) -- the layout flags for
 * the plan's block size (AL_FLAG_SPLIT_SPECTRA at 8192, + AL_FLAG_QUAD_SPECTRA at 16384) and the accumulate flags for the chunk's
 * event mix (AL_FLAG_STATIC_MAC when it has one-emitter events and at most AL_STATIC_MAC_MAX_PARTITIONS partitions, +
 * AL_FLAG_ONLY_STATIC when it has no multi-emitter event).  This IS the configuration bench.py times: a host that ORs the result
 * into al_batch.flags (plus AL_FLAG_NO_IR_NORM where it applies) runs the same kernels as audiblelight_amd/engine.py, which
 * calls this too; al_spectral_mac_variant on the finished descriptor tells which. */
int al_plan_batch_flags(const al_plan *plan, const al_chunk *chunk, int32_t *flags);
int al_plan_mixdown(const double *starts, const double *ends, const int32_t *lens, const int32_t *rows, const int64_t *src_offsets,
                    const int32_t *event_index, int32_t n, double duration, double sample_rate, int32_t n_capsules, int32_t tile,
                    al_mix_plan **out);
void al_mix_plan_destroy(al_mix_plan *plan);
int al_mix_plan_get(const al_mix_plan *plan, al_mix_tables *tables);

/* Shoebox room impulse responses by the image-source method (DESIGN.md "Shoebox IRs"; kernel: csrc/al_ism.h), written straight into
 * the (C, N, pitch) float32 layout al_batch.ir reads (ir_stride_c = N * pitch, ir_stride_n = pitch).  For p in {0,1}^3 and m in Z^3,
 * per axis (x shown): R_x = (1 - 2 p_x) s_x + 2 m_x L_x - r_x, k_x0 = |m_x - p_x|, k_x1 = |m_x|; d = |R|, tau = d fs / c samples,
 * order = sum of the six k, a = prod beta^k / (4 pi d) with 0^0 = 1.  An image of order <= max_order (max_order == -1: no limit)
 * adds  a * 0.5 (1 + cos(2 pi (t - tau) / 81)) * sinc(t - tau)  to every integer t in [0, ir_len) with |t - tau| < 40.5.  Each sample
 * is the float64 sum of its taps in one fixed image order, rounded to float32 once: bit-reproducible, a row's bits do not depend on
 * the other rows of the call.  out[(c * n_sources + n) * pitch + t]; the pad samples [ir_len, pitch) are written as zeros.
 *   sources (n_sources, 3), capsules (n_capsules, 3): float64 DEVICE tables of points strictly inside the room, every source at a
 *   distance > 0 from every capsule (not checked: the tables are never read on the host);
 *   L[3] (metres), beta[6] = (x0, x1, y0, y1, z0, z1) in [0, 1]: HOST arrays, read while the launch is built.
 * One launch on `stream`; no allocation, no synchronisation.  Cost without max_order grows as ir_len^3 / (L_x L_y L_z) per pair.
 * AL_E_BADARG: a null pointer, a non-positive or non-finite L, c or fs, a beta outside [0, 1], n_sources < 1, n_capsules < 1,
 * ir_len < 1, pitch < ir_len, pitch % 4 != 0, max_order < -1, more than 2^31 - 1 workgroups ((pitch / 256 rounded up) * pairs), or a
 * room so small that c (ir_len + 42) / fs spans more than 2^20 mirror cells of an axis. */
int al_ism_shoebox(const double *sources, int32_t n_sources, const double *capsules, int32_t n_capsules, const double *L,
                   const double *beta, double c, double fs, int32_t max_order, int32_t ir_len, int32_t pitch, float *out,
                   al_stream_t stream);
/* The same rows with a DIFFUSE TAIL (DESIGN.md "Shoebox IRs: the diffuse tail"): the exact image sum up to a mixing sample, seeded
 * Gaussian noise under an envelope past it.  Everything of al_ism_shoebox stands; further, with M = mix >= 0, F = fade >= 1 and
 * ln_env a float64 DEVICE table of n_knots = (ir_len - 1) / 256 + 2 log-amplitude knots, knot k at sample 256 k, for t in [0, ir_len)
 * of row (c, n):
 *   x = clamp((t - M) / F, 0, 1), w_e = cos(pi x / 2), w_l = sin(pi x / 2): exactly (1, 0) for t <= M, exactly (0, 1) for t >= M + F;
 *   e(t) = exp((1 - p) ln_env[k] + p ln_env[k + 1]), k = t / 256, p = (t % 256) / 256 (p == 0 reads knot k alone);
 *   g(t) = normal number t % 4 of the Philox-4x32-10 block with counter (t / 4, source_id0 + n, 4, capsule_id0 + c) and key
 *          (seed lo, seed hi), Box-Muller as al_normal_fill has it (u1, u2 formed in float32; pairs (x, y) and (z, w));
 *   out[(c * n_sources + n) * pitch + t] = w_e y_ism(t) + w_l e(t) g(t), y_ism the float64 image sum of al_ism_shoebox (max_order still
 *   applies; needed for t < M + F only, and the images past it are never visited), combined in float64 and rounded to float32 once;
 *   where w_l == 0 no noise term is formed.  Pad samples [ir_len, pitch) are +0.
 * A row's bits depend on the room, the pair, the seed and the two ids alone: not on n_sources, n_capsules, the pitch, the grid or
 * the other rows; two runs are identical; with mix >= ir_len the output has the bits of al_ism_shoebox.  Every sample is written
 * exactly once and out is never read.  Two launches on `stream` (the image part below ceil((M + F) / 256) * 256, the tail from there
 * on); no allocation, no synchronisation.
 * AL_E_BADARG: everything al_ism_shoebox refuses; mix < 0; fade < 1; a negative id; source_id0 + n_sources or capsule_id0 +
 * n_capsules above 2^32; n_knots other than (ir_len - 1) / 256 + 2; a null table; an `out` that is not 16-byte aligned (REFUSED, not
 * worked around: the tail is written with 16-byte stores). */
int al_ism_shoebox_tail(const double *sources, int32_t n_sources, const double *capsules, int32_t n_capsules, const double *L,
                        const double *beta, double c, double fs, int32_t max_order, int32_t ir_len, int32_t pitch, int64_t mix,
                        int64_t fade, uint64_t seed, int64_t source_id0, int64_t capsule_id0, const double *ln_env, int32_t n_knots,
                        float *out, al_stream_t stream);
/* The same rows for FIRST-ORDER DIRECTIONAL RECEIVERS (DESIGN.md "Shoebox IRs: directional receivers").  `receivers` holds
 * n_receivers positions, each with n_channels (1 .. 4) channels; `patterns` is a float64 DEVICE table (n_receivers, n_channels, 4) of
 * finite (w, vx, vy, vz) in room axes (not checked: the table is never read on the host).  Row c = p * n_channels + k of the output
 * is the image sum of al_ism_shoebox for position p with every amplitude a replaced by a (w + vx ux + vy uy + vz uz), u = R / |R| the
 * direction the image arrives from (R: image position minus receiver); tap shape, reach, order rule and the beta = 0 rule are
 * al_ism_shoebox's.  out[(c * n_sources + n) * pitch + t], c < n_receivers * n_channels; pads are +0.  Every sample is the float64 sum
 * of its taps in the same fixed image order, rounded to float32 once; a row's bits depend on the room, the pair, its position's
 * patterns and n_channels alone, not on n_receivers, n_sources, the pitch or the other positions.  The channels of a position share
 * one image search: one launch of one workgroup per (position, source, tile of 256 samples).
 * AL_E_BADARG: everything al_ism_shoebox refuses (workgroups counted per position); n_channels outside 1 .. 4; a null `patterns`;
 * more than 2^31 - 1 rows. */
int al_ism_shoebox_dir(const double *sources, int32_t n_sources, const double *receivers, int32_t n_receivers, const double *patterns,
                       int32_t n_channels, const double *L, const double *beta, double c, double fs, int32_t max_order, int32_t ir_len,
                       int32_t pitch, float *out, al_stream_t stream);
/* al_ism_shoebox_dir with the diffuse tail of al_ism_shoebox_tail.  Row c draws as capsule capsule_id0 + c and reads ITS OWN knot
 * table: ln_env is a DEVICE table (n_receivers * n_channels, n_knots), n_knots = (ir_len - 1) / 256 + 2.  With mix >= ir_len the output
 * has the bits of al_ism_shoebox_dir.  AL_E_BADARG: everything al_ism_shoebox_dir and al_ism_shoebox_tail refuse, the id range and the
 * tail's workgroup limit counted over the n_receivers * n_channels rows. */
int al_ism_shoebox_dir_tail(const double *sources, int32_t n_sources, const double *receivers, int32_t n_receivers,
                            const double *patterns, int32_t n_channels, const double *L, const double *beta, double c, double fs,
                            int32_t max_order, int32_t ir_len, int32_t pitch, int64_t mix, int64_t fade, uint64_t seed,
                            int64_t source_id0, int64_t capsule_id0, const double *ln_env, int32_t n_knots, float *out,
                            al_stream_t stream);

/* The same rows with FREQUENCY-DEPENDENT WALLS in n_bands (1 .. 8) bands (DESIGN.md "Shoebox IRs: frequency-dependent walls").
 * beta is a HOST array (6, n_bands): column b holds the six reflection coefficients of band b.  filters is a float64 DEVICE table
 * (n_bands, 2 half + 1) of zero-phase FIRs phi_b[j], j = -half .. half (shoebox.band_filters: the table IS the definition; not checked,
 * never read on the host).  With y_b[s] the float64 image sum of al_ism_shoebox under beta[:, b] at every integer s in
 * [-half, ir_len + half) -- negative s included, the row boundary does not truncate a band sum --
 *   out[(c * n_sources + n) * pitch + t] = float32( sum_b sum_{j = -half .. half} phi_b[j] y_b[t - j] ),
 * the double sum in float64 in the order b ascending, then j ascending, rounded once; pad samples [ir_len, pitch) are +0.  A row's
 * bits depend on the room, the pair, beta, the table and half alone: not on n_sources, n_capsules, the pitch, the other rows or
 * workspace_bytes; two runs are identical.
 * workspace: DEVICE memory, 16-byte aligned, of workspace_bytes >= al_ism_shoebox_bands_workspace_bytes(n_bands, half, ir_len, -1, 0)
 * (the bytes of ONE pair: n_bands rows of ir_len + 2 half float64 rounded up to 256).  The entry takes workspace_bytes / that many
 * pairs per pass, each pass ceil(n_bands / 4) gathers and one combine, in order on `stream`: the workspace is reused in stream
 * order; no allocation, no synchronisation.  Its contents after the call are unspecified.
 * al_ism_shoebox_bands_workspace_bytes: mix < 0 sizes a row without a tail; mix >= 0 with fade >= 1 sizes the image part of a row
 * with a tail (al_ism_shoebox_bands_tail), min(ir_len, mix + fade) samples.  Negative (AL_E_BADARG) for n_bands outside
 * 1 .. 8, half outside 1 .. 4096, ir_len < 1, or mix >= 0 with fade < 1.
 * AL_E_BADARG: everything al_ism_shoebox refuses, for every band's column; n_bands outside 1 .. 8; half < 1 or half > 4096; a null
 * table; a workspace that is null, not 16-byte aligned or smaller than one pair; a room so small that c (ir_len + half + 42) / fs
 * spans more than 2^20 mirror cells of an axis. */
int64_t al_ism_shoebox_bands_workspace_bytes(int32_t n_bands, int32_t half, int32_t ir_len, int64_t mix, int64_t fade);
int al_ism_shoebox_bands(const double *sources, int32_t n_sources, const double *capsules, int32_t n_capsules, const double *L,
                         const double *beta, int32_t n_bands, const double *filters, int32_t half, double c, double fs,
                         int32_t max_order, int32_t ir_len, int32_t pitch, void *workspace, int64_t workspace_bytes, float *out,
                         al_stream_t stream);

/* al_ism_shoebox_bands with the DIFFUSE TAIL of al_ism_shoebox_tail, a decay per band.  ln_env is a float64 DEVICE table
 * (n_bands, n_knots), n_knots = (ir_len - 1) / 256 + 2: band b's log-amplitude knots (shoebox.tail_envelope of beta[:, b]).  M, F, the
 * fade weights w_e, w_l, the draws g(s) of row (c, n) -- zero outside [0, ir_len) -- and the ids are al_ism_shoebox_tail's.  With
 * y_end = min(ir_len, M + F) the band sums y_b are formed for s in [-half, y_end + half) and y(t) as in al_ism_shoebox_bands; with
 *   psi_k[j] = sum_b exp(ln_env[b][k]) phi_b[j]   (a knot of -inf contributes 0),  k = t / 256,  p = (t % 256) / 256,
 *   n(t) = (1 - p) sum_j psi_k[j] g(t - j) + p sum_j psi_{k+1}[j] g(t - j)         (p == 0 reads knot k alone),
 *   out = float32(w_e y(t) + w_l n(t)),  no noise term where w_l == 0,  pads +0.
 * The envelope is interpolated linearly in AMPLITUDE between two knots (al_ism_shoebox_tail interpolates its one envelope in the
 * logarithm, which does not factor out of a sum over bands): two FIRs per sample whatever n_bands is.  Sums are float64, one rounding
 * to float32.  With mix >= ir_len the output has the bits of al_ism_shoebox_bands.  A row's bits depend on the room, the pair, beta,
 * the tables, half, the seed and the two ids alone.  workspace: as al_ism_shoebox_bands, a pair taking
 * al_ism_shoebox_bands_workspace_bytes(n_bands, half, ir_len, mix, fade) bytes.  Per pass ceil(n_bands / 4) gathers and one combine (the
 * samples below ceil((M + F) / 256) * 256), then one launch for the samples from there on of every row; no allocation, no
 * synchronisation.
 * AL_E_BADARG: everything al_ism_shoebox_bands and al_ism_shoebox_tail refuse; half > 1024. */
int al_ism_shoebox_bands_tail(const double *sources, int32_t n_sources, const double *capsules, int32_t n_capsules, const double *L,
                              const double *beta, int32_t n_bands, const double *filters, int32_t half, double c, double fs,
                              int32_t max_order, int32_t ir_len, int32_t pitch, int64_t mix, int64_t fade, uint64_t seed,
                              int64_t source_id0, int64_t capsule_id0, const double *ln_env, int32_t n_knots, void *workspace,
                              int64_t workspace_bytes, float *out, al_stream_t stream);

/* The same rows with DIRECTIONAL SOURCES and AIR ABSORPTION (DESIGN.md "Shoebox IRs: directional sources and air").  One entry for
 * omnidirectional and directional receivers, with and without a tail:
 *   source_patterns: float64 DEVICE table (n_sources, 4) of finite (w, vx, vy, vz) in room axes, or NULL (omni sources);
 *   patterns: as al_ism_shoebox_dir, or NULL with n_channels == 1 for omnidirectional capsules (the rows of al_ism_shoebox);
 *   air: amplitude attenuation m >= 0 in Np/m;
 *   mix < 0: no tail, and fade, seed, the ids, ln_env and n_knots are ignored; mix >= 0: the tail of al_ism_shoebox_tail, with ln_env a
 *   DEVICE table (n_receivers * n_channels, n_sources, n_knots): the pair of row c and source n reads table c * n_sources + n.
 * For the image (qx, qy, qz) = 2 m - p with offset R, d = |R| and u = R / d, the ray leaves the real source in the direction e,
 * e_i = -(-1)^{q_i} u_i (a reflection on an axis-i wall flips component i; the direct path leaves along -u).  The image's amplitude in
 * row c is  a (w_s + v_s . e) exp(-m d) (w_c + v_c . u): a of al_ism_shoebox, the last factor 1 for an omni capsule.  Tap shape, reach,
 * order rule, beta = 0 rule and summation order are unchanged.  With omni sources (NULL, or rows (1, 0, 0, 0)) and air == 0 the
 * output has the bits of al_ism_shoebox, al_ism_shoebox_dir and, given the same table for every source, of their _tail entries.
 * AL_E_BADARG: everything those four refuse; air negative or not finite; patterns == NULL with n_channels != 1;
 * n_knots * n_sources >= 2^32.  The launches of the entry it stands for; no allocation, no synchronisation, no atomics. */
int al_ism_shoebox_src(const double *sources, int32_t n_sources, const double *source_patterns, const double *receivers,
                       int32_t n_receivers, const double *patterns, int32_t n_channels, const double *L, const double *beta, double air,
                       double c, double fs, int32_t max_order, int32_t ir_len, int32_t pitch, int64_t mix, int64_t fade, uint64_t seed,
                       int64_t source_id0, int64_t capsule_id0, const double *ln_env, int32_t n_knots, float *out, al_stream_t stream);
/* al_ism_shoebox_src with a diffuse tail that is COHERENT between the rows of the call (DESIGN.md "Shoebox IRs: the coherent tail"): the
 * rows are one group, and the noise g(t) of the tail's definition becomes a sum of n_waves plane waves the group shares,
 *   g(t) = sum_{p < n_waves} sum_{j < n_taps} taps[c][p][j] s_{n,p}(t - delays[c][p] - j)        for row c and source n,
 * in float64, p ascending outside and j ascending inside, each term one fma into an accumulator that starts at 0.  s_{n,p}(m) is
 * normal m & 3 of the Philox-4x32-10 block with counter ((uint32)(m >> 2), source_id0 + n, 5 + 256 p, group_id) and key (seed lo,
 * seed hi), formed in float32 as the tail's normals are and widened; the shift is arithmetic, so a negative m wraps to counter words no
 * sample index reaches.  Mixing sample, fade, envelope (ln_env as al_ism_shoebox_src: a table per (row, source)), the one rounding to
 * float32 and the pads are those of al_ism_shoebox_tail; capsule_id0 is range-checked as there and enters no draw.
 *   taps:   float64 DEVICE table (n_receivers * n_channels, n_waves, n_taps);
 *   delays: int32 DEVICE table (n_receivers * n_channels, n_waves).  THE TABLES' CONTRACT: every entry D satisfies -256 <= D and
 *           D + n_taps - 1 <= 256.  The tables are not read on the host; the caller answers for the limit.
 * A row's bits depend on the room, the pair, the seed, source_id0 + n, group_id and its own rows of the two tables alone; with
 * mix >= ir_len they are those of al_ism_shoebox_src.  Every sample is written once and out is never read.
 * AL_E_BADARG: everything al_ism_shoebox_src refuses; mix < 0; n_waves outside 1 .. 256; n_taps outside 1 .. 32; a null table;
 * group_id outside [0, 2^32).  Two launches (the image kernel below ceil((M + F) / 256) * 256, one kernel past it); no allocation, no
 * synchronisation, no atomics. */
int al_ism_shoebox_coherent(const double *sources, int32_t n_sources, const double *source_patterns, const double *receivers,
                            int32_t n_receivers, const double *patterns, int32_t n_channels, const double *L, const double *beta,
                            double air, double c, double fs, int32_t max_order, int32_t ir_len, int32_t pitch, int64_t mix, int64_t fade,
                            uint64_t seed, int64_t source_id0, int64_t capsule_id0, const double *ln_env, int32_t n_knots,
                            const double *taps, const int32_t *delays, int32_t n_waves, int32_t n_taps, int64_t group_id, float *out,
                            al_stream_t stream);
/* al_ism_shoebox_bands (mix < 0) or al_ism_shoebox_bands_tail (mix >= 0) with source_patterns as above and air a HOST array of n_bands
 * coefficients m_b: the image sum y_b of band b carries (w_s + v_s . e) exp(-m_b d) per image.  With a tail ln_env is a DEVICE table
 * (n_sources, n_bands, n_knots): source n's band b reads table n * n_bands + b.  The workspace is sized by
 * al_ism_shoebox_bands_workspace_bytes.  AL_E_BADARG: everything the two band entries refuse; a null air; an air[b] negative or not
 * finite. */
int al_ism_shoebox_bands_src(const double *sources, int32_t n_sources, const double *source_patterns, const double *capsules,
                             int32_t n_capsules, const double *L, const double *beta, int32_t n_bands, const double *filters,
                             int32_t half, const double *air, double c, double fs, int32_t max_order, int32_t ir_len, int32_t pitch,
                             int64_t mix, int64_t fade, uint64_t seed, int64_t source_id0, int64_t capsule_id0, const double *ln_env,
                             int32_t n_knots, void *workspace, int64_t workspace_bytes, float *out, al_stream_t stream);

/* The rows of CAPSULES ON A RIGID SPHERE of centre `centre` (HOST, 3 numbers) with the unit directions `directions` (float64 DEVICE
 * table (n_capsules, 3), room axes): a rigid-sphere array or the ears of a spherical head (DESIGN.md "Shoebox IRs: rigid-sphere
 * receivers").  Images are taken relative to the centre: R = image - centre, d = |R|, u = R / d, tau = d fs / c, amplitude A as in
 * al_ism_shoebox_src with omni capsules (source_patterns: DEVICE (n_sources, 4) or NULL; air in Np/m).  Each image reaches the sphere
 * as a plane wave from u.  With mu = clamp(n_c . u, -1, 1) and the Legendre recurrence in float64, in this order,
 *   P_0 = 1,  P_1 = mu,  P_{l+1} = ((2 l + 1) mu P_l - l P_{l-1}) / (l + 1),
 *   y_l[s] = sum over the images of A P_l(mu) tap(s - tau)  at every integer s in [-half, y_end + half),  l = 0 .. n_orders - 1,
 *   y(t)   = sum_l sum_{j = -half .. half} filters[l][j + half] y_l[t - j]   (float64, l ascending, then j ascending),
 * out = float32(y(t)), pads +0.  filters: float64 DEVICE table (n_orders, 2 half + 1), the radial FIRs of the sphere
 * (shoebox.sphere_filters; any table is taken: the radius lives in it alone).  Tap shape, reach, order rule, beta = 0 rule and the
 * canonical image order are al_ism_shoebox's.  mix < 0: no tail (y_end = ir_len; fade, seed, the ids, ln_env, n_knots and diffuse are
 * ignored).  mix >= 0: the tail of al_ism_shoebox_bands_tail with ONE band whose filter is `diffuse` (float64 DEVICE, 2 half + 1 taps:
 * shoebox.sphere_diffuse_filter) and whose knots are ln_env, a DEVICE table (n_sources, n_knots): y_end = min(ir_len, M + F),
 *   n(t) = ((1 - p) exp(ln_env[n][k]) + p exp(ln_env[n][k + 1])) sum_j diffuse[j + half] g(t - j),  out = float32(w_e y(t) + w_l n(t)),
 * row (c, n) drawing as source source_id0 + n at capsule capsule_id0 + c.  With mix >= ir_len the output has the bits of mix < 0; omni
 * source rows and air == 0 give the bits of NULL and 0.  A row's bits depend on the room, the pair, the direction, the tables, half
 * and n_orders (and the seed and ids) alone, not on n_capsules, n_sources, the pitch or the workspace size.
 * workspace: DEVICE, 16-byte aligned, workspace_bytes >= al_ism_shoebox_sphere_workspace_bytes(n_orders, half, ir_len, mix, fade) (one
 * pair: n_orders float64 rows of y_end + 2 half samples rounded up to 256); the pairs are walked in passes of what it holds, per pass
 * ceil(n_orders / 4) gathers and one combine, then one launch for the samples past the split.  No allocation, no synchronisation, no
 * atomics.
 * AL_E_BADARG: everything al_ism_shoebox_src (omni capsules) and the band entries refuse for the arguments they share; n_orders outside
 * 1 .. 64; half outside 1 .. 1024; a null centre, filters or (with a tail) diffuse; a centre that is not finite; the workspace rules. */
int64_t al_ism_shoebox_sphere_workspace_bytes(int32_t n_orders, int32_t half, int32_t ir_len, int64_t mix, int64_t fade);
int al_ism_shoebox_sphere(const double *sources, int32_t n_sources, const double *source_patterns, const double *centre,
                          const double *directions, int32_t n_capsules, const double *L, const double *beta, double air,
                          const double *filters, int32_t n_orders, int32_t half, const double *diffuse, double c, double fs,
                          int32_t max_order, int32_t ir_len, int32_t pitch, int64_t mix, int64_t fade, uint64_t seed, int64_t source_id0,
                          int64_t capsule_id0, const double *ln_env, int32_t n_knots, void *workspace, int64_t workspace_bytes, float *out,
                          al_stream_t stream);

/* ROOM-ACOUSTIC METRICS of an IR tensor where it lies (DESIGN.md "IR metrics").  irs: float32 DEVICE tensor h[c, n, t], c < n_capsules,
 * n < n_sources, t < ir_len = L >= 1, element c * stride_c + n * pitch + t (floats; pitch >= L, stride_c >= n_sources * pitch: what
 * al_ism_shoebox* write and what a view into a larger tensor has).  Samples [L, pitch) are never read.  fs > 0 is the sample rate.
 * The window lengths are integers formed once on the host, round-half-even: w_d = rint(0.0025 fs), w_50 = rint(0.05 fs),
 * w_80 = rint(0.08 fs) (each kept at 2^31 at the most).  Per row, everything in float64:
 *   e[t] = (double)h[t] * (double)h[t] (exact);  E(t) = sum_{u = t}^{L-1} e[u], E(t) = 0 for t >= L  (Schroeder's backward integral)
 *   bad = number of non-finite samples;  peak = max_t |h[t]|;  t0 = the smallest t with |h[t]| == peak;  energy = E(0)
 *   D = sum of e[t] over max(0, t0 - w_d) <= t <= min(L - 1, t0 + w_d) (summed directly);  R = E(t0 + w_d + 1)
 *   drr_db = 10 log10(D / R), +inf when R == 0
 *   X in {50, 80}: early_X = sum of e[t] over t0 <= t < min(L, t0 + w_X) (summed directly), late_X = E(t0 + w_X),
 *                  cX_db = 10 log10(early_X / late_X), +inf when late_X == 0
 *   d50 = early_50 / E(t0);   ts = sum_{t >= t0} (t - t0) e[t] / (fs E(t0))  (centre time, seconds)
 *   three decay fits over (hi, lo) dB: EDT (0, -10), T20 (-5, -25), T30 (-5, -35):
 *     S = { t in [t0, L) : E(t) > E(t0) 10^(lo/10) and (hi == 0 or E(t) <= E(t0) 10^(hi/10)) },  n = |S|
 *     valid when n >= 2 and E(L - 1) <= E(t0) 10^(lo/10) (the decay reaches lo inside the row), else the time is NaN
 *     ordinary least squares of y_t = 10 log10(E(t) / E(t0)) on u = t - t0 over S:
 *     a = (n sum(u y) - sum(u) sum(y)) / (n sum(u^2) - sum(u)^2),  RT = -60 / (a fs) seconds, a == 0 gives NaN
 *     (EDT has no upper test: with one, sample t0 would sit exactly on its threshold)
 *   dyn_db = 10 log10(E(L - 1) / E(t0)): the decay the row has room for (-inf when the last sample is zero)
 *   a silent row (peak == 0): bad = energy = peak = t0 = 0, NaN in every other column;  a row with bad > 0: NaN in every column but bad
 * NO NOISE-FLOOR COMPENSATION (no Lundeby truncation, no subtraction): a measured IR with a noise floor reads long; dyn_db says so.
 * out: float64 DEVICE table (rows, 16), row = c * n_sources + n, columns in this order:
 *   bad, energy, t0, peak, drr_db, c50_db, c80_db, d50, ts, edt, t20, t30, n_edt, n_t20, n_t30, dyn_db
 * edc: NULL, or a float64 DEVICE table (rows, n_knots), n_knots = (L - 1) / 256 + 2: edc[row][k] = E(256 k), so the last knot is 0 (of a
 * row with non-finite samples: what the sum gives, NaN or inf in front of them).  The table has the same bits with and without it.
 * workspace: DEVICE, 16-byte aligned, workspace_bytes >= al_ir_metrics_workspace_bytes(n_capsules, n_sources, ir_len) (0 for extents
 * below 1).  Four launches on `stream`: the tensor is read twice (tiles in front of every window with edc == NULL: once).  Every sum is
 * float64 in an order that depends on ir_len alone (csrc/al_irmetrics.h), so a row's 16 columns and knots have the same bits alone,
 * among other rows, at any pitch or stride_c, and in two runs.  No allocation, no synchronisation, no atomics.
 * AL_E_BADARG: null irs, out or workspace; an extent below 1; pitch < ir_len; stride_c < n_sources * pitch; more than 2^31 - 1 rows or
 * (row, 1024-sample tile) pairs; fs not finite or not positive; a workspace that is too small or not 16-byte aligned. */
int64_t al_ir_metrics_workspace_bytes(int32_t n_capsules, int32_t n_sources, int32_t ir_len);
int al_ir_metrics(const float *irs, int32_t n_capsules, int32_t n_sources, int64_t stride_c, int64_t pitch, int32_t ir_len, double fs,
                  void *workspace, int64_t workspace_bytes, double *out, double *edc, al_stream_t stream);

/* THE SAME PER OCTAVE BAND (DESIGN.md "IR metrics: octave bands").  al_ir_band_split cuts every row of the view al_ir_metrics takes (irs,
 * n_capsules, n_sources, stride_c, pitch, ir_len = L: element c * stride_c + n * pitch + t, samples [L, pitch) never read, any
 * alignment of the rows) into n_bands = B band rows.  filters: float64 DEVICE table (B, 2 half + 1), filters[b][j + half] = phi_b[j]
 * (shoebox.band_filters: zero-phase FIRs that sum to an impulse; any table is taken, never read on the host: the table handed in is the
 * definition).  With row = c * n_sources + n and h taken as +0 outside [0, L):
 *   out[(row * B + b) * out_pitch + t] = float32( sum_{j = -half .. half} phi_b[j] * (double)h[t - j] ),   t < L,
 * one float64 accumulator per output starting at +0, j ascending, every step one fused multiply-add (written as such: the bits do not
 * depend on the compiler's contraction).  The filter's ring in front of sample 0 and past sample L - 1 is cut, so a band row holds
 * slightly less energy than the infinite convolution.  Pads [L, out_pitch) are written +0; every output word is written once.  A
 * non-finite sample spreads over the 2 half + 1 outputs around it in every band.  A band row's bits depend on the row's samples, the
 * table, half and L alone.  One launch, no atomics, all offsets 64-bit.
 * AL_E_BADARG: what al_ir_metrics refuses for irs and the five extents and strides; n_bands outside 1 .. 8; half outside 1 .. 4096; null
 * filters or out; out not 16-byte aligned; out_pitch < ir_len or not a multiple of 4; more than 2^31 - 1 (row, 1024-sample tile of
 * out_pitch) pairs.  A refused call writes nothing.
 * al_ir_band_metrics: the 16 columns and the knots of al_ir_metrics for every band row.  out: float64 DEVICE table (rows, B, 16); edc:
 * NULL or (rows, B, n_knots).  THE CONTRACT: columns and knots of (row, b) carry the bits al_ir_metrics gives for row (row, b) of the
 * tensor al_ir_band_split writes (as a tensor of rows x B rows), whatever pass the row fell into, pitch, stride_c and the other rows
 * are.  t0 of a band is the peak of the BAND row (a zero-phase filter rings before the direct sound).  workspace: DEVICE, 16-byte
 * aligned, workspace_bytes >= al_ir_band_metrics_workspace_bytes(n_bands, ir_len), ONE ROW'S SHARE (its B band rows at the pitch L
 * rounded up to 4, and al_ir_metrics' workspace for them; negative, AL_E_BADARG, for n_bands outside 1 .. 8 or ir_len < 1).  The rows
 * are walked in passes of workspace_bytes / share rows (never more (row, band, tile) triples than al_ir_metrics accepts): per pass one
 * split into the workspace and al_ir_metrics' five launches over it, in order on `stream`.  No allocation, no synchronisation, no atomics.
 * AL_E_BADARG: what al_ir_band_split refuses for the arguments they share; null out or workspace; fs not finite or not positive; a
 * workspace that is not 16-byte aligned or smaller than one row's share. */
int al_ir_band_split(const float *irs, int32_t n_capsules, int32_t n_sources, int64_t stride_c, int64_t pitch, int32_t ir_len,
                     const double *filters, int32_t n_bands, int32_t half, float *out, int64_t out_pitch, al_stream_t stream);
int64_t al_ir_band_metrics_workspace_bytes(int32_t n_bands, int32_t ir_len);
int al_ir_band_metrics(const float *irs, int32_t n_capsules, int32_t n_sources, int64_t stride_c, int64_t pitch, int32_t ir_len,
                       double fs, const double *filters, int32_t n_bands, int32_t half, void *workspace, int64_t workspace_bytes,
                       double *out, double *edc, al_stream_t stream);

/* PAIRS OF ROWS: inter-aural cross-correlation (ISO 3382-1 Annex B), the lag of its peak (ITD of a binaural pair, TDOA of a capsule
 * pair) and the level difference (DESIGN.md "IR metrics: channel pairs").  The view is al_ir_metrics' (irs, n_capsules, n_sources,
 * stride_c, pitch, ir_len = L: float32 h[c, n, t] at c * stride_c + n * pitch + t, samples [L, pitch) never read, any alignment).
 * rows: the float64 DEVICE table (n_capsules * n_sources, 16) al_ir_metrics wrote for the same view; only its columns bad, energy and
 * t0 are read, and t0 is only ever compared with t, never used to form an address.  pairs: DEVICE int32 table (n_pairs, 2) of capsule
 * indices (a, b).  max_lag = J in 0 .. 1024.  w_80 = rint(0.08 fs), round-half-even, formed once on the host as al_ir_metrics forms it.
 * Per (pair p, source n), x = h[a, n, :] and y = h[b, n, :] widened to float64, y taken as +0 outside [0, L):
 *   T0 = min(t0_a, t0_b);   windows E = [T0, min(L, T0 + w_80)), Lw = [min(L, T0 + w_80), L)
 *   for W in (E, Lw) and j = -J .. J:  r_W[j] = sum_{t in W} x[t] y[t + j]  (the window limits t, not t + j: ISO's integral),
 *                                      exx_W = sum_{t in W} x[t]^2,  eyy_W = sum_{t in W} y[t]^2
 *   the whole window A, one float64 addition each:  r_A[j] = r_E[j] + r_L[j],  exx_A = exx_E + exx_L,  eyy_A = eyy_E + eyy_L
 *   per window: lag_W = the first j, ascending from -J, at which |r_W[j]| is largest;  peak_W = r_W[lag_W] / sqrt(exx_W eyy_W), signed
 *   and not clamped (IACC is its absolute value; a lag moves energy of y across the window's edge, so it can pass 1 slightly);
 *   ild_db_W = 10 log10(exx_W / eyy_W) with the IEEE results at 0.  A positive lag: the sound reaches row a first.
 *   either row with bad > 0: bad = the sum of the two, NaN in every other column.  Either row silent (energy == 0): bad = 0, NaN in
 *   every other column.  An empty window, or exx_W eyy_W == 0: peak_W and lag_W NaN, the other three as computed.  A pair index outside
 *   [0, n_capsules): NaN in every column, and the view is not touched for that pair.
 * out: float64 DEVICE table (n_pairs * n_sources, 17), line = p * n_sources + n, columns in this order:
 *   bad, t0 (= T0; NaN where a table al_ir_metrics did not write holds an infinity), then peak, lag, ild_db, exx, eyy of E, the same
 *   five of Lw, the same five of A
 * xcorr: NULL, or a float64 DEVICE table (n_pairs * n_sources, 2, 2 J + 1) of r_E[j] and r_L[j] (NaN for a line that is NaN by its
 * state).  The table has the same bits with and without it.
 * workspace: DEVICE, 16-byte aligned, workspace_bytes >= al_ir_pair_metrics_workspace_bytes(n_pairs, n_sources, ir_len, max_lag)
 * (2 (2 J + 1) + 4 float64 per (pair x source, 1024-sample tile); negative, AL_E_BADARG, for what is refused).  Two launches on `stream`.
 * Every product is exact in float64 and every sum is float64 in an order that depends on (ir_len, max_lag) alone
 * (csrc/al_irmetrics.h), so a line has the same bits alone, among other pairs, at any pitch or stride_c, with and without xcorr and
 * in two runs.  No allocation, no synchronisation, no atomics.
 * AL_E_BADARG: what al_ir_metrics refuses for irs, out, workspace, the view and fs; null rows or pairs; n_pairs < 1; max_lag outside
 * 0 .. 1024; more than 2^31 - 1 (pair x source, tile) workgroups; a workspace that is too small.  A refused call writes nothing. */
int64_t al_ir_pair_metrics_workspace_bytes(int32_t n_pairs, int32_t n_sources, int32_t ir_len, int32_t max_lag);
int al_ir_pair_metrics(const float *irs, int32_t n_capsules, int32_t n_sources, int64_t stride_c, int64_t pitch, int32_t ir_len, double fs,
                       const double *rows, const int32_t *pairs, int32_t n_pairs, int32_t max_lag, void *workspace,
                       int64_t workspace_bytes, double *out, double *xcorr, al_stream_t stream);

/* dst[t] = src[t mod m] for t < n: np.pad(..., mode="wrap") of Augmentation.process. */
int al_wrap_copy(const float *src, int64_t m, float *dst, int64_t n, al_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
