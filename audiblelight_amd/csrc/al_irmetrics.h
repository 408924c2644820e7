// Room-acoustic metrics of an impulse-response tensor that lies in HBM (al_ir_metrics; DESIGN.md "IR metrics"): the Schroeder
// backward integral E(t) of every row in float64 and, from it, the direct-to-reverberant ratio, the clarities C50 / C80, D50, the
// centre time, the three decay fits EDT / T20 / T30 with their sample counts and the decay the row has room for; optionally the
// curve itself at every 256th sample.  The definition is the header comment of al_ir_metrics in include/audiblelight_hip.h; what
// is here is how it is summed.  The same per octave band (al_ir_band_split, al_ir_band_metrics) is the second part of this file: a
// band split in front of these passes.  The third part measures PAIRS of rows (al_ir_pair_metrics): the windowed cross-correlation of
// two rows behind IACC, ITD and ILD.
//
// THE TILE.  A row is cut into tiles of IRM_TILE = 1024 samples, a tile into 4 sub-tiles of 256; a workgroup is ONE WAVE and lane i owns
// the four samples 4 i .. 4 i + 3 of every sub-tile, so a sub-tile is one 16-byte load per lane and the wave reads 1 KiB in one piece.
// Rows whose base is not 16-byte aligned take scalar loads (chosen per row).  Samples at and past ir_len are never read.  One wave per
// workgroup: the LDS hand-overs below are ordered by the wave's own program order (hipcc drops the s_barrier of __syncthreads()), no
// wave ever waits for another, and the schedule-perturbed builds still sleep around every hand-over.  The code is written for
// IRM_WAVES waves; with one, the sums over the waves behind are empty.
//
// THE ORDER OF E(t) (irm_scan), every term float64, e = (double)h * (double)h exact:
//   inside a thread   E3 = e3, E2 = e2 + E3, E1 = e1 + E2, E0 = e0 + E1                                  (per sub-tile)
//   across a wave     the inclusive suffix scan of the threads' E0 in 6 doubling steps (x_l += x_{l + 2^s})
//   across the waves  the totals of the waves behind this one, from the last backwards (none with one wave per workgroup)
//   across sub-tiles  the totals of the sub-tiles behind this one, added from the last backwards
//   across tiles      suffix[k] = suffix[k + 1] + total[k + 1] from the last tile backwards (k_irm_rows, one thread)
//   E(t) = (own E_k + ((next lane's scan + waves behind) + sub-tiles behind)) + suffix[tile]
// A tile's total is the value this gives at its first sample, so E(t) is the same expression wherever it is formed: in the first
// pass (totals), the second (E(t0)) and the two kernels of the third (every sample).  All terms are >= 0, so a term e reaches E(t) through at most
// 3 (thread) + 6 (wave) + 3 (waves) + 1 + 3 (a sub-tile's total) + 3 (sub-tiles) + 2 (the two outer additions) + 1 (suffix) = 22
// additions inside its tile and one per tile behind it, each a relative rounding of 2^-53 of a partial sum no larger than E(t):
// |E - E_exact| <= (22 + n_tiles) 2^-53 E to first order.
//
// THE PASSES (no atomics; every hand-over is the workspace between two launches of the stream, or LDS behind a barrier):
//   k_irm_tiles    (row, tile)  the tile's total, max |h| with its first index, count of non-finite samples
//   k_irm_rows     row          suffix over the tile totals, peak and t0 (first tile that reaches the maximum), E(t0) by re-reading the
//                               tile that holds t0, the four thresholds
//   k_irm_sums     (row, tile)  re-reads the tile, forms E(t) per sample; each sample decides from t alone which window it belongs to.
//                               The tile's four window sums: workgroup reductions in a fixed shape (irm_block_sum); the knots.  The
//                               four point values E(t0 + w_d + 1), E(t0 + w_50), E(t0 + w_80), E(L - 1) have one sample and so one
//                               writer each.  A tile in front of every window whose knots nobody asked for leaves at once.
//   k_irm_fits     (row, tile)  the fifteen sums of the three fits, each sample deciding from t and E(t) alone: only in the tiles that
//                               reach past t0 and start above the -35 dB threshold (known from the stored total before anything is
//                               read: every other workgroup leaves at once); log10 only for samples above that threshold.
//   k_irm_columns  row          the tile partials, lane-strided and then a shuffle tree (an order that depends on the tile count
//                               alone), and the 16 columns.
// A row's numbers depend on its samples, ir_len and fs alone: not on its place in the tensor, the pitch, the strides or the other rows.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "al_common.h"
#include "al_status.h"

namespace al {

constexpr int IRM_THREADS = 64;                    // one wave: its LDS hand-overs need no s_barrier
constexpr int IRM_WAVES = IRM_THREADS / 64;
constexpr int IRM_SUBS = 4;                        // sub-tiles of a tile
constexpr int IRM_SUB = IRM_THREADS * 4;           // samples of a sub-tile
constexpr int IRM_TILE = IRM_SUBS * IRM_SUB;       // samples of a tile
constexpr int IRM_KNOT = 256;                      // samples between two knots of the curve (shoebox.n_knots_of)
constexpr int IRM_COLS = 16;                       // columns of the table
constexpr int IRM_HEAD = 4;                        // partials of a tile: sum (t - t0) e, D, early_50, early_80 ...
constexpr int IRM_FIT = 15;                        // ... and n, sum u, sum u^2, sum y, sum u y of EDT, T20, T30
constexpr int IRM_PART = IRM_HEAD + IRM_FIT;
constexpr int IRM_OK = 0, IRM_SILENT = 1, IRM_BAD = 2;

// E(t0) 10^(x/10) for x = -5, -10, -25, -35
#define AL_IRM_M5 0.31622776601683794
#define AL_IRM_M10 0.1
#define AL_IRM_M25 0.0031622776601683794
#define AL_IRM_M35 0.00031622776601683794

struct IrmRow {          // what k_irm_rows leaves for the passes behind it
  double e_t0;           // E(t0)
  double thr[4];         // E(t0) 10^(x/10), x = -5, -10, -25, -35
  double point[4];       // E(t0 + w_d + 1), E(t0 + w_50), E(t0 + w_80), E(L - 1): zeroed there, written by the sample that holds each
  double energy, bad;    // E(0), count of non-finite samples
  float peak;
  int32_t t0, state, reserved;
};

struct IrmJob {
  const float *irs;
  int32_t n_sources, ir_len, n_tiles, n_knots;
  int64_t stride_c, pitch, w_d, w_50, w_80;
  double fs;
  double *tile_total, *tile_suffix, *partials;   // (rows, n_tiles), (rows, n_tiles), (rows, n_tiles, IRM_PART)
  IrmRow *rows;
  float *tile_peak;                              // (rows, n_tiles)
  int32_t *tile_arg, *tile_bad;
  double *out, *edc;
};

inline int64_t irm_tiles(int32_t ir_len) { return ((int64_t)ir_len + IRM_TILE - 1) / IRM_TILE; }

inline int64_t irm_workspace_bytes(int64_t rows, int32_t ir_len) {
  const int64_t pairs = rows * irm_tiles(ir_len);
  return pairs * (int64_t)((2 + IRM_PART) * sizeof(double) + sizeof(float) + 2 * sizeof(int32_t)) + rows * (int64_t)sizeof(IrmRow);
}

// round-half-even of x fs, kept below 2^31 (a window longer than any row is past the end of every row)
inline int64_t irm_window(double seconds, double fs) {
  const double w = nearbyint(seconds * fs);
  return w < 2147483648.0 ? (int64_t)w : (int64_t)2147483648LL;
}

// what al_ir_metrics and al_ir_pair_metrics check alike: the three pointers, the view, fs and the workspace's alignment
inline int irm_check(const char *entry, const float *irs, int32_t n_capsules, int32_t n_sources, int64_t stride_c, int64_t pitch,
                     int32_t ir_len, double fs, const void *workspace, const double *out) {
  if (!irs || !out || !workspace) return fail_arg(entry, "irs, out and workspace must not be null");
  if (n_capsules < 1 || n_sources < 1 || ir_len < 1) return fail_arg(entry, "n_capsules, n_sources and ir_len must be >= 1");
  if (pitch < ir_len) return fail_arg(entry, "pitch < ir_len");
  if (pitch > INT64_MAX / n_sources || stride_c < (int64_t)n_sources * pitch) return fail_arg(entry, "stride_c < n_sources * pitch");
  const int64_t rows = (int64_t)n_capsules * n_sources, tiles = irm_tiles(ir_len);
  if (rows > 0x7fffffff) return fail_arg(entry, "more than 2^31 - 1 rows");
  if (rows * tiles > 0x7fffffff) return fail_arg(entry, "more than 2^31 - 1 (row, tile) pairs");
  if (!(fs > 0.0) || !(fs <= 1.7976931348623157e308)) return fail_arg(entry, "fs must be finite and positive");
  if (((uintptr_t)workspace & 15) != 0) return fail_arg(entry, "workspace must be 16-byte aligned");
  return AL_OK;
}

inline int irm_prepare(const float *irs, int32_t n_capsules, int32_t n_sources, int64_t stride_c, int64_t pitch, int32_t ir_len, double fs,
                       void *workspace, int64_t workspace_bytes, double *out, double *edc, IrmJob *job) {
  const char *entry = "al_ir_metrics";
  if (int rc = irm_check(entry, irs, n_capsules, n_sources, stride_c, pitch, ir_len, fs, workspace, out)) return rc;
  const int64_t rows = (int64_t)n_capsules * n_sources, tiles = irm_tiles(ir_len);
  if (workspace_bytes < irm_workspace_bytes(rows, ir_len)) return fail_arg(entry, "workspace_bytes < al_ir_metrics_workspace_bytes(...)");
  const int64_t pairs = rows * tiles;
  job->irs = irs;
  job->n_sources = n_sources; job->ir_len = ir_len; job->n_tiles = (int32_t)tiles; job->n_knots = (ir_len - 1) / IRM_KNOT + 2;
  job->stride_c = stride_c; job->pitch = pitch;
  job->w_d = irm_window(0.0025, fs); job->w_50 = irm_window(0.05, fs); job->w_80 = irm_window(0.08, fs);
  job->fs = fs;
  job->tile_total = static_cast<double *>(workspace);
  job->tile_suffix = job->tile_total + pairs;
  job->partials = job->tile_suffix + pairs;
  job->rows = reinterpret_cast<IrmRow *>(job->partials + pairs * IRM_PART);
  job->tile_peak = reinterpret_cast<float *>(job->rows + rows);
  job->tile_arg = reinterpret_cast<int32_t *>(job->tile_peak + pairs);
  job->tile_bad = job->tile_arg + pairs;
  job->out = out; job->edc = edc;
  return AL_OK;
}

// ---------------------------------------------------------------------------------------------------------------- device side
__device__ __forceinline__ const float *irm_row_base(const IrmJob &job, int64_t row) {
  const int64_t c = row / job.n_sources, n = row % job.n_sources;
  return job.irs + c * job.stride_c + n * job.pitch;
}

// the thread's 16 samples of the tile that starts at tile0: v[j][k] is sample tile0 + j IRM_SUB + 4 tid + k, 0 at and past L
__device__ __forceinline__ void irm_load(const float *row, int64_t tile0, int64_t L, int tid, float (&v)[IRM_SUBS][4]) {
  const bool wide = ((uintptr_t)row & 15) == 0;
#pragma unroll
  for (int j = 0; j < IRM_SUBS; ++j) {
    const int64_t t = tile0 + (int64_t)j * IRM_SUB + 4 * tid;
    if (wide && t + 4 <= L) {
      const float4 q = *reinterpret_cast<const float4 *>(row + t);
      v[j][0] = q.x; v[j][1] = q.y; v[j][2] = q.z; v[j][3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[j][k] = t + k < L ? row[t + k] : 0.f;
    }
  }
}

// E[j][k]: the sum of e over this sample and every later one of the tile, in the order of the head comment; returns the tile's total
// (E of its first sample) to every thread.  lds: IRM_WAVES IRM_SUBS + 1 doubles of this call's own.
__device__ __forceinline__ double irm_scan(const float (&v)[IRM_SUBS][4], double (&E)[IRM_SUBS][4], double *lds, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  double x[IRM_SUBS];
#pragma unroll
  for (int j = 0; j < IRM_SUBS; ++j) {
    E[j][3] = (double)v[j][3] * (double)v[j][3];
#pragma unroll
    for (int k = 2; k >= 0; --k) E[j][k] = (double)v[j][k] * (double)v[j][k] + E[j][k + 1];
    x[j] = E[j][0];
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
    for (int j = 0; j < IRM_SUBS; ++j) {
      const double o = __shfl_down(x[j], off, 64);
      if (lane + off < 64) x[j] += o;
    }
  }
  double behind[IRM_SUBS];                    // the scan of the next lane: what lies behind this thread inside its wave
#pragma unroll
  for (int j = 0; j < IRM_SUBS; ++j) {
    const double o = __shfl_down(x[j], 1, 64);
    behind[j] = lane < 63 ? o : 0.0;
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < IRM_SUBS; ++j) lds[wave * IRM_SUBS + j] = x[j];
  }
  __syncthreads();
  double subs = 0.0;                          // the sub-tiles behind sub-tile j
#pragma unroll
  for (int j = IRM_SUBS - 1; j >= 0; --j) {
    double waves = 0.0;                       // the waves behind this one
    for (int w = IRM_WAVES - 1; w > wave; --w) waves += lds[w * IRM_SUBS + j];
    const double add = (behind[j] + waves) + subs;
#pragma unroll
    for (int k = 0; k < 4; ++k) E[j][k] += add;
    double others = 0.0;
    for (int w = IRM_WAVES - 1; w >= 1; --w) others += lds[w * IRM_SUBS + j];
    subs += lds[j] + others;
  }
  if (tid == 0) lds[IRM_WAVES * IRM_SUBS] = E[0][0];
  __syncthreads();
  return lds[IRM_WAVES * IRM_SUBS];
}

// v[i] summed over the workgroup, in thread 0: a shuffle tree inside each wave, then the waves in order.  lds: IRM_WAVES N doubles of this
// call's own.
template <int N>
__device__ __forceinline__ void irm_block_sum(double (&v)[N], double *lds, int tid) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += __shfl_down(v[i], off, 64);
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) lds[(tid >> 6) * N + i] = v[i];
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      double t = lds[i];
      for (int w = 1; w < IRM_WAVES; ++w) t += lds[w * N + i];
      v[i] = t;
    }
  }
}

// ---- pass 1: one workgroup per (row, tile)
__global__ __launch_bounds__(IRM_THREADS) void k_irm_tiles(IrmJob job) {
  __shared__ double scan_lds[IRM_WAVES * IRM_SUBS + 1];
  __shared__ float peak_lds[IRM_WAVES];
  __shared__ int32_t arg_lds[IRM_WAVES], bad_lds[IRM_WAVES];
  const int tid = threadIdx.x;
  const int64_t pair = blockIdx.x, row = pair / job.n_tiles, tile0 = (pair % job.n_tiles) * IRM_TILE, L = job.ir_len;
  const float *base = irm_row_base(job, row);
  float v[IRM_SUBS][4];
  double E[IRM_SUBS][4];
  irm_load(base, tile0, L, tid, v);
  const double total = irm_scan(v, E, scan_lds, tid);
  float peak = 0.f;
  int32_t arg = (int32_t)tile0, bad = 0;       // samples past L are zeros with larger indices: they never win
#pragma unroll
  for (int j = 0; j < IRM_SUBS; ++j) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float a = fabsf(v[j][k]);
      if (a > peak) {                          // strictly: the first of equal maxima stays
        peak = a;
        arg = (int32_t)(tile0 + j * IRM_SUB + 4 * tid + k);
      }
      bad += isfinite(v[j][k]) ? 0 : 1;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float p2 = __shfl_down(peak, off, 64);
    const int32_t a2 = __shfl_down(arg, off, 64);
    bad += __shfl_down(bad, off, 64);
    if (p2 > peak || (p2 == peak && a2 < arg)) {
      peak = p2;
      arg = a2;
    }
  }
  if ((tid & 63) == 0) {
    peak_lds[tid >> 6] = peak;
    arg_lds[tid >> 6] = arg;
    bad_lds[tid >> 6] = bad;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < IRM_WAVES; ++w) {
      if (peak_lds[w] > peak || (peak_lds[w] == peak && arg_lds[w] < arg)) {
        peak = peak_lds[w];
        arg = arg_lds[w];
      }
      bad += bad_lds[w];
    }
    job.tile_total[pair] = total;
    job.tile_peak[pair] = peak;
    job.tile_arg[pair] = arg;
    job.tile_bad[pair] = bad;
  }
}

// ---- pass 2: one workgroup per row
__global__ __launch_bounds__(IRM_THREADS) void k_irm_rows(IrmJob job) {
  __shared__ double scan_lds[IRM_WAVES * IRM_SUBS + 1];
  __shared__ double suffix_lds;
  __shared__ int32_t t0_lds, state_lds;
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x, first = row * job.n_tiles, L = job.ir_len;
  IrmRow *rec = job.rows + row;
  if (tid == 0) {
    double s = 0.0;
    for (int64_t k = job.n_tiles - 1; k >= 0; --k) {
      job.tile_suffix[first + k] = s;
      s += job.tile_total[first + k];
    }
    float peak = 0.f;
    int32_t t0 = 0;
    int64_t bad = 0;
    for (int64_t k = 0; k < job.n_tiles; ++k) {
      if (job.tile_peak[first + k] > peak) {
        peak = job.tile_peak[first + k];
        t0 = job.tile_arg[first + k];
      }
      bad += job.tile_bad[first + k];
    }
    const int32_t state = bad > 0 ? IRM_BAD : peak == 0.f ? IRM_SILENT : IRM_OK;
    rec->energy = s;
    rec->bad = (double)bad;
    rec->peak = peak;
    rec->t0 = t0;
    rec->state = state;
    rec->reserved = 0;
    for (int i = 0; i < 4; ++i) rec->point[i] = rec->thr[i] = 0.0;
    rec->e_t0 = 0.0;
    t0_lds = t0;
    state_lds = state;
    suffix_lds = job.tile_suffix[first + t0 / IRM_TILE];
  }
  __syncthreads();
  if (state_lds != IRM_OK) return;             // the whole workgroup: nothing of such a row is fitted
  const int64_t t0 = t0_lds, tile0 = t0 / IRM_TILE * IRM_TILE;
  float v[IRM_SUBS][4];
  double E[IRM_SUBS][4];
  irm_load(irm_row_base(job, row), tile0, L, tid, v);
  irm_scan(v, E, scan_lds, tid);
  const int64_t at = t0 - tile0;               // the one thread that holds t0
  if ((at % IRM_SUB) / 4 == tid) {
    const int j = (int)(at / IRM_SUB), k = (int)(at % 4);
    double e_t0 = 0.0;
#pragma unroll
    for (int jj = 0; jj < IRM_SUBS; ++jj) {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
        if (jj == j && kk == k) e_t0 = E[jj][kk] + suffix_lds;
    }
    rec->e_t0 = e_t0;
    rec->thr[0] = e_t0 * AL_IRM_M5;
    rec->thr[1] = e_t0 * AL_IRM_M10;
    rec->thr[2] = e_t0 * AL_IRM_M25;
    rec->thr[3] = e_t0 * AL_IRM_M35;
  }
}

// a sample index of the row as an offset from the tile's start, clamped to +-2^30: compared with offsets in [0, IRM_TILE) only
__device__ __forceinline__ int irm_rel(int64_t t, int64_t tile0) {
  const int64_t d = t - tile0;
  return (int)(d < -(1 << 30) ? -(1 << 30) : d > (1 << 30) ? (1 << 30) : d);
}

// ---- pass 3: one workgroup per (row, tile)
__global__ __launch_bounds__(IRM_THREADS) void k_irm_sums(IrmJob job) {
  __shared__ double scan_lds[IRM_WAVES * IRM_SUBS + 1];
  __shared__ double head_lds[IRM_WAVES * IRM_HEAD];
  const int tid = threadIdx.x;
  const int64_t pair = blockIdx.x, row = pair / job.n_tiles, tile = pair % job.n_tiles, tile0 = tile * IRM_TILE, L = job.ir_len;
  const int64_t tile_end = tile0 + IRM_TILE < L ? tile0 + IRM_TILE : L;
  float v[IRM_SUBS][4];
  irm_load(irm_row_base(job, row), tile0, L, tid, v);       // in flight while the row's record is read
  IrmRow *rec = job.rows + row;
  double *part = job.partials + pair * IRM_PART;
  const bool ok = rec->state == IRM_OK;
  const int64_t t0 = rec->t0, t_r = t0 + job.w_d + 1, t_50 = t0 + job.w_50, t_80 = t0 + job.w_80;
  const int64_t d_lo = t0 - job.w_d > 0 ? t0 - job.w_d : 0, d_hi = t0 + job.w_d;
  const int64_t reach = t_80 > t_r ? t_80 : t_r;
  const bool after = ok && tile_end > t0;                                       // sum (t - t0) e runs to the end of the row
  const bool head = ok && tile_end > d_lo && tile0 <= reach;
  if (!after && !head && !job.edc) {           // no window and no knot: nothing of the tile is used (the whole workgroup leaves)
    if (tid < IRM_HEAD) part[tid] = 0.0;
    return;
  }
  double E[IRM_SUBS][4];
  const double suffix = job.tile_suffix[pair];
  irm_scan(v, E, scan_lds, tid);
  // everything below counts samples from the tile's start: i = t - tile0 in [0, IRM_TILE), the row's marks clamped to +-2^30 around it
  const int n_valid = (int)(tile_end - tile0);
  const int r_t0 = irm_rel(t0, tile0), r_r = irm_rel(t_r, tile0), r_50 = irm_rel(t_50, tile0), r_80 = irm_rel(t_80, tile0);
  const int r_lo = irm_rel(d_lo, tile0), r_hi = irm_rel(d_hi, tile0), r_last = irm_rel(L - 1, tile0);
  const double u0 = (double)(tile0 - t0);                                       // t - t0 = u0 + i, exact
  double hs[IRM_HEAD] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int j = 0; j < IRM_SUBS; ++j) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = j * IRM_SUB + 4 * tid + k;
      const double Et = E[j][k] + suffix;
      if (i >= n_valid) continue;
      if (job.edc && k == 0 && (tid & 63) == 0) job.edc[row * job.n_knots + (tile0 + i) / IRM_KNOT] = Et;
      if (!ok) continue;
      const double e = (double)v[j][k] * (double)v[j][k];
      if (i == r_last) rec->point[3] = Et;
      if (head) {                              // (uniform) the tiles the windows reach
        if (i == r_r) rec->point[0] = Et;
        if (i == r_50) rec->point[1] = Et;
        if (i == r_80) rec->point[2] = Et;
        if (i >= r_lo && i <= r_hi) hs[1] += e;
        if (i >= r_t0 && i < r_50) hs[2] += e;
        if (i >= r_t0 && i < r_80) hs[3] += e;
      }
      if (i >= r_t0) hs[0] += (u0 + (double)i) * e;
    }
  }
  if (job.edc && tid == 0 && tile == job.n_tiles - 1) job.edc[row * job.n_knots + job.n_knots - 1] = 0.0;   // E(256 k) at 256 k >= L
  if (after || head) irm_block_sum<IRM_HEAD>(hs, head_lds, tid);
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < IRM_HEAD; ++i) part[i] = after || head ? hs[i] : 0.0;
  }
}

// ---- pass 3, the fits: one workgroup per (row, tile); all but the tiles in which a fit can have samples leave at once
__global__ __launch_bounds__(IRM_THREADS) void k_irm_fits(IrmJob job) {
  __shared__ double scan_lds[IRM_WAVES * IRM_SUBS + 1];
  __shared__ double fit_lds[IRM_WAVES * IRM_FIT];
  const int tid = threadIdx.x;
  const int64_t pair = blockIdx.x, row = pair / job.n_tiles, tile0 = (pair % job.n_tiles) * IRM_TILE, L = job.ir_len;
  const int64_t tile_end = tile0 + IRM_TILE < L ? tile0 + IRM_TILE : L;
  const IrmRow *rec = job.rows + row;
  double *part = job.partials + pair * IRM_PART + IRM_HEAD;
  const int64_t t0 = rec->t0;
  const double suffix = job.tile_suffix[pair], thr35 = rec->thr[3];
  // E at the tile's first sample, the largest of the tile: the stored total is what the scan below returns, bit for bit
  const bool fit = rec->state == IRM_OK && tile_end > t0 && job.tile_total[pair] + suffix > thr35;
  if (!fit) {                                  // (uniform) wholly before t0 or wholly below -35 dB
    if (tid < IRM_FIT) part[tid] = 0.0;
    return;
  }
  float v[IRM_SUBS][4];
  double E[IRM_SUBS][4];
  irm_load(irm_row_base(job, row), tile0, L, tid, v);
  irm_scan(v, E, scan_lds, tid);
  const int n_valid = (int)(tile_end - tile0), r_t0 = irm_rel(t0, tile0);
  const double u0 = (double)(tile0 - t0);
  const double e_t0 = rec->e_t0, thr5 = rec->thr[0], thr10 = rec->thr[1], thr25 = rec->thr[2];
  double ft[IRM_FIT];
#pragma unroll
  for (int i = 0; i < IRM_FIT; ++i) ft[i] = 0.0;
#pragma unroll
  for (int j = 0; j < IRM_SUBS; ++j) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = j * IRM_SUB + 4 * tid + k;
      const double Et = E[j][k] + suffix;
      if (i >= n_valid || i < r_t0 || !(Et > thr35)) continue;
      const double u = u0 + (double)i;
      const double y = 10.0 * log10(Et / e_t0);
      if (Et > thr10) {                        // EDT: no upper test
        ft[0] += 1.0; ft[1] += u; ft[2] += u * u; ft[3] += y; ft[4] += u * y;
      }
      if (Et <= thr5) {
        if (Et > thr25) {
          ft[5] += 1.0; ft[6] += u; ft[7] += u * u; ft[8] += y; ft[9] += u * y;
        }
        ft[10] += 1.0; ft[11] += u; ft[12] += u * u; ft[13] += y; ft[14] += u * y;
      }
    }
  }
  irm_block_sum<IRM_FIT>(ft, fit_lds, tid);
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < IRM_FIT; ++i) part[i] = ft[i];
  }
}

// one decay fit from its five sums: (seconds, or NaN)
__device__ __forceinline__ double irm_fit(const double *s, double e_last, double thr_lo, double fs) {
  const double n = s[0];
  if (!(n >= 2.0) || !(e_last <= thr_lo)) return __builtin_nan("");
  const double a = (n * s[4] - s[1] * s[3]) / (n * s[2] - s[1] * s[1]);
  return a == 0.0 ? __builtin_nan("") : -60.0 / (a * fs);
}

__device__ __forceinline__ double irm_db(double num, double den) { return den == 0.0 ? __builtin_inf() : 10.0 * log10(num / den); }

// ---- pass 4: one wave per row
__global__ __launch_bounds__(64) void k_irm_columns(IrmJob job) {
  const int lane = threadIdx.x;
  const int64_t row = blockIdx.x;
  const IrmRow *rec = job.rows + row;
  const double *part = job.partials + row * job.n_tiles * IRM_PART;
  double s[IRM_PART];
#pragma unroll
  for (int i = 0; i < IRM_PART; ++i) s[i] = 0.0;
  if (rec->state == IRM_OK) {                  // (uniform)
    for (int64_t k = lane; k < job.n_tiles; k += 64) {
#pragma unroll
      for (int i = 0; i < IRM_PART; ++i) s[i] += part[k * IRM_PART + i];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
      for (int i = 0; i < IRM_PART; ++i) s[i] += __shfl_down(s[i], off, 64);
    }
  }
  if (lane != 0) return;
  double *o = job.out + row * IRM_COLS;
  const double nan = __builtin_nan("");
  o[0] = rec->bad;
  if (rec->state != IRM_OK) {
    const bool silent = rec->state == IRM_SILENT;
    o[1] = silent ? 0.0 : nan;
    o[2] = silent ? 0.0 : nan;
    o[3] = silent ? 0.0 : nan;
    for (int i = 4; i < IRM_COLS; ++i) o[i] = nan;
    return;
  }
  const double e_t0 = rec->e_t0, e_last = rec->point[3];
  o[1] = rec->energy;
  o[2] = (double)rec->t0;
  o[3] = (double)rec->peak;
  o[4] = irm_db(s[1], rec->point[0]);
  o[5] = irm_db(s[2], rec->point[1]);
  o[6] = irm_db(s[3], rec->point[2]);
  o[7] = s[2] / e_t0;
  o[8] = s[0] / (job.fs * e_t0);
  o[9] = irm_fit(s + IRM_HEAD, e_last, rec->thr[1], job.fs);
  o[10] = irm_fit(s + IRM_HEAD + 5, e_last, rec->thr[2], job.fs);
  o[11] = irm_fit(s + IRM_HEAD + 10, e_last, rec->thr[3], job.fs);
  o[12] = s[IRM_HEAD];
  o[13] = s[IRM_HEAD + 5];
  o[14] = s[IRM_HEAD + 10];
  o[15] = 10.0 * log10(e_last / e_t0);
}

inline void launch_ir_metrics(const IrmJob &job, int64_t rows, hipStream_t stream) {
  const unsigned pairs = (unsigned)(rows * job.n_tiles);
  hipLaunchKernelGGL(k_irm_tiles, dim3(pairs), dim3(IRM_THREADS), 0, stream, job);
  hipLaunchKernelGGL(k_irm_rows, dim3((unsigned)rows), dim3(IRM_THREADS), 0, stream, job);
  hipLaunchKernelGGL(k_irm_sums, dim3(pairs), dim3(IRM_THREADS), 0, stream, job);
  hipLaunchKernelGGL(k_irm_fits, dim3(pairs), dim3(IRM_THREADS), 0, stream, job);
  hipLaunchKernelGGL(k_irm_columns, dim3((unsigned)rows), dim3(64), 0, stream, job);
}

// =============================================================================================== the octave-band split in front
// BAND ROWS of an IR tensor where it lies (al_ir_band_split, al_ir_band_metrics; DESIGN.md "IR metrics: octave bands").  With phi_b
// the zero-phase FIR of band b (2 half + 1 float64 taps, a device table: shoebox.band_filters; the table handed in is the definition)
// and h taken as +0 outside [0, L):
//   g_b[t] = float32( sum_{j = -half .. half} phi_b[j] (double)h[t - j] ),   one float64 accumulator, j ascending, every step an fma
// (written as fma(): the bits do not depend on what the compiler contracts per basic block, which the schedule-perturbed builds
// split).  The filter's ring past either end of the row is cut: a band row holds the samples [0, L) of the infinite convolution.
// THE KERNEL.  One workgroup of ONE WAVE per (row, tile of IRB_TILE = 1024 outputs).  The row's samples tile0 - half .. tile0 + 1023 +
// half go into LDS ONCE, as float32, and serve all B bands; the taps of a band follow IRB_CHUNK = 256 at a time.  A lane owns
// IRB_PER_LANE = 16 CONSECUTIVE outputs: per tap it reads the tap (a broadcast) and ONE new sample, the other fifteen slide through
// registers as float64 (one conversion per tap), and does 16 float64 multiply-adds into 16 accumulators (the scheme of
// k_ism_band_tail, four times as wide: a quarter of the LDS reads per multiply-add).  The lanes read the segment 16 words apart, which
// on 32 banks would be a 16-way conflict: word i lies at i + i / 16 (irb_at), so the lanes are 17 words apart and no two of a
// 32-lane group share a bank; the segment is shifted by 16 .. 31 words so that the 16 words a lane takes in during one turn of its
// window never straddle a skipped word (one address per turn, 16 immediate offsets).  Four 16-byte stores per lane and band; pads [L, out_pitch) are written +0; every output word has one
// writer.  HCAP (256, 1024, 4096: the smallest that holds `half`) sizes the segment.  One wave: the __syncthreads() order LDS traffic
// only (no barrier instruction), and the perturbed builds sleep around each.
// al_ir_band_metrics walks the rows in PASSES of what its workspace holds: per pass one split into the workspace (float32 band rows at
// the pitch ir_len rounded up to 4) and the five k_irm_* passes above over them as a tensor of (rows in the pass, n_bands) rows, with the
// pass's slice of the tables as targets; all in order on the one stream.  A row's band rows depend on its samples, the table, half and
// ir_len alone, and the metrics on the band rows alone: not on the pass, the pitch, the strides or the other rows.
constexpr int IRB_TILE = 1024;         // outputs of a workgroup
constexpr int IRB_PER_LANE = 16;       // consecutive outputs of a lane
constexpr int IRB_CHUNK = 256;         // taps staged per step
constexpr int IRB_MAX_BANDS = 8;
constexpr int IRB_MAX_HALF = 4096;
static_assert(64 * IRB_PER_LANE == IRB_TILE, "k_ir_band_split: a wave covers a tile");
static_assert(IRB_CHUNK % IRB_PER_LANE == 0, "k_ir_band_split: the window turns a whole number of times per chunk");

struct IrbJob {
  const float *irs;
  const double *filters;               // (n_bands, 2 half + 1), device
  float *out;                          // band rows of the first row of the launch: [row - row0][n_bands][out_pitch]
  int64_t stride_c, pitch, out_pitch;
  int64_t row0;                        // first row of the launch (a pass of al_ir_band_metrics)
  int32_t n_sources, ir_len, n_bands, half;
  int32_t n_tiles;                     // ceil(out_pitch / IRB_TILE)
};

// where word i of the staged segment lies: one word skipped after every 16
__device__ __forceinline__ int irb_at(int i) { return i + (i >> 4); }

template <int HCAP>
__global__ __launch_bounds__(64) void k_ir_band_split(IrbJob job) {
  __shared__ float seg[(IRB_TILE + 2 * HCAP + 32) / 16 * 17];   // sample tile0 - half + i is word i + shift, which lies at irb_at(i + shift)
  __shared__ double tap[IRB_CHUNK];
  const int lane = threadIdx.x;
  const int64_t local = blockIdx.x / (unsigned)job.n_tiles, row = job.row0 + local, L = job.ir_len;
  const int64_t tile0 = (int64_t)(blockIdx.x % (unsigned)job.n_tiles) * IRB_TILE, t0 = tile0 + IRB_PER_LANE * lane;
  const int half = job.half, n_taps = 2 * half + 1;
  float *g = job.out + local * job.n_bands * job.out_pitch;
  if (tile0 >= L) {   // (uniform) a tile of pad samples only; out_pitch is a multiple of 4: a quad is inside the row or outside it
    for (int b = 0; b < job.n_bands; ++b)
#pragma unroll
      for (int q = 0; q < IRB_PER_LANE; q += 4)
        if (t0 + q < job.out_pitch) *reinterpret_cast<float4 *>(g + b * job.out_pitch + t0 + q) = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  // shift in [16, 32) puts the word that enters a lane's window behind tap 16 k on the last word of a run of 16 (2 half - 1 + shift = 15
  // mod 16): the 16 words of one turn of the window then lie side by side, one address per turn
  const int shift = 16 + ((16 - ((2 * half) & 15)) & 15);
  const float *h = job.irs + (row / job.n_sources) * job.stride_c + (row % job.n_sources) * job.pitch;
  const int64_t s_first = tile0 - half;
  for (int i = lane; i < IRB_TILE + 2 * half; i += 64) {
    const int64_t s = s_first + i;
    seg[irb_at(i + shift)] = s >= 0 && s < L ? h[s] : 0.f;   // samples at and past L are never read
  }
  if (lane == 0) seg[irb_at(shift - 1)] = 0.f;   // what lane 0 loads behind the last tap; no output uses it
  __syncthreads();
  // output t0 + q under tap m = j + half reads sample t0 + q + half - m: word at + q - m
  const int at = IRB_PER_LANE * lane + 2 * half + shift;
  for (int b = 0; b < job.n_bands; ++b) {
    const double *phi = job.filters + (int64_t)b * n_taps;
    double acc[IRB_PER_LANE], d[IRB_PER_LANE];
#pragma unroll
    for (int q = 0; q < IRB_PER_LANE; ++q) {
      acc[q] = 0.0;
      d[q] = (double)seg[irb_at(at + q)];
    }
    for (int c0 = 0; c0 < n_taps; c0 += IRB_CHUNK) {
      __syncthreads();   // the reads of the chunk before are over
      for (int k = lane; k < IRB_CHUNK; k += 64) tap[k] = c0 + k < n_taps ? phi[c0 + k] : 0.0;
      __syncthreads();
      const int m_end = min(IRB_CHUNK, n_taps - c0), enter = at - c0 - 1;   // word enter - i comes in behind tap c0 + i
      int i = 0;
      for (; i + IRB_PER_LANE <= m_end; i += IRB_PER_LANE) {   // whole turns: the window comes round, no register moves
        const float *run = seg + irb_at(enter - i);             // word enter - i - k at run[-k], k < 16
#pragma unroll
        for (int k = 0; k < IRB_PER_LANE; ++k) {
          const double w = tap[i + k];
#pragma unroll
          for (int q = 0; q < IRB_PER_LANE; ++q) acc[q] = fma(w, d[q], acc[q]);
#pragma unroll
          for (int q = IRB_PER_LANE - 1; q > 0; --q) d[q] = d[q - 1];
          d[0] = (double)run[-k];
        }
      }
      for (; i < m_end; ++i) {   // the taps past the last whole turn (the last chunk only)
        const double w = tap[i];
#pragma unroll
        for (int q = 0; q < IRB_PER_LANE; ++q) acc[q] = fma(w, d[q], acc[q]);
#pragma unroll
        for (int q = IRB_PER_LANE - 1; q > 0; --q) d[q] = d[q - 1];
        d[0] = (double)seg[irb_at(enter - i)];
      }
    }
    float *gb = g + b * job.out_pitch;
#pragma unroll
    for (int q = 0; q < IRB_PER_LANE; q += 4) {
      if (t0 + q >= job.out_pitch) continue;
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = t0 + q + k < L ? (float)acc[q + k] : 0.f;
      *reinterpret_cast<float4 *>(gb + t0 + q) = make_float4(v[0], v[1], v[2], v[3]);
    }
  }
}

// what al_ir_band_split and al_ir_band_metrics check alike: the view (as al_ir_metrics), the table and the two ranges
inline int irb_check(const char *entry, const float *irs, int32_t n_capsules, int32_t n_sources, int64_t stride_c, int64_t pitch,
                     int32_t ir_len, const double *filters, int32_t n_bands, int32_t half) {
  if (!irs) return fail_arg(entry, "irs must not be null");
  if (n_capsules < 1 || n_sources < 1 || ir_len < 1) return fail_arg(entry, "n_capsules, n_sources and ir_len must be >= 1");
  if (pitch < ir_len) return fail_arg(entry, "pitch < ir_len");
  if (pitch > INT64_MAX / n_sources || stride_c < (int64_t)n_sources * pitch) return fail_arg(entry, "stride_c < n_sources * pitch");
  if ((int64_t)n_capsules * n_sources > 0x7fffffff) return fail_arg(entry, "more than 2^31 - 1 rows");
  if (n_bands < 1 || n_bands > IRB_MAX_BANDS) return fail_arg(entry, "n_bands must be in 1 .. 8");
  if (half < 1 || half > IRB_MAX_HALF) return fail_arg(entry, "half must be in 1 .. 4096");
  if (!filters) return fail_arg(entry, "filters must not be null");
  return AL_OK;
}

inline void irb_fill(IrbJob *job, const float *irs, int32_t n_sources, int64_t stride_c, int64_t pitch, int32_t ir_len,
                     const double *filters, int32_t n_bands, int32_t half, float *out, int64_t out_pitch) {
  job->irs = irs; job->filters = filters; job->out = out;
  job->stride_c = stride_c; job->pitch = pitch; job->out_pitch = out_pitch; job->row0 = 0;
  job->n_sources = n_sources; job->ir_len = ir_len; job->n_bands = n_bands; job->half = half;
  job->n_tiles = (int32_t)((out_pitch + IRB_TILE - 1) / IRB_TILE);
}

inline int irb_split_prepare(const float *irs, int32_t n_capsules, int32_t n_sources, int64_t stride_c, int64_t pitch, int32_t ir_len,
                             const double *filters, int32_t n_bands, int32_t half, float *out, int64_t out_pitch, IrbJob *job) {
  const char *entry = "al_ir_band_split";
  if (int rc = irb_check(entry, irs, n_capsules, n_sources, stride_c, pitch, ir_len, filters, n_bands, half)) return rc;
  if (!out) return fail_arg(entry, "out must not be null");
  if (((uintptr_t)out & 15) != 0) return fail_arg(entry, "out must be 16-byte aligned");
  if (out_pitch < ir_len) return fail_arg(entry, "out_pitch < ir_len");
  if ((out_pitch & 3) != 0) return fail_arg(entry, "out_pitch must be a multiple of 4");
  const int64_t rows = (int64_t)n_capsules * n_sources;
  if (out_pitch > INT64_MAX - IRB_TILE || rows > 0x7fffffff / ((out_pitch + IRB_TILE - 1) / IRB_TILE))
    return fail_arg(entry, "more than 2^31 - 1 (row, 1024-sample tile of out_pitch) pairs: split the call");
  irb_fill(job, irs, n_sources, stride_c, pitch, ir_len, filters, n_bands, half, out, out_pitch);
  return AL_OK;
}

// `rows` rows from job.row0 on
inline void launch_ir_band_split(const IrbJob &job, int64_t rows, hipStream_t stream) {
  const dim3 grid((unsigned)(rows * job.n_tiles)), block(64);
  if (job.half <= 256)
    hipLaunchKernelGGL(k_ir_band_split<256>, grid, block, 0, stream, job);
  else if (job.half <= 1024)
    hipLaunchKernelGGL(k_ir_band_split<1024>, grid, block, 0, stream, job);
  else
    hipLaunchKernelGGL(k_ir_band_split<4096>, grid, block, 0, stream, job);
}

// ---- the band metrics: the split and the five passes above, pass by pass over a capped workspace
struct IrbMetricsJob {
  IrbJob split;                        // out: the band rows at the head of the workspace
  char *metrics_workspace;             // behind the band rows of a full pass
  int64_t metrics_bytes, rows, rows_per_pass;
  double fs, *out, *edc;
};

inline int64_t irb_pitch(int32_t ir_len) { return ((int64_t)ir_len + 3) / 4 * 4; }

// one row's share of the workspace: its n_bands band rows and what al_ir_metrics needs for them, a multiple of 16 bytes
inline int64_t irb_row_bytes(int32_t n_bands, int32_t ir_len) {
  const int64_t bytes = (int64_t)n_bands * irb_pitch(ir_len) * (int64_t)sizeof(float) + irm_workspace_bytes(n_bands, ir_len);
  return (bytes + 15) / 16 * 16;
}

inline int64_t irb_metrics_workspace_bytes(int32_t n_bands, int32_t ir_len) {
  const char *entry = "al_ir_band_metrics_workspace_bytes";
  if (n_bands < 1 || n_bands > IRB_MAX_BANDS) return fail_arg(entry, "n_bands must be in 1 .. 8");
  if (ir_len < 1) return fail_arg(entry, "ir_len must be >= 1");
  return irb_row_bytes(n_bands, ir_len);
}

inline int irb_metrics_prepare(const float *irs, int32_t n_capsules, int32_t n_sources, int64_t stride_c, int64_t pitch, int32_t ir_len,
                               double fs, const double *filters, int32_t n_bands, int32_t half, void *workspace, int64_t workspace_bytes,
                               double *out, double *edc, IrbMetricsJob *job) {
  const char *entry = "al_ir_band_metrics";
  if (int rc = irb_check(entry, irs, n_capsules, n_sources, stride_c, pitch, ir_len, filters, n_bands, half)) return rc;
  if (!out || !workspace) return fail_arg(entry, "out and workspace must not be null");
  if (!(fs > 0.0) || !(fs <= 1.7976931348623157e308)) return fail_arg(entry, "fs must be finite and positive");
  if (((uintptr_t)workspace & 15) != 0) return fail_arg(entry, "workspace must be 16-byte aligned");
  const int64_t per_row = irb_row_bytes(n_bands, ir_len);
  if (workspace_bytes < per_row) return fail_arg(entry, "workspace_bytes < al_ir_band_metrics_workspace_bytes(...) (one row)");
  const int64_t rows = (int64_t)n_capsules * n_sources, P = irb_pitch(ir_len);
  int64_t per_pass = workspace_bytes / per_row;   // ... and no more than al_ir_metrics accepts: (row, band, tile) triples below 2^31
  if (per_pass > rows) per_pass = rows;
  if (per_pass > 0x7fffffff / (n_bands * irm_tiles(ir_len))) per_pass = 0x7fffffff / (n_bands * irm_tiles(ir_len));
  irb_fill(&job->split, irs, n_sources, stride_c, pitch, ir_len, filters, n_bands, half, static_cast<float *>(workspace), P);
  job->metrics_workspace = static_cast<char *>(workspace) + per_pass * n_bands * P * (int64_t)sizeof(float);   // a multiple of 16
  job->metrics_bytes = irm_workspace_bytes(per_pass * n_bands, ir_len);
  job->rows = rows; job->rows_per_pass = per_pass;
  job->fs = fs; job->out = out; job->edc = edc;
  return AL_OK;
}

inline int launch_ir_band_metrics(const IrbMetricsJob &job, hipStream_t stream) {
  IrbJob split = job.split;
  const int32_t B = split.n_bands, L = split.ir_len;
  const int64_t n_knots = (L - 1) / IRM_KNOT + 2;
  for (int64_t row0 = 0; row0 < job.rows; row0 += job.rows_per_pass) {
    const int64_t in_pass = job.rows - row0 < job.rows_per_pass ? job.rows - row0 : job.rows_per_pass;
    split.row0 = row0;
    launch_ir_band_split(split, in_pass, stream);
    IrmJob metrics;   // the band rows as a tensor of (in_pass, B) rows
    if (int rc = irm_prepare(split.out, (int32_t)in_pass, B, B * split.out_pitch, split.out_pitch, L, job.fs, job.metrics_workspace,
                             job.metrics_bytes, job.out + row0 * B * IRM_COLS, job.edc ? job.edc + row0 * B * n_knots : nullptr, &metrics))
      return rc;
    launch_ir_metrics(metrics, in_pass * B, stream);
  }
  return AL_OK;
}

// ======================================================================================================== pairs of rows
// INTERAURAL / INTER-CAPSULE MEASURES of an IR tensor where it lies (al_ir_pair_metrics; DESIGN.md "IR metrics: channel pairs"): per
// (pair (a, b), source n), with x = h[a, n, :], y = h[b, n, :] (+0 outside [0, L)), T0 the earlier of the two rows' t0 and the windows
// E = [T0, min(L, T0 + w_80)), Lw = [min(L, T0 + w_80), L):  r_W[j] = sum_{t in W} x[t] y[t + j] for j = -J .. J,  exx_W = sum x[t]^2,
// eyy_W = sum y[t]^2, and from them the peak of the normalised correlation, its lag and the level difference of the early, the late and
// the whole window.  The definition is the header comment of al_ir_pair_metrics in include/audiblelight_hip.h; what is here is how
// it is summed.
//
// THE TILE.  One workgroup of ONE WAVE per (pair x source, tile of IRP_TILE = 1024 samples t, counted from sample 0 of the row whatever
// T0 is).  x[tile] and y[tile0 - J .. tile0 + 1023 + J] go into LDS once, as float32 (4 KiB and at most 12.3 KiB: JCAP = 64, 256 or
// 1024, the smallest that holds J, sizes the second).  LANES OWN LAGS: lane l holds the lags j = -J + l + 64 k, IRP_BLOCK = 4 values of
// k at a time (then 2, then 1 for what is left of ceil((2 J + 1) / 64)).  The loop over t is uniform over the wave, so the two window
// boundaries cut it into at most two plain ranges and nothing is masked.  Per t the wave reads x[t] once (a broadcast) and, per lag,
// y[t + j] (consecutive lanes, consecutive words: no bank conflict) and does one float64 fused multiply-add per lag.
//
// THE ORDER, every term float64, every product of two float32 exact:
//   r_W[j] of a tile    one accumulator from +0, t ascending over the tile's samples that lie in W, each step one fma()
//   exx_W, eyy_W        the same chain over the same t, of x[t] x[t] and y[t] y[t] (carried by every lane beside the first block of
//   of a tile           lags): for y == x all three are the same bits, so a row against itself correlates to exactly 1
//   across tiles        from +0, the tiles' partials in ascending tile order (k_irp_columns, one lane per lag)
//   the whole window    r_A[j] = r_E[j] + r_L[j], exx_A = exx_E + exx_L, eyy_A = eyy_E + eyy_L: one addition each
// so a term reaches r_W[j], exx_W or eyy_W through at most 1024 + n_tiles additions (+ 1 for A): an order that depends on
// (ir_len, max_lag) alone, a sample being given to its window by comparing t.  T0 is read from the rows table and only ever compared
// with t (clamped to [0, L] first): no address is formed from it.
// THE ARG-MAX over the lags: a lane keeps the first of its lags (ascending) at which |r_W[j]| is largest, then a shuffle tree takes
// the larger |r|, on a tie the smaller j.
//
// THE PASSES (no atomics; the hand-over is the workspace between the two launches of the stream):
//   k_irp_tiles    (pair x source, tile)  the tile's 2 (2 J + 1) + 4 partials; a tile in front of T0 writes zeros and leaves at once;
//                                         a (pair, source) whose line is NaN by its state reads and writes nothing
//   k_irp_columns  pair x source          the tiles added up per (window, lag) -- this is also the optional curve --, the three
//                                         arg-maxima, the 17 columns.  (The issue's second and third kernel in one: the sums over the
//                                         tiles are the lanes' own lags of the arg-max, so nothing needs to be handed over.)
// A (pair, source)'s numbers depend on its two rows, their two lines of the rows table, ir_len, max_lag and fs alone.
constexpr int IRP_TILE = 1024;         // samples t of a workgroup
constexpr int IRP_BLOCK = 4;           // lags a lane carries through one walk over the tile
constexpr int IRP_COLS = 17;
constexpr int IRP_MAX_LAG = 1024;
constexpr int IRP_OK = 0, IRP_SILENT = 1, IRP_BAD = 2, IRP_RANGE = 3;
static_assert(IRP_TILE == IRM_TILE, "al_ir_pair_metrics: the (row, tile) limit of irm_check is counted in these tiles");

struct IrpJob {
  const float *irs;
  const double *rows;                  // (n_capsules n_sources, IRM_COLS): al_ir_metrics' table of the same view; bad, energy, t0 are read
  const int32_t *pairs;                // (n_pairs, 2)
  double *partials;                    // (n_pairs n_sources, n_tiles, 2 n_lags + 4): r_E, r_L, then exx_E, eyy_E, exx_L, eyy_L
  double *out, *xcorr;                 // (n_pairs n_sources, 17); NULL or (n_pairs n_sources, 2, n_lags)
  int64_t stride_c, pitch, w_80;
  int32_t n_capsules, n_sources, ir_len, n_tiles, max_lag, n_lags, n_chunks, n_pairs;
};

// the two extents the workspace is sized by, checked: (pair x source, tile) workgroups through *groups
inline int irp_extent(const char *entry, int32_t n_pairs, int32_t n_sources, int32_t ir_len, int32_t max_lag, int64_t *groups) {
  if (n_pairs < 1) return fail_arg(entry, "n_pairs must be >= 1");
  if (n_sources < 1 || ir_len < 1) return fail_arg(entry, "n_sources and ir_len must be >= 1");
  if (max_lag < 0 || max_lag > IRP_MAX_LAG) return fail_arg(entry, "max_lag must be in 0 .. 1024");
  const int64_t lines = (int64_t)n_pairs * n_sources, tiles = irm_tiles(ir_len);
  if (lines > 0x7fffffff / tiles) return fail_arg(entry, "more than 2^31 - 1 (pair x source, tile) workgroups: split the pairs");
  *groups = lines * tiles;
  return AL_OK;
}

inline int64_t irp_part(int32_t max_lag) { return 2 * (2 * (int64_t)max_lag + 1) + 4; }

inline int64_t irp_workspace_bytes(int32_t n_pairs, int32_t n_sources, int32_t ir_len, int32_t max_lag) {
  int64_t groups;
  if (int rc = irp_extent("al_ir_pair_metrics_workspace_bytes", n_pairs, n_sources, ir_len, max_lag, &groups)) return rc;
  return groups * irp_part(max_lag) * (int64_t)sizeof(double);
}

inline int irp_prepare(const float *irs, int32_t n_capsules, int32_t n_sources, int64_t stride_c, int64_t pitch, int32_t ir_len, double fs,
                       const double *rows, const int32_t *pairs, int32_t n_pairs, int32_t max_lag, void *workspace, int64_t workspace_bytes,
                       double *out, double *xcorr, IrpJob *job) {
  const char *entry = "al_ir_pair_metrics";
  if (int rc = irm_check(entry, irs, n_capsules, n_sources, stride_c, pitch, ir_len, fs, workspace, out)) return rc;
  if (!rows || !pairs) return fail_arg(entry, "rows and pairs must not be null");
  int64_t groups;
  if (int rc = irp_extent(entry, n_pairs, n_sources, ir_len, max_lag, &groups)) return rc;
  if (workspace_bytes < groups * irp_part(max_lag) * (int64_t)sizeof(double))
    return fail_arg(entry, "workspace_bytes < al_ir_pair_metrics_workspace_bytes(...)");
  job->irs = irs; job->rows = rows; job->pairs = pairs;
  job->partials = static_cast<double *>(workspace); job->out = out; job->xcorr = xcorr;
  job->stride_c = stride_c; job->pitch = pitch; job->w_80 = irm_window(0.08, fs);
  job->n_capsules = n_capsules; job->n_sources = n_sources; job->ir_len = ir_len; job->n_tiles = (int32_t)irm_tiles(ir_len);
  job->max_lag = max_lag; job->n_lags = 2 * max_lag + 1; job->n_chunks = (job->n_lags + 63) / 64; job->n_pairs = n_pairs;
  return AL_OK;
}

struct IrpLine {           // what both kernels derive alike for line = pair * n_sources + source
  int32_t state, a, b;
  double bad, t0;          // the two rows' bad added; T0 as the table has it
  int64_t e_lo, e_hi;      // E = [e_lo, e_hi), Lw = [e_hi, L): T0 and T0 + w_80 clamped to [0, L]
};

__device__ __forceinline__ IrpLine irp_line(const IrpJob &job, int64_t line) {
  IrpLine r;
  const int64_t p = line / job.n_sources, n = line % job.n_sources, L = job.ir_len;
  r.a = job.pairs[2 * p];
  r.b = job.pairs[2 * p + 1];
  r.bad = r.t0 = __builtin_nan("");
  r.e_lo = r.e_hi = L;
  r.state = IRP_RANGE;
  if (r.a < 0 || r.a >= job.n_capsules || r.b < 0 || r.b >= job.n_capsules) return r;   // the view is not touched for such a pair
  const double *ra = job.rows + ((int64_t)r.a * job.n_sources + n) * IRM_COLS, *rb = job.rows + ((int64_t)r.b * job.n_sources + n) * IRM_COLS;
  r.bad = ra[0] + rb[0];
  r.state = ra[0] > 0.0 || rb[0] > 0.0 ? IRP_BAD : ra[1] == 0.0 || rb[1] == 0.0 ? IRP_SILENT : IRP_OK;
  if (r.state != IRP_OK) return r;
  r.t0 = fmin(ra[2], rb[2]);
  const double up = ceil(r.t0);                // t >= T0 is t >= ceil(T0); a table of al_ir_metrics holds whole numbers
  if (up == up) {                              // a NaN compares false with every t: both windows stay empty
    const int64_t first = up < -2147483648.0 ? -2147483648LL : up > 2147483648.0 ? 2147483648LL : (int64_t)up;
    r.e_lo = first < 0 ? 0 : first > L ? L : first;
    r.e_hi = first + job.w_80 < r.e_lo ? r.e_lo : first + job.w_80 > L ? L : first + job.w_80;
  }
  return r;
}

// K lags of every lane (index idx0 + 64 q of the 2 J + 1, q < K) over the tile's samples [e0, e1) of window E and [e1, nv) of window Lw;
// with ENERGY the two energies of either window ride along in the same order (yz: y at lag 0, ys + J)
template <int K, bool ENERGY>
__device__ __forceinline__ void irp_lags(const float *xs, const float *yl, const float *yz, int e0, int e1, int nv, double *part, int idx0,
                                         int n_lags) {
  double acc[2][K], en[2][2];
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    en[w][0] = en[w][1] = 0.0;
#pragma unroll
    for (int q = 0; q < K; ++q) acc[w][q] = 0.0;
  }
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    const int first = w == 0 ? e0 : e1, last = w == 0 ? e1 : nv;
#pragma unroll 4
    for (int i = first; i < last; ++i) {
      const double xv = (double)xs[i];
#pragma unroll
      for (int q = 0; q < K; ++q) acc[w][q] = fma(xv, (double)yl[i + 64 * q], acc[w][q]);
      if constexpr (ENERGY) {
        const double yv = (double)yz[i];
        en[w][0] = fma(xv, xv, en[w][0]);
        en[w][1] = fma(yv, yv, en[w][1]);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < K; ++q) {
    const int idx = idx0 + 64 * q;
    if (idx < n_lags) {
      part[idx] = acc[0][q];
      part[n_lags + idx] = acc[1][q];
    }
  }
  if constexpr (ENERGY) {
    if (idx0 == 0) {                           // lane 0 of the first block: exx_E, eyy_E, exx_L, eyy_L
      part[2 * n_lags] = en[0][0];
      part[2 * n_lags + 1] = en[0][1];
      part[2 * n_lags + 2] = en[1][0];
      part[2 * n_lags + 3] = en[1][1];
    }
  }
}

// ---- pass 1: one workgroup per (pair x source, tile)
template <int JCAP>
__global__ __launch_bounds__(64) void k_irp_tiles(IrpJob job) {
  __shared__ float xs[IRP_TILE];
  __shared__ float ys[IRP_TILE + 64 * (JCAP / 32 + 1)];       // sample tile0 - J + i at ys[i], i < IRP_TILE + 64 n_chunks
  const int lane = threadIdx.x;
  const int64_t group = blockIdx.x, line = group / job.n_tiles, tile0 = (group % job.n_tiles) * IRP_TILE, L = job.ir_len;
  const IrpLine ln = irp_line(job, line);
  if (ln.state != IRP_OK) return;              // (uniform) k_irp_columns reads nothing of such a line
  const int J = job.max_lag, n_lags = job.n_lags;
  const int nv = (int)(tile0 + IRP_TILE < L ? IRP_TILE : L - tile0);
  const int e0 = (int)(ln.e_lo - tile0 < 0 ? 0 : ln.e_lo - tile0 > nv ? nv : ln.e_lo - tile0);
  const int e1 = (int)(ln.e_hi - tile0 < 0 ? 0 : ln.e_hi - tile0 > nv ? nv : ln.e_hi - tile0);
  double *part = job.partials + group * (2 * (int64_t)n_lags + 4);
  if (e0 == nv) {                              // (uniform) the tile lies in front of T0: e1 == nv as well, both windows miss it
    for (int i = lane; i < 2 * n_lags + 4; i += 64) part[i] = 0.0;
    return;
  }
  const int64_t n = line % job.n_sources;
  const float *x = job.irs + ln.a * job.stride_c + n * job.pitch, *y = job.irs + ln.b * job.stride_c + n * job.pitch;
  for (int i = lane; i < IRP_TILE; i += 64) xs[i] = tile0 + i < L ? x[tile0 + i] : 0.f;     // samples at and past L are never read
  for (int i = lane; i < IRP_TILE + 64 * job.n_chunks; i += 64) {
    const int64_t s = tile0 - J + i;
    ys[i] = s >= 0 && s < L ? y[s] : 0.f;
  }
  __syncthreads();
  const float *yl = ys + lane, *yz = ys + J;
  int kb = job.n_chunks >= IRP_BLOCK ? IRP_BLOCK : job.n_chunks >= 2 ? 2 : 1;   // the first block of lags carries the energies
  if (kb == IRP_BLOCK)
    irp_lags<IRP_BLOCK, true>(xs, yl, yz, e0, e1, nv, part, lane, n_lags);
  else if (kb == 2)
    irp_lags<2, true>(xs, yl, yz, e0, e1, nv, part, lane, n_lags);
  else
    irp_lags<1, true>(xs, yl, yz, e0, e1, nv, part, lane, n_lags);
  for (; kb + IRP_BLOCK <= job.n_chunks; kb += IRP_BLOCK) irp_lags<IRP_BLOCK, false>(xs, yl + 64 * kb, yz, e0, e1, nv, part, lane + 64 * kb, n_lags);
  if (kb + 2 <= job.n_chunks) {
    irp_lags<2, false>(xs, yl + 64 * kb, yz, e0, e1, nv, part, lane + 64 * kb, n_lags);
    kb += 2;
  }
  if (kb < job.n_chunks) irp_lags<1, false>(xs, yl + 64 * kb, yz, e0, e1, nv, part, lane + 64 * kb, n_lags);
}

// ---- pass 2: one wave per (pair x source)
__global__ __launch_bounds__(64) void k_irp_columns(IrpJob job) {
  const int lane = threadIdx.x;
  const int64_t line = blockIdx.x, L = job.ir_len;
  const IrpLine ln = irp_line(job, line);
  const int n_lags = job.n_lags, none = 0x7fffffff;
  const int64_t S = 2 * (int64_t)n_lags + 4;
  const double nan = __builtin_nan("");
  double *o = job.out + line * IRP_COLS;
  double *xc = job.xcorr ? job.xcorr + line * 2 * n_lags : nullptr;
  if (ln.state != IRP_OK) {                    // (uniform)
    if (xc)
      for (int i = lane; i < 2 * n_lags; i += 64) xc[i] = nan;
    if (lane == 0) {
      o[0] = ln.state == IRP_BAD ? ln.bad : ln.state == IRP_SILENT ? 0.0 : nan;
      for (int i = 1; i < IRP_COLS; ++i) o[i] = nan;
    }
    return;
  }
  const double *part = job.partials + line * job.n_tiles * S;
  double best[3] = {-1.0, -1.0, -1.0}, at[3] = {nan, nan, nan};     // the largest |r_W|, r_W there, and where: E, Lw, A
  int32_t arg[3] = {none, none, none};
  for (int idx = lane; idx < n_lags; idx += 64) {                   // ascending j inside a lane
    double r[3] = {0.0, 0.0, 0.0};
    for (int64_t k = 0; k < job.n_tiles; ++k) {
      r[0] += part[k * S + idx];
      r[1] += part[k * S + n_lags + idx];
    }
    r[2] = r[0] + r[1];
    if (xc) {
      xc[idx] = r[0];
      xc[n_lags + idx] = r[1];
    }
#pragma unroll
    for (int w = 0; w < 3; ++w) {
      if (fabs(r[w]) > best[w]) {              // strictly: the first of equal maxima stays
        best[w] = fabs(r[w]);
        at[w] = r[w];
        arg[w] = idx - job.max_lag;
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int w = 0; w < 3; ++w) {
      const double b2 = __shfl_down(best[w], off, 64), r2 = __shfl_down(at[w], off, 64);
      const int32_t j2 = __shfl_down(arg[w], off, 64);
      if (b2 > best[w] || (b2 == best[w] && j2 < arg[w])) {
        best[w] = b2;
        at[w] = r2;
        arg[w] = j2;
      }
    }
  }
  double en[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t k = 0; k < job.n_tiles; ++k) {
#pragma unroll
    for (int i = 0; i < 4; ++i) en[i] += part[k * S + 2 * n_lags + i];
  }
  if (lane != 0) return;
  const double exx[3] = {en[0], en[2], en[0] + en[2]}, eyy[3] = {en[1], en[3], en[1] + en[3]};
  const int64_t count[3] = {ln.e_hi - ln.e_lo, L - ln.e_hi, L - ln.e_lo};
  o[0] = 0.0;
  o[1] = isfinite(ln.t0) ? ln.t0 : nan;        // an infinity can only come from a table al_ir_metrics did not write
#pragma unroll
  for (int w = 0; w < 3; ++w) {
    const double den = exx[w] * eyy[w];
    const bool peak = count[w] > 0 && den != 0.0 && arg[w] != none;
    o[2 + 5 * w] = peak ? at[w] / sqrt(den) : nan;
    o[3 + 5 * w] = peak ? (double)arg[w] : nan;
    o[4 + 5 * w] = 10.0 * log10(exx[w] / eyy[w]);
    o[5 + 5 * w] = exx[w];
    o[6 + 5 * w] = eyy[w];
  }
}

inline void launch_ir_pair_metrics(const IrpJob &job, hipStream_t stream) {
  const int64_t lines = (int64_t)job.n_pairs * job.n_sources;
  const dim3 grid((unsigned)(lines * job.n_tiles)), block(64);
  if (job.max_lag <= 64)
    hipLaunchKernelGGL(k_irp_tiles<64>, grid, block, 0, stream, job);
  else if (job.max_lag <= 256)
    hipLaunchKernelGGL(k_irp_tiles<256>, grid, block, 0, stream, job);
  else
    hipLaunchKernelGGL(k_irp_tiles<1024>, grid, block, 0, stream, job);
  hipLaunchKernelGGL(k_irp_columns, dim3((unsigned)lines), block, 0, stream, job);
}

}  // namespace al
