// Shoebox room impulse responses with FREQUENCY-DEPENDENT WALLS in B <= 8 bands (al_ism_shoebox_bands; DESIGN.md "Shoebox IRs:
// frequency-dependent walls").  Every band b has its own column beta[:, b] of six reflection coefficients and its own zero-phase
// FIR phi_b of 2 half + 1 taps (shoebox.band_filters; sum_b phi_b = delta).  With y_b the image sum of al_ism.h under beta[:, b],
// evaluated at every integer s in [-half, y_end + half) (negative s included: the row boundary does not truncate a band sum),
//   y(t) = sum_b sum_{j = -half .. half} phi_b[j] y_b[t - j],   float64, b ascending, then j ascending,
// rounded to float32 once.  Two kernels share a row through a caller-provided float64 workspace [pair in pass][B][W],
// W = y_end + 2 half rounded up to ISM_TILE, whose index w holds sample s = w - half:
//   k_ism_bands<NB>  ism_gather (al_ism.h: its walk, its canonical order) over the shifted axis, one workgroup of ONE WAVE per
//     (pair, tile of W).  A list entry carries NB <= 4 BAND GAINS
//     exp(sum k ln beta_b) in place of the pattern gains (logarithms taken on the host; a wall of beta_b == 0 in the path makes gain b
//     exactly 0, which adds +-0 to that band's sum: the bits of leaving the image out; an image dead in every band of the group is
//     left out of the list), a lane forms the tap's shape once per (image, sample) and adds it into NB float64 accumulators.  B > 4
//     takes ceil(B / 4) launches over groups of bands: each band's sum keeps the canonical order, so grouping cannot change bits.
//     Every word of the workspace rows of the pass is written (zeros where no image reaches), none is read.  The kernel constructs
//     its variant and calls ism_workspace_rows, the body it shares with k_ism_sphere (al_ism_sphere.h).
//   k_ism_band_combine  one workgroup of ONE WAVE per (pair, output tile of ISM_TILE samples), as every kernel of al_ism.h.  Band
//     rows and phi_b go through LDS one band at a time, ISM_BAND_CHUNK taps at a time (2 ISM_BAND_CHUNK - 1 row samples serve a
//     chunk: 6 KB of LDS whatever `half` is); a lane keeps ONE float64 accumulator for each of its ISM_PER_LANE outputs
//     (t_lo + lane + 64 s) and adds the products in the stated order; one float32 store per sample, pads +0.  With one wave no
//     wave can be out of step with another: the __syncthreads() order LDS traffic only and there is no barrier instruction.
// THE DIFFUSE TAIL WITH BANDS (al_ism_shoebox_bands_tail).  ln_env is a table (B, n_knots): band b decays under its own knots.  With
// g(s) the row's draws of al_ism.h (zero outside [0, ir_len)), psi_k[j] = sum_b exp(ln_env[b][k]) phi_b[j], k = t / 256, p = (t % 256) / 256,
//   n(t) = (1 - p) sum_j psi_k[j] g(t - j) + p sum_j psi_{k+1}[j] g(t - j)      (p == 0 reads knot k alone),
//   h = float32(w_e y(t) + w_l n(t)) with the fade weights of al_ism.h; where w_l == 0 no noise term is formed.
// The band sums end at y_end = min(ir_len, M + F) and a row is shared as in al_ism.h:
//   k_ism_band_combine<true>  the tiles below SPLIT.  A tile with a sample past M stages the draws beside the band rows and runs a
//     second FIR per band over them, n(t) = sum_b ((1 - p) e_b[k] + p e_b[k + 1]) sum_j phi_b[j] g(t - j): the same number with the
//     two sums exchanged (the bound carries the difference), so no psi is formed for at most F + 256 samples of a row.
//   k_ism_band_tail<HCAP>  every sample at or past SPLIT, pad included.  One workgroup of ONE WAVE takes ISM_BT_SPAN = 1024 samples
//     of a row, four knot intervals one after the other.  It holds in LDS the draws of its span +- half as float32 and
//     (psi_k, psi_{k+1}) of the interval at hand, interleaved in pairs of 16 bytes and formed in-kernel from the knot tables and phi (b
//     ascending; a knot of -inf gives e_b = 0); from one interval to the next psi_{k+1} becomes psi_k and one psi is formed.  A lane
//     owns FOUR consecutive outputs: per tap it reads one pair of psi (a broadcast) and ONE new draw, the other three slide
//     through registers, and does eight float64 multiply-adds into eight accumulators; one 16-byte store per lane and interval.
//     Accumulation is float64: the draws are float32 values and psi spans the decay of a whole row, so float32 sums would put
//     about 1025 * 2^-24 of sum |psi| |g| into every sample, and the FIR is bound by multiply-add issue either way.  HCAP (256,
//     512, 1024: the smallest that holds `half`) sizes the LDS arrays; ISM_BAND_TAIL_MAX_HALF = 1024 is the cap with a tail.
// The entry walks the pairs in PASSES of workspace_bytes / bytes_per_pair pairs, gather then combine, in order on the one stream: the
// workspace is reused in stream order, nothing is allocated and nothing synchronises.  A row's bits do not depend on the pass it is
// generated in: both kernels index the workspace by the pair's place in its pass only to find their own rows.  The pass loop
// (ism_rows_passes), the checks of rows, half, workspace and tail (ism_rows_range, ism_rows_prepare) and the workspace's size
// (ism_rows_workspace_bytes) serve the sphere call too; the three band entries go through one ism_bands_prepare (mix < 0: no tail).
// SOURCE PATTERNS AND AIR WITH BANDS (al_ism_shoebox_bands_src; al_ism.h "THE SOURCE SIDE").  k_ism_bands<NB, true> takes IsmBandsSrc<NB>:
// the source gain gs goes into the rigid-wall amplitude 1 / (4 pi d), and band b's gain becomes exp(sum k ln beta_b - m_b d) with
// its own air coefficient m_b (IsmBandJob::air).  With a tail the knot tables are (N, B, n_knots): a table per (source, band),
// found through IsmTail::env_src_stride by k_ism_band_combine<true> and k_ism_band_tail.
#pragma once
#include "al_ism.h"

namespace al {

constexpr int ISM_MAX_BANDS = 8;
constexpr int ISM_BAND_GROUP = 4;        // bands per launch of k_ism_bands (the accumulators of k_ism_shoebox_dir<4>)
constexpr int ISM_BAND_MAX_HALF = 4096;  // the cap on `half`: 8193 taps per band
constexpr int ISM_BAND_CHUNK = 256;      // taps staged per step of k_ism_band_combine
constexpr int ISM_BAND_TAIL_MAX_HALF = 1024;   // the cap on `half` with a tail (the LDS of k_ism_band_tail)
constexpr int ISM_BT_PER_LANE = 4;             // consecutive outputs per lane of k_ism_band_tail: one knot interval per wave
constexpr int ISM_BT_INTERVALS = 4;            // knot intervals per workgroup
constexpr int ISM_BT_SPAN = ISM_BT_INTERVALS * ISM_TILE;
static_assert(ISM_THREADS * ISM_BT_PER_LANE == ISM_TILE, "k_ism_band_tail: a wave covers one knot interval");
static_assert(ISM_BAND_CHUNK == ISM_TILE, "k_ism_band_combine: the staged row segment spans a tile of outputs and a chunk of taps");

struct IsmBandJob {
  IsmJob base;                       // ln_beta / beta_zero unused: the per-band tables below
  double ln_beta[ISM_MAX_BANDS][6];  // 0 where beta == 0
  int32_t beta_zero[ISM_MAX_BANDS][6];
  const double *filters;             // (n_bands, 2 half + 1), device
  double *workspace;                 // [pair in pass][n_bands][W], device
  int32_t n_bands, half, y_end;      // y_end: the image sum is formed below it (ir_len, or min(ir_len, M + F) with a tail)
  int32_t band_tail_blocks;          // workgroups of k_ism_band_tail per row
  int32_t W, n_ws_tiles;             // W = n_ws_tiles * ISM_TILE
  int32_t n_out_tiles;               // ceil(pitch / ISM_TILE)
  int32_t band0;                     // first band of this launch of k_ism_bands
  int64_t pair0;                     // first pair of the pass
  int64_t pairs_per_pass;
  double air[ISM_MAX_BANDS];         // m_b of al_ism_shoebox_bands_src, Np/m (read by k_ism_bands<NB, true> only)
};

struct alignas(16) IsmPsi {
  double x, y;   // psi_k[j], psi_{k+1}[j]: one 16-byte LDS read per tap
};

// the band variant: the gains of the NB bands [band0, band0 + NB) beside the image between rigid walls
template <int NB>
struct IsmBands {
  static constexpr int NG = NB, LIST = ISM_DIR_LIST;
  using Entry = IsmDirEntry<NB>;
  const IsmBandJob &bj;
  // the bands of the group in which image q of the axis is alive (no wall of beta_b == 0 hit)
  __device__ __forceinline__ unsigned alive(int axis, int q) const {
    unsigned mask = 0;
#pragma unroll
    for (int k = 0; k < NB; ++k)
      if (ism_alive(q, bj.beta_zero[bj.band0 + k] + 2 * axis)) mask |= 1u << k;
    return mask;
  }
  __device__ __forceinline__ void fill(Entry &e, const IsmImage &im) const {
#pragma unroll
    for (int k = 0; k < NB; ++k) {   // prod beta_b^k, the logarithms summed as al_ism.h sums them: (x + y) + z
      const double *lb = bj.ln_beta[bj.band0 + k];
      const double ln_xy = ism_log_gain(im.qx, lb) + ism_log_gain(im.qy, lb + 2), ln_z = ism_log_gain(im.qz, lb + 4);
      e.gain[k] = ((im.alive >> k) & 1u) ? exp(ln_xy + ln_z) : 0.0;
    }
    ism_fill_shape(e, im, 1.0 / (4.0 * M_PI * im.d));   // a, g of the image between rigid walls
  }
};

// IsmBands with a source pattern and an air coefficient per band
template <int NB>
struct IsmBandsSrc : IsmBands<NB> {
  using Entry = IsmDirEntry<NB>;
  IsmSource src;
  __device__ __forceinline__ void fill(Entry &e, const IsmImage &im) const {
    const IsmBandJob &bj = this->bj;
    e.a = src.gain(im);   // parked in the list and read back below: not live while the NB exp are evaluated
    ism_park();
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      const double *lb = bj.ln_beta[bj.band0 + k];
      const double ln_xy = ism_log_gain(im.qx, lb) + ism_log_gain(im.qy, lb + 2), ln_z = ism_log_gain(im.qz, lb + 4);
      e.gain[k] = ((im.alive >> k) & 1u) ? exp((ln_xy + ln_z) - bj.air[bj.band0 + k] * im.d) : 0.0;
    }
    ism_fill_shape(e, im, 1.0 / (4.0 * M_PI * im.d) * e.a);
  }
};

// the pair of a workgroup of a pass whose grid has `tiles` workgroups per pair: its place in the pass, its source n and its row cap
__device__ __forceinline__ int64_t ism_pass_pair(const IsmBandJob &bj, int tiles, int &n, int &cap) {
  const int64_t local = blockIdx.x / (unsigned)tiles, pair = bj.pair0 + local;   // c * N + n
  n = (int)(pair % bj.base.n_sources), cap = (int)(pair / bj.base.n_sources);
  return local;
}

// THE WORKSPACE ROWS of one (pair, tile of W), what k_ism_bands and k_ism_sphere (al_ism_sphere.h) share: the V::NG rows
// [band0, band0 + V::NG) of the pair are the gather of source n at receiver pos of `job` under the variant v over the shifted axis,
// zeros in a tile that no tap reaches
template <class V>
__device__ __forceinline__ void ism_workspace_rows(const IsmBandJob &bj, const IsmJob &job, const V &v, int n, int pos) {
  constexpr int NB = V::NG;
  __shared__ typename V::Entry list[V::LIST];
  __shared__ double win_c[ISM_TAPS], win_s[ISM_TAPS];
  __shared__ int wave_total[2];
  const int tid = threadIdx.x;
  const int tile = (int)(blockIdx.x % (unsigned)bj.n_ws_tiles);
  const int64_t local = blockIdx.x / (unsigned)bj.n_ws_tiles;
  // the tile in workspace words w and in samples s = w - half
  const int w_lo = tile * ISM_TILE, w = w_lo + tid;
  const int s_lo = w_lo - bj.half;
  const int s_end = bj.y_end + bj.half;                // the row sums are formed for s < s_end
  const int t_hi = min(s_lo + ISM_TILE, s_end) - 1;
  double *rows = bj.workspace + (local * bj.n_bands + bj.band0) * (int64_t)bj.W;   // row band0 of the pair; row k is k * W on
  if (t_hi < s_lo || t_hi < -ISM_HALF) {   // a tile past s_end, or so far below sample 0 that no tap reaches it (tau > 0)
    for (int k = 0; k < NB; ++k)
      for (int s = 0; s < ISM_PER_LANE; ++s) rows[(int64_t)k * bj.W + w + s * ISM_THREADS] = 0.0;
    return;
  }
  double acc[ISM_PER_LANE][NB] = {};
  ism_gather(job, v, n, pos, s_lo, t_hi, s_end, list, win_c, win_s, wave_total, acc);
#pragma unroll
  for (int s = 0; s < ISM_PER_LANE; ++s)   // w + s * ISM_THREADS < W: the tile lies inside the row
#pragma unroll
    for (int k = 0; k < NB; ++k) rows[(int64_t)k * bj.W + w + s * ISM_THREADS] = acc[s][k];
}

template <int NB, bool SRC = false>
__global__ __launch_bounds__(ISM_THREADS) void k_ism_bands(IsmBandJob bj) {
  int n, cap;
  ism_pass_pair(bj, bj.n_ws_tiles, n, cap);
  if constexpr (SRC)
    ism_workspace_rows(bj, bj.base, IsmBandsSrc<NB>{{bj}, ism_source(bj.base, n)}, n, cap);
  else
    ism_workspace_rows(bj, bj.base, IsmBands<NB>{bj}, n, cap);
}

// draw s of row (cap, n); zero outside [0, ir_len)
__device__ __forceinline__ float ism_band_draw(const IsmJob &job, int s, int n, int cap) {
  return s < 0 || s >= job.ir_len ? 0.f : ism_tail_normal(job.tail, s, n, cap);
}

// out[t] = float32(sum_b sum_j phi_b[j] y_b[t - j]); grid: n_out_tiles workgroups of ONE WAVE per pair of the pass, a lane owning
// outputs t_lo + lane + 64 s, s < ISM_PER_LANE (so the lanes of a wave read consecutive LDS words), each with an accumulator of its
// own.  TAIL: the fade and the noise term for the samples past M (the tiles below the split).  (One wave: the __syncthreads() below
// order LDS traffic only, hipcc emits no barrier instruction for them.)
template <bool TAIL>
__global__ __launch_bounds__(ISM_THREADS) void k_ism_band_combine(IsmBandJob bj) {
  __shared__ double seg[2 * ISM_BAND_CHUNK], tap[ISM_BAND_CHUNK];
  __shared__ float gseg[TAIL ? 2 * ISM_BAND_CHUNK : 1];
  const IsmJob &job = bj.base;
  const int tid = threadIdx.x;
  const int tile = (int)(blockIdx.x % (unsigned)bj.n_out_tiles);
  const int64_t local = blockIdx.x / (unsigned)bj.n_out_tiles, pair = bj.pair0 + local;
  const int n = (int)(pair % job.n_sources), cap = (int)(pair / job.n_sources);
  const int t_lo = tile * ISM_TILE, t = t_lo + tid;   // the lane's first output
  float *row = job.out + pair * (int64_t)job.pitch;
  if (t_lo >= job.ir_len) {   // a tile of pad samples only
    for (int s = 0; s < ISM_PER_LANE; ++s)
      if (t + s * ISM_THREADS < job.pitch) row[t + s * ISM_THREADS] = 0.f;
    return;
  }
  // does a sample of this tile carry noise?  (uniform over the workgroup)
  const bool noisy = TAIL && (int64_t)t_lo + ISM_TILE - 1 > job.tail.mix;
  const int n_taps = 2 * bj.half + 1;
  double acc[ISM_PER_LANE] = {}, noise[ISM_PER_LANE] = {};
  for (int b = 0; b < bj.n_bands; ++b) {
    const double *y = bj.workspace + (local * bj.n_bands + b) * (int64_t)bj.W;
    const double *phi = bj.filters + (int64_t)b * n_taps;
    double acc_g[ISM_PER_LANE] = {};   // sum_j phi_b[j] g(t - j)
    for (int c0 = 0; c0 < n_taps; c0 += ISM_BAND_CHUNK) {
      // taps j = -half + c0 + i, i < ISM_BAND_CHUNK: output t_lo + o reads word t - j + half = first + (ISM_BAND_CHUNK - 1) + o - i
      const int first = t_lo + 2 * bj.half - c0 - (ISM_BAND_CHUNK - 1);
      __syncthreads();   // the reads of the chunk before are over
      for (int k = tid; k < 2 * ISM_BAND_CHUNK - 1; k += ISM_THREADS) {
        const int idx = first + k;   // below 0 only under taps past the last one, at or past W only under outputs past y_end
        seg[k] = idx >= 0 && idx < bj.W ? y[idx] : 0.0;
        if constexpr (TAIL)
          if (noisy) gseg[k] = ism_band_draw(job, idx - bj.half, n, cap);   // word idx holds sample idx - half
      }
      for (int k = tid; k < ISM_BAND_CHUNK; k += ISM_THREADS) tap[k] = c0 + k < n_taps ? phi[c0 + k] : 0.0;
      __syncthreads();
      const int m = min(ISM_BAND_CHUNK, n_taps - c0);
      const double *mine = seg + (ISM_BAND_CHUNK - 1) + tid;
      for (int i = 0; i < m; ++i) {
        const double w = tap[i];
#pragma unroll
        for (int s = 0; s < ISM_PER_LANE; ++s) acc[s] += w * mine[s * ISM_THREADS - i];
      }
      if constexpr (TAIL) {
        if (noisy) {
          const float *mine_g = gseg + (ISM_BAND_CHUNK - 1) + tid;
          for (int i = 0; i < m; ++i) {
            const double w = tap[i];
#pragma unroll
            for (int s = 0; s < ISM_PER_LANE; ++s) acc_g[s] += w * (double)mine_g[s * ISM_THREADS - i];
          }
        }
      }
    }
    if constexpr (TAIL) {
      if (noisy) {
        const double *ln_env = ism_tail_table(job.tail, b, n);   // band b's table, the source's with al_ism_shoebox_bands_src
#pragma unroll
        for (int s = 0; s < ISM_PER_LANE; ++s) {
          const int ts = t + s * ISM_THREADS;
          if (ts > job.tail.mix && ts < job.ir_len) {   // the band's envelope at ts, interpolated in amplitude
            const int k = ts / ISM_TILE, r = ts % ISM_TILE;
            const double p = (double)r / (double)ISM_TILE;
            const double e = r == 0 ? exp(ln_env[k]) : (1.0 - p) * exp(ln_env[k]) + p * exp(ln_env[k + 1]);
            noise[s] += e * acc_g[s];
          }
        }
      }
    }
  }
#pragma unroll
  for (int s = 0; s < ISM_PER_LANE; ++s) {
    const int ts = t + s * ISM_THREADS;
    if (ts >= job.pitch) continue;
    double v = acc[s];
    if constexpr (TAIL) {
      if (ts > job.tail.mix && ts < job.ir_len) {   // at or below M: w_e = 1, w_l = 0, the image part as it is
        const double x = ((double)ts - (double)job.tail.mix) / (double)job.tail.fade;
        if (x < 1.0) {
          double w_e, w_l;
          sincospi(0.5 * x, &w_l, &w_e);
          v = w_e * acc[s] + w_l * noise[s];
        } else {
          v = noise[s];
        }
      }
    }
    row[ts] = ts < job.ir_len ? (float)v : 0.f;
  }
}

// the samples [split, pitch) of every row: the draws through psi_k, psi_{k+1}; grid: band_tail_blocks workgroups of one wave per pair
template <int HCAP>
__global__ __launch_bounds__(ISM_THREADS) void k_ism_band_tail(IsmBandJob bj) {
  __shared__ IsmPsi psi[2 * HCAP + 1];             // (psi_k[j], psi_{k+1}[j]) at j + half
  __shared__ float g[ISM_BT_SPAN + 2 * HCAP];      // draw span_lo - half + i at i
  const IsmJob &job = bj.base;
  const int lane = threadIdx.x;
  const int block = (int)(blockIdx.x % (unsigned)bj.band_tail_blocks);
  const int64_t pair = blockIdx.x / (unsigned)bj.band_tail_blocks;   // every pair in one launch: no workspace is touched
  const int n = (int)(pair % job.n_sources), cap = (int)(pair / job.n_sources);
  float *row = job.out + pair * (int64_t)job.pitch;
  const int half = bj.half, n_taps = 2 * half + 1;
  const int64_t span_lo = (int64_t)job.tail.split + (int64_t)block * ISM_BT_SPAN;   // < pitch <= 2^31 - 1
  // the draws of the span +- half, a Philox block of four at a time (span_lo - half may not be a multiple of 4: block by block)
  const int g_len = ISM_BT_SPAN + 2 * half, s_first = (int)span_lo - half;
  const int q_first = s_first >> 2;   // arithmetic shift: floor for negative samples too
  for (int q = q_first + lane; 4 * q < s_first + g_len; q += ISM_THREADS) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q >= 0 && 4 * (int64_t)q < job.ir_len) v = ism_tail_normal4(job.tail, q, n, cap);
    const float vs[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int s = 4 * q + i, at = s - s_first;
      if (at >= 0 && at < g_len) g[at] = s >= 0 && s < job.ir_len ? vs[i] : 0.f;
    }
  }
  // psi of one knot into half `which` of the double2 table
  const double *ln_env = ism_tail_table(job.tail, 0, n);   // band 0's table, the source's with al_ism_shoebox_bands_src
  auto form = [&](int knot, int which) {
    double e[ISM_MAX_BANDS];   // unrolled to the full count: registers, no indexed array
#pragma unroll
    for (int b = 0; b < ISM_MAX_BANDS; ++b) e[b] = b < bj.n_bands ? exp(ln_env[(int64_t)b * job.tail.env_stride + knot]) : 0.0;
    for (int m = lane; m < n_taps; m += ISM_THREADS) {
      double v = 0.0;
#pragma unroll
      for (int b = 0; b < ISM_MAX_BANDS; ++b)
        if (b < bj.n_bands) v += e[b] * bj.filters[(int64_t)b * n_taps + m];
      if (which) psi[m].y = v; else psi[m].x = v;
    }
  };
  for (int iv = 0; iv < ISM_BT_INTERVALS; ++iv) {
    const int64_t t_base64 = span_lo + (int64_t)iv * ISM_TILE;
    if (t_base64 >= job.pitch) break;   // uniform over the wave
    const int t_base = (int)t_base64, t0 = t_base + ISM_BT_PER_LANE * lane;
    if (t_base >= job.ir_len) {   // pad samples only
      if (t0 < job.pitch) *reinterpret_cast<float4 *>(row + t0) = make_float4(0.f, 0.f, 0.f, 0.f);
      continue;
    }
    const int knot = t_base / ISM_TILE;   // knot + 1 <= (ir_len - 1) / 256 + 1: inside the table
    __syncthreads();   // one wave: orders the LDS traffic (the draws, the table's readers of the interval before)
    if (iv == 0) {
      form(knot, 0);
    } else {
      for (int m = lane; m < n_taps; m += ISM_THREADS) psi[m].x = psi[m].y;   // psi_{k+1} of the interval before is this one's psi_k
    }
    form(knot + 1, 1);
    __syncthreads();
    // output t0 + q reads draw t0 + q - j at g[at + q - m], m = j + half
    const int at = t0 - (int)span_lo + 2 * half;
    double a[ISM_BT_PER_LANE] = {}, c[ISM_BT_PER_LANE] = {};
    // the window slides as float64: one conversion per tap, of the draw that enters
    double d0 = (double)g[at], d1 = (double)g[at + 1], d2 = (double)g[at + 2], d3 = (double)g[at + 3];
#pragma unroll 4
    for (int m = 0; m < n_taps; ++m) {
      const IsmPsi ps = psi[m];
      a[0] += ps.x * d0, a[1] += ps.x * d1, a[2] += ps.x * d2, a[3] += ps.x * d3;
      c[0] += ps.y * d0, c[1] += ps.y * d1, c[2] += ps.y * d2, c[3] += ps.y * d3;
      d3 = d2, d2 = d1, d1 = d0;
      d0 = (double)g[max(at - m - 1, 0)];   // at - m - 1 >= 0 but behind the last tap, whose draw is not used
    }
    if (t0 < job.pitch) {   // pitch is a multiple of 4: a quad is inside the row or outside it
      float vs[ISM_BT_PER_LANE];
#pragma unroll
      for (int q = 0; q < ISM_BT_PER_LANE; ++q) {
        const int r = ISM_BT_PER_LANE * lane + q;
        const double p = (double)r / (double)ISM_TILE;
        const double v = r == 0 ? a[q] : (1.0 - p) * a[q] + p * c[q];
        vs[q] = t0 + q < job.ir_len ? (float)v : 0.f;
      }
      *reinterpret_cast<float4 *>(row + t0) = make_float4(vs[0], vs[1], vs[2], vs[3]);
    }
  }
}

// THE LAYOUT of a job (n_bands, half and base.n_tiles set) whose band sums end at y_end, in a workspace of workspace_bytes: W of a row
// (y_end + 2 half rounded up to the tile), the two tile counts, and the pairs per pass: what the workspace holds, and no grid above
// 2^31 - 1 workgroups.  Returns the bytes a pair takes; a workspace below that holds no pair (pairs_per_pass == 0)
inline int64_t ism_bands_layout(IsmBandJob *bj, int32_t y_end, int64_t workspace_bytes) {
  const int64_t W = ((int64_t)y_end + 2 * (int64_t)bj->half + ISM_TILE - 1) / ISM_TILE * ISM_TILE;
  const int64_t per_pair = (int64_t)bj->n_bands * W * (int64_t)sizeof(double);
  bj->y_end = y_end;
  bj->W = (int32_t)W;
  bj->n_ws_tiles = (int32_t)(W / ISM_TILE);
  bj->n_out_tiles = bj->base.n_tiles;   // with a tail: the tiles below the split
  const int64_t most_tiles = bj->n_ws_tiles > bj->n_out_tiles ? bj->n_ws_tiles : bj->n_out_tiles;
  int64_t per_pass = workspace_bytes < per_pair ? 0 : workspace_bytes / per_pair;
  if (per_pass > 0x7fffffff / most_tiles) per_pass = 0x7fffffff / most_tiles;
  bj->pairs_per_pass = per_pass;
  return per_pair;
}

// THE WORKSPACE FAMILIES (bands here, Legendre orders in al_ism_sphere.h) share their row checks, their workspace and their passes.
// `entry` names the C entry in every refusal, `what` its row count ("n_bands", "n_orders")
inline int ism_rows_range(const char *entry, const char *what, int32_t n_rows, int32_t max_rows, int32_t half, int32_t max_half) {
  char why[64];
  if (n_rows < 1 || n_rows > max_rows)
    snprintf(why, sizeof(why), "%s must be in 1 .. %d", what, max_rows);
  else if (half < 1 || half > max_half)
    snprintf(why, sizeof(why), "half must be in 1 .. %d", max_half);
  else
    return AL_OK;
  return fail_arg(entry, why);
}

// al_ism_shoebox_bands_workspace_bytes and al_ism_shoebox_sphere_workspace_bytes: bytes per pair, or AL_E_BADARG.  mix < 0: no tail
// (y_end = ir_len)
inline int64_t ism_rows_workspace_bytes(const char *entry, const char *what, int32_t n_rows, int32_t max_rows, int32_t half, int32_t max_half,
                                        int32_t ir_len, int64_t mix, int64_t fade) {
  if (int rc = ism_rows_range(entry, what, n_rows, max_rows, half, max_half)) return rc;
  if (ir_len < 1) return fail_arg(entry, "ir_len must be >= 1");
  if (mix >= 0 && fade < 1) return fail_arg(entry, "fade must be >= 1");
  IsmBandJob bj;
  bj.n_bands = n_rows;
  bj.half = half;
  bj.base.n_tiles = 1;
  return ism_bands_layout(&bj, mix < 0 ? ir_len : ism_tail_y_end(mix, fade, ir_len), 0);
}

// what both families check once ism_prepare has filled bj->base and n_bands and half are set (ism_rows_range): the mirror cells the
// row sums reach, the workspace, with mix >= 0 the tail (ism_tail_prepare, the pitch and the grid of k_ism_band_tail), and the
// workspace's size against the layout of a row that ends at y_end
inline int ism_rows_prepare(const char *entry, const double *L, void *workspace, int64_t workspace_bytes, int64_t mix, int64_t fade,
                            uint64_t seed, int64_t source_id0, int64_t capsule_id0, const double *ln_env, int32_t n_knots, IsmBandJob *bj) {
  IsmJob &base = bj->base;
  for (int i = 0; i < 3; ++i)   // the row sums reach `half` past the row
    if (!(base.c * ((double)base.ir_len + (double)bj->half + 42.0) / base.fs / L[i] + 2.0 <= ISM_MAX_HALF_WIDTH))
      return fail_arg(entry, "c (ir_len + half + 42) / fs spans more than 2^20 mirror cells of the room");
  if (!workspace || ((uintptr_t)workspace & 15) != 0) return fail_arg(entry, "workspace must be 16-byte aligned and not null");
  bj->workspace = (double *)workspace;
  bj->band0 = 0;
  bj->pair0 = 0;
  bj->band_tail_blocks = 0;
  int32_t y_end = base.ir_len;
  if (mix >= 0) {   // a row with a tail needs y_end = min(ir_len, M + F) samples of every row sum only
    if (int rc = ism_tail_prepare(mix, fade, seed, source_id0, capsule_id0, ln_env, n_knots, &base)) return rc;
    if (base.pitch > 0x7fffffff - 2 * (ISM_BT_SPAN + ISM_BAND_TAIL_MAX_HALF))   // k_ism_band_tail counts span + half past the row in int32
      return fail_arg(entry, "pitch must be at most 2^31 - 4097 with a tail");
    y_end = base.tail.y_end;
    bj->band_tail_blocks = base.tail.split < base.pitch ? (base.pitch - base.tail.split + ISM_BT_SPAN - 1) / ISM_BT_SPAN : 0;
    if ((int64_t)bj->band_tail_blocks * base.n_sources * base.n_capsules > 0x7fffffff)
      return fail_arg(entry, "more than 2^31 - 1 workgroups (spans of 1024 samples x pairs): split the call");
  }
  if (workspace_bytes < ism_bands_layout(bj, y_end, workspace_bytes)) {
    char why[96];
    snprintf(why, sizeof(why), "workspace smaller than %s_workspace_bytes (one pair)", entry);
    return fail_arg(entry, why);
  }
  return AL_OK;
}

// the arguments of al_ism_shoebox_bands, _bands_tail and _bands_src as the kernels' job: 0 with *bj filled, or the error of the first
// bad argument.  mix < 0: no tail, and the tail's arguments are not looked at; else ln_env is (B, n_knots)
inline int ism_bands_prepare(const double *sources, int32_t n_sources, const double *capsules, int32_t n_capsules, const double *L,
                             const double *beta, int32_t n_bands, const double *filters, int32_t half, double c, double fs,
                             int32_t max_order, int32_t ir_len, int32_t pitch, int64_t mix, int64_t fade, uint64_t seed, int64_t source_id0,
                             int64_t capsule_id0, const double *ln_env, int32_t n_knots, void *workspace, int64_t workspace_bytes, float *out,
                             IsmBandJob *bj) {
  if (int rc = ism_rows_range("al_ism_shoebox_bands", "n_bands", n_bands, ISM_MAX_BANDS, half, ISM_BAND_MAX_HALF)) return rc;
  if (mix >= 0 && half > ISM_BAND_TAIL_MAX_HALF) return fail(AL_E_BADARG, "al_ism_shoebox_bands_tail: half must be in 1 .. 1024 with a tail");
  if (!beta) return fail(AL_E_BADARG, "al_ism_shoebox: null pointer");
  if (!filters) return fail(AL_E_BADARG, "al_ism_shoebox_bands: null filter table");
  double column[6];
  for (int b = 0; b < n_bands; ++b) {   // ism_prepare refuses what al_ism_shoebox refuses, band by band
    for (int i = 0; i < 6; ++i) column[i] = beta[i * n_bands + b];
    if (int rc = ism_prepare(sources, n_sources, capsules, n_capsules, L, column, c, fs, max_order, ir_len, pitch, out, &bj->base)) return rc;
    for (int i = 0; i < 6; ++i) {
      bj->ln_beta[b][i] = bj->base.ln_beta[i];
      bj->beta_zero[b][i] = bj->base.beta_zero[i];
    }
  }
  for (int b = n_bands; b < ISM_MAX_BANDS; ++b)
    for (int i = 0; i < 6; ++i) bj->ln_beta[b][i] = 0.0, bj->beta_zero[b][i] = 0;
  bj->filters = filters;
  bj->n_bands = n_bands;
  bj->half = half;
  for (int b = 0; b < ISM_MAX_BANDS; ++b) bj->air[b] = 0.0;
  if (int rc = ism_rows_prepare("al_ism_shoebox_bands", L, workspace, workspace_bytes, mix, fade, seed, source_id0, capsule_id0, ln_env, n_knots, bj))
    return rc;
  if (mix >= 0) bj->base.tail.env_stride = (uint32_t)n_knots;   // from band b to band b + 1
  return AL_OK;
}

// al_ism_shoebox_bands_src's further arguments into a job ism_bands_prepare has filled: the source patterns, the air coefficient of
// every band, a knot table per (source, band)
inline int ism_bands_source_prepare(const double *source_patterns, const double *air, bool with_tail, IsmBandJob *bj) {
  if (!air) return fail(AL_E_BADARG, "al_ism_shoebox_bands_src: null air table");
  for (int b = 0; b < bj->n_bands; ++b) {
    if (int rc = ism_source_prepare(source_patterns, air[b], &bj->base)) return rc;
    bj->air[b] = air[b];
  }
  bj->base.air = 0.0;   // the bands carry their own
  if (with_tail) bj->base.tail.env_src_stride = bj->base.tail.env_stride * (uint32_t)bj->n_bands;   // (N, B, n_knots): at most 8 x 2^23 knots
  return AL_OK;
}

// THE PASS LOOP of both families: the pairs in passes of what the workspace holds, per pass the gathers over groups of at most
// ISM_BAND_GROUP rows and then the combine, in order on the one stream.  bj is the band job INSIDE the job the two callables hand their
// kernels: the loop sets its pair0 and band0.  gather(group size as an integral constant, grid), combine(grid)
template <class Gather, class Combine>
inline void ism_rows_passes(IsmBandJob &bj, Gather gather, Combine combine) {
  const int64_t pairs = (int64_t)bj.base.n_sources * bj.base.n_capsules;
  for (int64_t pair0 = 0; pair0 < pairs; pair0 += bj.pairs_per_pass) {
    const int64_t in_pass = pairs - pair0 < bj.pairs_per_pass ? pairs - pair0 : bj.pairs_per_pass;
    bj.pair0 = pair0;
    const dim3 grid((unsigned)(in_pass * bj.n_ws_tiles));
    for (int band0 = 0; band0 < bj.n_bands; band0 += ISM_BAND_GROUP) {
      bj.band0 = band0;
      switch (bj.n_bands - band0 < ISM_BAND_GROUP ? bj.n_bands - band0 : ISM_BAND_GROUP) {
        case 1: gather(std::integral_constant<int, 1>{}, grid); break;
        case 2: gather(std::integral_constant<int, 2>{}, grid); break;
        case 3: gather(std::integral_constant<int, 3>{}, grid); break;
        default: gather(std::integral_constant<int, 4>{}, grid); break;
      }
    }
    bj.band0 = 0;
    combine(dim3((unsigned)(in_pass * bj.n_out_tiles)));
  }
}

// the samples past the split of every row of a job with a tail
inline void launch_ism_band_tail(const IsmBandJob &job, hipStream_t stream) {
  if (job.band_tail_blocks > 0) {
    const dim3 grid((unsigned)((int64_t)job.band_tail_blocks * job.base.n_sources * job.base.n_capsules)), block(ISM_THREADS);
    if (job.half <= 256)
      hipLaunchKernelGGL(k_ism_band_tail<256>, grid, block, 0, stream, job);
    else if (job.half <= 512)
      hipLaunchKernelGGL(k_ism_band_tail<512>, grid, block, 0, stream, job);
    else
      hipLaunchKernelGGL(k_ism_band_tail<1024>, grid, block, 0, stream, job);
  }
}

// THE LAUNCH OF THE BAND ENTRIES: the passes, then with a tail the samples past the split.  src: k_ism_bands<NB, true>
// (al_ism_shoebox_bands_src takes it whatever its source table and air are)
template <bool TAIL, bool SRC>
inline void launch_ism_bands_passes(const IsmBandJob &job, hipStream_t stream) {
  IsmBandJob bj = job;
  const dim3 block(ISM_THREADS);
  ism_rows_passes(
      bj, [&](auto nb, dim3 grid) { hipLaunchKernelGGL((k_ism_bands<decltype(nb)::value, SRC>), grid, block, 0, stream, bj); },
      [&](dim3 grid) { hipLaunchKernelGGL(k_ism_band_combine<TAIL>, grid, block, 0, stream, bj); });
  if (TAIL) launch_ism_band_tail(job, stream);
}

inline void launch_ism_shoebox_bands(const IsmBandJob &job, bool with_tail, bool src, hipStream_t stream) {
  if (with_tail)
    src ? launch_ism_bands_passes<true, true>(job, stream) : launch_ism_bands_passes<true, false>(job, stream);
  else
    src ? launch_ism_bands_passes<false, true>(job, stream) : launch_ism_bands_passes<false, false>(job, stream);
}

}  // namespace al
