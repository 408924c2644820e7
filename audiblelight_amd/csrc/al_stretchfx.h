// Time-stretch FX (A14: SpeedUp, PitchShift; audiblelight/augmentation.py:1232-1347).  The reference calls pedalboard.time_stretch
// (Rubber Band, an un-vendored wheel): the effect is pinned by the definition in DESIGN.md "Time-stretch FX" (librosa 0.11's
// effects.time_stretch / phase_vocoder restated, plus a Kaiser-windowed sinc resampler) and NOT checked against a running pedalboard
// or librosa.  hop = n_fft / 4, w[t] = sin^2(pi t / n_fft), F = 1 + n / hop analysis frames, T output frames (t rate < F).
//
// One stretch, all on the caller's stream, no host synchronisation (launch_time_stretch):
//   k_pv_pack         z[f][t] = w[t] xpad[f hop + t] as complex float64 rows (x zero-padded by n_fft / 2 on both sides)
//   k_pv_pass64       D[f] = FFT(z[f]): Stockham radix-4 / 2 passes in FLOAT64 over all F rows at once (bins 0 .. n_fft / 2 are
//                     the rfft).  Why not big_fft: a float32 analysis puts an error of about 1e-7 |frame| / |D[f][k]| into every
//                     arg D, and the accumulator sums those over the frames like a random walk (they only cancel at rate 1), so
//                     the output error grew with the frame count (DESIGN.md "Time-stretch FX", "why the analysis is float64")
//   k_pv_phase_sums   per tile of PV_TILE output frames and per bin: the sum of the tile's phase increments, mod 2 pi
//   k_pv_phase_carry  per bin: the exclusive prefix sum of the tile sums from arg D[0][k]  (T / PV_TILE steps, not T)
//   k_pv_phase        per tile and bin: walks the tile from its carried phase, writes S[t][k] = mag e^{i acc} (float32) and its
//                     Hermitian mirror for the inverse transform
//   big_fft +1        fr[t] = n_fft irfft(S[t]), T rows in groups of MAX_GRID_ROWS as al_stft does (float32: its error does not
//                     accumulate)
//   k_pv_ola          gather: window, overlap-add of the <= 4 frames over a sample, 1 / n_fft, window-sum-square normalisation,
//                     trim by n_fft / 2, zero tail
// The phase scan is a two-pass block scan: the increments are computed twice (once for the tile sums, once for the walk) by the
// same device function on the same operands, so both passes see the same bits.  Bins are the fastest index everywhere: a wave
// reads and writes 64 consecutive bins of one frame.  atan2, sincos, the wrap and the accumulator are float64.  No kernel here
// has a barrier and no workgroup waits on another.
//
// k_resample_sinc   one thread per output sample: out[t] = sum_j y1[j] c sinc(c (p - j)) I0(beta sqrt(1 - ((p - j) / H)^2)) / I0(beta),
//                   p = t m / n in exact integer arithmetic, float64 per sample, I0 by its power series.
#pragma once
#include <float.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "al_bigfft.h"
#include "al_common.h"
#include "al_status.h"
#include "al_stft.h"

namespace al {

constexpr int PV_TILE = 32;        // output frames per tile of the phase scan
constexpr int PV_LANES = 64;       // bins per workgroup of the phase kernels (one wave)
constexpr int PV_MIN_FFT = 64, PV_MAX_FFT = 4096;
constexpr int64_t PV_MAX_FRAMES = (int64_t)1 << 30;   // F and T: a frame index times n_fft stays far inside int64, tiles inside a grid
constexpr double PV_PI = 3.14159265358979323846264338327950288;
constexpr double PV_TWO_PI = 6.283185307179586476925286766559;
constexpr double RS_BETA = 8.6, RS_ROLLOFF = 0.95, RS_ZEROS = 16.0;   // the resampler's Kaiser beta, c at n >= m, H c

// w[t] = sin^2(pi t / n_fft)
__device__ inline double pv_window(int t, int n_fft) {
  double s, c;
  sincospi((double)t / (double)n_fft, &s, &c);
  return s * s;
}

struct alignas(16) PvC {   // a float64 complex number of the analysis
  double x, y;
};

// arg z, with arg 0 = 0
__device__ inline double pv_arg(PvC z) { return (z.x == 0.0 && z.y == 0.0) ? 0.0 : atan2(z.y, z.x); }

__device__ inline double pv_abs(PvC z) { return sqrt(z.x * z.x + z.y * z.y); }

// magnitude and phase increment of output frame t at bin k: step = t rate = i + alpha, D[i] and D[i + 1] (zero from row F on)
__device__ inline void pv_mag_inc(const PvC *__restrict__ D, int64_t F, int n_fft, int64_t t, double rate, int k, double &mag,
                                  double &inc) {
  const double step = (double)t * rate, whole = floor(step), alpha = step - whole;
  const int64_t i = (int64_t)whole;   // < F: the host counted T so
  const PvC a = D[i * n_fft + k];
  const PvC b = i + 1 < F ? D[(i + 1) * n_fft + k] : PvC{0.0, 0.0};
  mag = (1.0 - alpha) * pv_abs(a) + alpha * pv_abs(b);
  const double phi = PV_PI * (double)(n_fft / 4) * (double)k / (double)(n_fft / 2);
  double d = pv_arg(b) - pv_arg(a) - phi;
  d -= PV_TWO_PI * rint(d / PV_TWO_PI);
  inc = phi + d;
}

// z[f][t] = w[t] xpad[f hop + t] over all F rows (flat index, grid stride)
__global__ __launch_bounds__(256) void k_pv_pack(const float *__restrict__ x, int64_t n, int n_fft, int64_t F, PvC *__restrict__ z) {
  const int hop = n_fft / 4;
  const int64_t total = F * n_fft;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t f = e / n_fft;
    const int t = (int)(e - f * n_fft);
    const int64_t src = f * hop + t - n_fft / 2;
    double v = 0.0;
    if (src >= 0 && src < n) v = (double)x[src] * pv_window(t, n_fft);
    z[e] = PvC{v, 0.0};
  }
}

// One forward Stockham pass of radix R (4 or 2) over `rows` series of n float64 complex points (k_big_pass's indexing):
//   out[(j - k) R + k + q ns] = sum_r in[j + r n / R] w^(r k) (-i)^(r q),  k = j mod ns,  w = e^{-2 pi i / (ns R)}
template <int R>
__global__ __launch_bounds__(256) void k_pv_pass64(const PvC *__restrict__ in, PvC *__restrict__ out, int64_t rows, int n, int ns) {
  const int nb = n / R;
  const int64_t total = rows * nb;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t row = e / nb;
    const int j = (int)(e - row * nb), k = j % ns;
    const PvC *src = in + row * n;
    PvC *dst = out + row * n;
    PvC v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) v[r] = src[j + r * nb];
    if (ns > 1) {
      const double base = -2.0 * (double)k / (double)(ns * R);
#pragma unroll
      for (int r = 1; r < R; ++r) {
        double sn, cs;
        sincospi(base * r, &sn, &cs);
        v[r] = PvC{v[r].x * cs - v[r].y * sn, v[r].x * sn + v[r].y * cs};
      }
    }
    const int base_out = (j - k) * R + k;
    if (R == 2) {
      dst[base_out] = PvC{v[0].x + v[1].x, v[0].y + v[1].y};
      dst[base_out + ns] = PvC{v[0].x - v[1].x, v[0].y - v[1].y};
    } else {
      const PvC a0{v[0].x + v[2].x, v[0].y + v[2].y}, a1{v[0].x - v[2].x, v[0].y - v[2].y};
      const PvC a2{v[1].x + v[3].x, v[1].y + v[3].y}, a3{v[1].y - v[3].y, v[3].x - v[1].x};   // a3 = -i (v1 - v3)
      dst[base_out] = PvC{a0.x + a2.x, a0.y + a2.y};
      dst[base_out + ns] = PvC{a1.x + a3.x, a1.y + a3.y};
      dst[base_out + 2 * ns] = PvC{a0.x - a2.x, a0.y - a2.y};
      dst[base_out + 3 * ns] = PvC{a1.x - a3.x, a1.y - a3.y};
    }
  }
}

// sums[tile][k] = sum of inc[t][k] over the tile's frames, mod 2 pi.  Grid: (tiles, ceil(bins / PV_LANES))
__global__ __launch_bounds__(PV_LANES) void k_pv_phase_sums(const PvC *__restrict__ D, int64_t F, int64_t T, int n_fft, double rate,
                                                            double *__restrict__ sums) {
  const int bins = n_fft / 2 + 1;
  const int k = blockIdx.y * PV_LANES + threadIdx.x;
  if (k >= bins) return;
  const int64_t tile = blockIdx.x, t0 = tile * PV_TILE, t1 = t0 + PV_TILE < T ? t0 + PV_TILE : T;
  double s = 0.0;
  for (int64_t t = t0; t < t1; ++t) {
    double mag, inc;
    pv_mag_inc(D, F, n_fft, t, rate, k, mag, inc);
    s += inc;
  }
  sums[tile * bins + k] = remainder(s, PV_TWO_PI);
}

// sums[tile][k] <- acc[tile PV_TILE][k] mod 2 pi: the exclusive prefix sum of the tile sums, starting from arg D[0][k]
__global__ __launch_bounds__(PV_LANES) void k_pv_phase_carry(const PvC *__restrict__ D, int n_fft, int64_t tiles,
                                                             double *__restrict__ sums) {
  const int bins = n_fft / 2 + 1;
  const int k = blockIdx.x * PV_LANES + threadIdx.x;
  if (k >= bins) return;
  double acc = pv_arg(D[k]);
  for (int64_t tile = 0; tile < tiles; ++tile) {
    const double s = sums[tile * bins + k];
    sums[tile * bins + k] = acc;
    acc = remainder(acc + s, PV_TWO_PI);
  }
}

// S[t][k] = mag[t][k] e^{i acc[t][k]} for the tile's frames, with the Hermitian mirror S[t][n_fft - k] (DC and Nyquist real)
__global__ __launch_bounds__(PV_LANES) void k_pv_phase(const PvC *__restrict__ D, int64_t F, int64_t T, int n_fft, double rate,
                                                       const double *__restrict__ carry, float2 *__restrict__ S) {
  const int bins = n_fft / 2 + 1;
  const int k = blockIdx.y * PV_LANES + threadIdx.x;
  if (k >= bins) return;
  const int64_t tile = blockIdx.x, t0 = tile * PV_TILE, t1 = t0 + PV_TILE < T ? t0 + PV_TILE : T;
  const bool real_bin = k == 0 || k == n_fft / 2;
  double acc = carry[tile * bins + k];
  for (int64_t t = t0; t < t1; ++t) {
    double mag, inc, s, c;
    pv_mag_inc(D, F, n_fft, t, rate, k, mag, inc);
    sincos(acc, &s, &c);
    const float re = (float)(mag * c), im = real_bin ? 0.f : (float)(mag * s);
    S[t * n_fft + k] = make_float2(re, im);
    if (!real_bin) S[t * n_fft + (n_fft - k)] = make_float2(re, -im);
    acc += inc;
  }
}

// out[j] = y[n_fft / 2 + j], y[u] = sum_t w[u - t hop] fr[t][u - t hop] / sum_t w^2[u - t hop]; frames: the UNNORMALISED inverse
// transforms (real parts).  Zero from u = n_fft + hop (T - 1) on.
__global__ __launch_bounds__(256) void k_pv_ola(const float2 *__restrict__ frames, int64_t T, int n_fft, float *__restrict__ out,
                                                int64_t n_out) {
  const int hop = n_fft / 4;
  const int64_t total = (int64_t)n_fft + (int64_t)hop * (T - 1);
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n_out; j += (int64_t)gridDim.x * 256) {
    const int64_t u = j + n_fft / 2;
    double acc = 0.0, ws = 0.0;
    if (u < total) {
      int64_t hi = u / hop;
      if (hi > T - 1) hi = T - 1;
      const int64_t lo = u - n_fft + hop <= 0 ? 0 : (u - n_fft + hop) / hop;   // smallest t with u - t hop < n_fft
      for (int64_t t = lo; t <= hi; ++t) {
        const int64_t off = u - t * hop;
        if (off < 0 || off >= n_fft) continue;
        const double w = pv_window((int)off, n_fft);
        acc += w * (double)frames[t * n_fft + off].x;
        ws += w * w;
      }
    }
    double y = acc / (double)n_fft;
    if (ws > (double)FLT_MIN) y /= ws;
    out[j] = (float)y;
  }
}

// I0(z) by its power series sum_k (z^2 / 4)^k / (k!)^2 (z <= 8.6 here: 30 terms reach 1e-17 of the sum)
__device__ inline double rs_bessel_i0(double z) {
  const double q = 0.25 * z * z;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 200; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-17 * sum) break;
  }
  return sum;
}

// out[t], t < n, from y1[0 .. m): c = 0.95 min(1, n / m), H = 16 / c, p = t m / n = i + rem / n
__global__ __launch_bounds__(256) void k_resample_sinc(const float *__restrict__ y1, int64_t m, float *__restrict__ out, int64_t n,
                                                       double c, double H, double inv_i0_beta) {
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
    const int64_t prod = t * m, i = prod / n, rem = prod - i * n;
    const double frac = (double)rem / (double)n;
    int64_t lo = i - (int64_t)H - 1, hi = i + (int64_t)H + 2;
    if (lo < 0) lo = 0;
    if (hi > m - 1) hi = m - 1;
    double acc = 0.0;
    for (int64_t j = lo; j <= hi; ++j) {
      const double dlt = (double)(i - j) + frac;   // p - j
      if (fabs(dlt) > H) continue;
      const double q = dlt / H;
      double in = 1.0 - q * q;
      if (in < 0.0) in = 0.0;
      const double xarg = c * dlt;
      double sn, cs, sinc = 1.0;
      if (xarg != 0.0) {
        sincospi(xarg, &sn, &cs);
        sinc = sn / (PV_PI * xarg);
      }
      acc += (double)y1[j] * (c * sinc * rs_bessel_i0(RS_BETA * sqrt(in)) * inv_i0_beta);
    }
    out[t] = (float)acc;
  }
}

// ------------------------------------------------------------------ host side: geometry, workspace, launch sequence
inline bool pv_fft_ok(int32_t n_fft) { return n_fft >= PV_MIN_FFT && n_fft <= PV_MAX_FFT && (n_fft & (n_fft - 1)) == 0; }

inline int64_t pv_frames_in(int64_t n, int32_t n_fft) { return 1 + n / (n_fft / 4); }

// the number of t >= 0 with (double)t * rate < F, by the comparison the kernels make
inline int64_t pv_frames_out(int64_t F, double rate) {
  int64_t T = (int64_t)ceil((double)F / rate);
  while (T > 0 && (double)(T - 1) * rate >= (double)F) --T;
  while ((double)T * rate < (double)F) ++T;
  return T;
}

struct PvPlan {
  int64_t F, T, tiles;
  int64_t carry_floats, analysis_floats, floats;
};

inline PvPlan pv_plan(int64_t n, double rate, int32_t n_fft) {
  PvPlan p;
  p.F = pv_frames_in(n, n_fft);
  p.T = pv_frames_out(p.F, rate);
  p.tiles = (p.T + PV_TILE - 1) / PV_TILE;
  p.carry_floats = (2 * p.tiles * (n_fft / 2 + 1) + 3) / 4 * 4;     // float64 carries, kept a multiple of 16 bytes
  p.analysis_floats = 4 * p.F * (int64_t)n_fft;                      // one F x n_fft buffer of float64 complex
  p.floats = p.carry_floats + 2 * p.analysis_floats + 2 * (2 * p.T * (int64_t)n_fft);   // + two T x n_fft float32 complex
  return p;
}

// 0, or the error of the first bad pointer or length; src of n samples, dst of n_out
inline int stretch_check(const char *fn, const float *src, int64_t n, const float *dst, int64_t n_out, const char *n_name,
                         const char *n_out_name, const void *workspace, bool needs_workspace) {
  if (!src || !dst || (needs_workspace && !workspace)) return fail_arg(fn, "null pointer");
  if (n >= 1 && n_out >= 1) return AL_OK;
  char why[160];
  snprintf(why, sizeof(why), "%s must be >= 1", n < 1 ? n_name : n_out_name);
  return fail_arg(fn, why);
}

inline int stretch_overlap_check(const char *fn, const float *src, int64_t n, const float *dst, int64_t n_out) {
  return fx_ranges_overlap(src, n, dst, n_out) ? fail_arg(fn, "dst overlaps src (out of place only)") : AL_OK;
}

// 0, or the error of a bad (n, rate, n_fft): the geometry both time-stretch entries derive
inline int stretch_geometry_check(const char *fn, int64_t n, double rate, int32_t n_fft) {
  const char *why = nullptr;
  if (!pv_fft_ok(n_fft)) why = "n_fft must be a power of two in [64, 4096]";
  else if (!isfinite(rate) || rate < 0.25 || rate > 4.0) why = "rate must be finite and in [0.25, 4]";
  else if (pv_frames_in(n, n_fft) > PV_MAX_FRAMES) why = "too many analysis frames (F = 1 + n / hop must be <= 2^30)";
  else if (pv_frames_out(pv_frames_in(n, n_fft), rate) > PV_MAX_FRAMES) why = "too many output frames (T must be <= 2^30)";
  return why ? fail_arg(fn, why) : AL_OK;
}

inline unsigned pv_flat_grid(int64_t elements) { return grid_1d(elements, 65536); }

// every argument checked by the caller; workspace: pv_plan(...).floats floats, 16-byte aligned
inline void launch_time_stretch(const float *src, int64_t n, float *dst, int64_t n_out, double rate, int32_t n_fft, float *workspace,
                                hipStream_t st) {
  const PvPlan p = pv_plan(n, rate, n_fft);
  double *carry = reinterpret_cast<double *>(workspace);
  PvC *za = reinterpret_cast<PvC *>(workspace + p.carry_floats), *zb = za + p.F * n_fft;
  float2 *sa = reinterpret_cast<float2 *>(workspace + p.carry_floats + 2 * p.analysis_floats), *sb = sa + p.T * n_fft;
  const int bins = n_fft / 2 + 1;
  const unsigned bin_blocks = (unsigned)((bins + PV_LANES - 1) / PV_LANES);
  hipLaunchKernelGGL(k_pv_pack, dim3(pv_flat_grid(p.F * n_fft)), dim3(256), 0, st, src, n, n_fft, p.F, za);
  PvC *in = za, *out = zb;
  for (int ns = 1; ns < n_fft;) {   // radix 4 while it divides, then one radix 2 (big_fft's order)
    const int radix = (n_fft / ns) % 4 == 0 ? 4 : 2;
    const dim3 grid(pv_flat_grid(p.F * (n_fft / radix)));
    if (radix == 4) hipLaunchKernelGGL((k_pv_pass64<4>), grid, dim3(256), 0, st, (const PvC *)in, out, p.F, n_fft, ns);
    else hipLaunchKernelGGL((k_pv_pass64<2>), grid, dim3(256), 0, st, (const PvC *)in, out, p.F, n_fft, ns);
    ns *= radix;
    PvC *t = in; in = out; out = t;
  }
  const PvC *D = in;
  hipLaunchKernelGGL(k_pv_phase_sums, dim3((unsigned)p.tiles, bin_blocks), dim3(PV_LANES), 0, st, D, p.F, p.T, n_fft, rate, carry);
  hipLaunchKernelGGL(k_pv_phase_carry, dim3(bin_blocks), dim3(PV_LANES), 0, st, D, n_fft, p.tiles, carry);
  hipLaunchKernelGGL(k_pv_phase, dim3((unsigned)p.tiles, bin_blocks), dim3(PV_LANES), 0, st, D, p.F, p.T, n_fft, rate,
                     (const double *)carry, sa);
  const float2 *frames = sa;
  for (int64_t t0 = 0; t0 < p.T; t0 += MAX_GRID_ROWS) {
    const int g = (int)(p.T - t0 < MAX_GRID_ROWS ? p.T - t0 : MAX_GRID_ROWS);
    float2 *z = big_fft(sa + t0 * n_fft, sb + t0 * n_fft, g, n_fft, +1, st);
    frames = z == sa + t0 * n_fft ? sa : sb;   // every group ends in the same buffer (same pass count)
  }
  hipLaunchKernelGGL(k_pv_ola, dim3(grid_1d(n_out, 8192)), dim3(256), 0, st, frames, p.T, n_fft, dst, n_out);
}

inline void launch_resample_sinc(const float *src, int64_t m, float *dst, int64_t n, hipStream_t st) {
  const double ratio = (double)n / (double)m;
  const double c = RS_ROLLOFF * (ratio < 1.0 ? ratio : 1.0), H = RS_ZEROS / c;
  double term = 1.0, i0 = 1.0;   // I0(beta), the series of rs_bessel_i0
  for (int k = 1; k < 200; ++k) {
    term *= 0.25 * RS_BETA * RS_BETA / ((double)k * (double)k);
    i0 += term;
    if (term < 1e-17 * i0) break;
  }
  hipLaunchKernelGGL(k_resample_sinc, dim3(grid_1d(n, 16384)), dim3(256), 0, st, src, m, dst, n, c, H, 1.0 / i0);
}

}  // namespace al
