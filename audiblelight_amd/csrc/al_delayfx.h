// Delay and modulation FX (A14: Delay, Chorus, Phaser; audiblelight/augmentation.py:746-829, 963-1043, 1046-1102) as linear
// recursions with feedback.  The definitions (pedalboard 0.9.17's Delay, JUCE's dsp::Chorus / dsp::Phaser as this project reads
// them, pinned by definition) are in DESIGN.md "Delay and modulation FX" and in include/audiblelight_hip.h; every state starts at
// zero and the output has the input's length.  All three are out of place, and no workgroup waits on another.
//
// k_fx_delay   d[t] = x[t-D] + fb d[t-D] is D interleaved first-order chains (residues t mod D).  A workgroup holds G
//              consecutive residues (coalesced) x P runs of each chain; a run's zero-state end value, a Hillis-Steele scan of
//              the runs' carries with Phi = fb^run over the P runs of a residue, then every run again from its true state.
// k_fx_chorus_ff   feedback 0: v is a gather-interpolate of x, grid-wide.
// k_fx_chorus_fb   feedback > 0: v[t] reads u at t - tau_t <= t - B, so ONE workgroup walks the clip in blocks of B samples:
//              v of the block from the u history (an LDS ring), then u of the block.
// k_fx_phaser  state S = (s1..s6, L); one workgroup, runs of a multiple of 4 samples (the LFO ticks every 4): each run's
//              affine map S_out = M S_in + e (7 basis trajectories + the particular one), the carries as a sequential
//              matrix-vector chain in one thread (through LDS in batches of PH_BATCH runs), every run again from its true state.
// Recursion state is float64 (where float32 misses 1e-5); the Chorus u history is float32 in LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "al_common.h"
#include "al_status.h"

namespace al {

constexpr double DFX_PI = 3.14159265358979323846;

// What the entries of these FX (and of the dynamics FX) ask of a clip and of its scalars: out of place, n >= 1, every named value
// finite and >= 0, "feedback" below 1.  0, or the error of the first bad argument under the entry's name `fn`.
inline int fx_check(const char *fn, const float *src, const float *dst, int64_t n, const char *const *names, const double *vals,
                    int count) {
  if (!src || !dst) return fail_arg(fn, "null pointer");
  if (n < 1) return fail_arg(fn, "n must be >= 1");
  if (fx_ranges_overlap(src, n, dst, n)) return fail_arg(fn, "dst overlaps src (out of place only)");
  for (int i = 0; i < count; ++i) {
    if (!isfinite(vals[i]) || vals[i] < 0.0) {
      char why[160];
      snprintf(why, sizeof(why), "%s must be finite and >= 0", names[i]);
      return fail_arg(fn, why);
    }
    if (!strcmp(names[i], "feedback") && vals[i] >= 1.0) return fail_arg(fn, "feedback must be < 1 (unstable loop)");
  }
  return AL_OK;
}

// ------------------------------------------------------------------ Delay
constexpr int DLY_THREADS = 1024;
constexpr int DLY_MIN_RUN = 16;   // chain steps per run below which more runs per residue stop paying

struct DelayPlan {
  int64_t D;          // delay in samples (>= 1 when K >= 1)
  int64_t K;          // longest chain: floor((n - 1) / D) delayed samples; 0 when D == 0 or D >= n
  int64_t R;          // chain steps per run
  int64_t residues;   // min(D, n), or n when there is no chain
  int32_t G, P;       // residues per workgroup (power of two), runs per residue (power of two); G * P threads
  double phi;         // fb^R
};

inline int64_t dfx_pow2_ceil(int64_t v) {
  int64_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

inline DelayPlan delay_plan(int64_t n, int64_t D, double fb) {
  DelayPlan p;
  p.D = D;
  p.K = (D >= 1 && D < n) ? (n - 1) / D : 0;
  p.residues = p.K > 0 ? D : n;
  if (p.K == 0) {
    p.G = DLY_THREADS;
    p.P = 1;
  } else {
    p.G = (int32_t)(p.residues < 64 ? dfx_pow2_ceil(p.residues) : 64);
    const int64_t want = dfx_pow2_ceil((p.K + DLY_MIN_RUN - 1) / DLY_MIN_RUN);
    p.P = (int32_t)(want < DLY_THREADS / p.G ? want : DLY_THREADS / p.G);
  }
  p.R = p.K > 0 ? (p.K + p.P - 1) / p.P : 0;
  p.phi = pow(fb, (double)p.R);
  return p;
}

inline int delay_check(const float *src, const float *dst, int64_t n, int64_t delay_samples, float feedback, float mix) {
  static const char *const names[] = {"feedback", "mix"};
  const double vals[] = {feedback, mix};
  if (int e = fx_check("al_fx_delay", src, dst, n, names, vals, 2)) return e;
  if (delay_samples < 0) return fail(AL_E_BADARG, "al_fx_delay: delay_samples must be >= 0");
  return AL_OK;
}

// y[t] = dry x[t] + wet d[t].  Thread (g, p): residue r = blockIdx.x * G + g, chain steps k in [p R + 1, (p + 1) R] (t = r + k D).
__global__ __launch_bounds__(1024) void k_fx_delay(const float *x, float *y, int64_t n, DelayPlan pl, double fb, double dry,
                                                   double wet) {
  __shared__ double carry[DLY_THREADS];
  const int tid = threadIdx.x;
  const int g = tid & (pl.G - 1), p = tid / pl.G;
  const int64_t r = (int64_t)blockIdx.x * pl.G + g;
  const bool active = r < pl.residues;
  if (active && p == 0) y[r] = (float)(dry * (double)x[r]);   // t < D: the line is still empty
  const int64_t kr = (active && pl.K > 0) ? (n - 1 - r) / pl.D : 0;   // this residue's chain length
  const int64_t k0 = (int64_t)p * pl.R + 1;
  const int64_t k1 = kr < k0 + pl.R - 1 ? kr : k0 + pl.R - 1;
  // 1. zero-state end value of the run
  double a = 0.0;
  for (int64_t k = k0; k <= k1; ++k) a = fma(fb, a, (double)x[r + (k - 1) * pl.D]);
  // 2. carries over the P runs of the residue: w[p] += Phi^d w[p - d]
  double w = a, ph = pl.phi;
  for (int d = 1; d < pl.P; d <<= 1) {
    carry[tid] = w;
    __syncthreads();
    if (p >= d) w = fma(ph, carry[tid - d * pl.G], w);
#ifndef AL_TEST_REVERT_DELAY_BARRIER   // tests/shake.py `revert`: without it the next step's carry[tid] = w overtakes this step's reads
    __syncthreads();
#endif
    ph *= ph;
  }
  carry[tid] = w;
  __syncthreads();
  double s = p > 0 ? carry[tid - pl.G] : 0.0;
  // 3. the run from its true entering value
  if (k0 <= k1) {
    float xprev = x[r + (k0 - 1) * pl.D];
    for (int64_t k = k0; k <= k1; ++k) {
      const int64_t t = r + k * pl.D;
      const float xt = x[t];
      s = fma(fb, s, (double)xprev);
      y[t] = (float)fma(wet, s, dry * (double)xt);
      xprev = xt;
    }
  }
}

// ------------------------------------------------------------------ Chorus
constexpr int CHO_THREADS = 1024;
constexpr int CHO_RING = 16384;   // float u history (64 KiB); al_fx_chorus refuses fs whose ceil(0.11 fs) + B + 2 exceeds it
constexpr int CHO_MAX_BLOCK = CHO_THREADS;

struct ChorusArgs {
  double fs, rate, depth10, centre_ms, tau_max, fb, dry, wet;
  int64_t block;   // B: floor of a lower bound of tau_t, at least floor(fs / 1000), at most CHO_MAX_BLOCK
};

// tau_t = clamp(max(1, 10 depth lfo_t + centre) fs / 1000, 0, tau_max), lfo_t = sin(2 pi rate t / fs - pi)
__device__ inline double chorus_tau(const ChorusArgs &a, int64_t t) {
  const double lfo = sin(2.0 * DFX_PI * a.rate * (double)t / a.fs - DFX_PI);
  const double tau = fmax(1.0, a.depth10 * lfo + a.centre_ms) * a.fs / 1000.0;
  return fmin(fmax(tau, 0.0), a.tau_max);
}

// v[t] = x[t - i] + f (x[t - i - 1] - x[t - i]), x[m] = 0 for m < 0
__global__ __launch_bounds__(256) void k_fx_chorus_ff(const float *x, float *y, int64_t n, ChorusArgs a) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
    const double tau = chorus_tau(a, t);
    const int64_t i = (int64_t)tau;
    const double f = tau - (double)i;
    const int64_t m = t - i;
    const double u0 = m >= 0 ? (double)x[m] : 0.0, u1 = m >= 1 ? (double)x[m - 1] : 0.0;
    const double v = fma(f, u1 - u0, u0);
    y[t] = (float)fma(a.wet, v, a.dry * (double)x[t]);
  }
}

// One clip's launch of k_fx_chorus_fb: what al_fx_chorus derives from its arguments (one per workgroup of a batched launch).
struct ChorusJob {
  const float *src;
  float *dst;
  int64_t n;
  ChorusArgs a;
};

// u[t] = x[t] - fb v[t-1]; v[t] from u[t - i], u[t - i - 1] with i >= B.  Block [s, s + B): every v, then every u.
// Workgroup b takes job b: table[b], or `one` when table == nullptr (grid of 1); the same instantiation either way.
__global__ __launch_bounds__(1024) void k_fx_chorus_fb(const ChorusJob *__restrict__ table, ChorusJob one) {
  __shared__ float ring[CHO_RING];   // u[m] at m & (CHO_RING - 1); holds u[s - tau_max - 1, s + B)
  __shared__ double vb[CHO_MAX_BLOCK];
  const ChorusJob *job = table ? table + blockIdx.x : nullptr;
  const float *x = job ? job->src : one.src;
  float *y = job ? job->dst : one.dst;
  const int64_t n = job ? job->n : one.n;
  const ChorusArgs a = job ? job->a : one.a;
  const int j = threadIdx.x;
  const int64_t B = a.block;
  double vlast = 0.0;   // v[s - 1]
  for (int64_t s = 0; s < n; s += B) {
    const int64_t t = s + j;
    const bool act = j < B && t < n;
    double xt = 0.0, v = 0.0;
    if (act) {
      xt = (double)x[t];
      const double tau = chorus_tau(a, t);
      const int64_t i = (int64_t)tau;
      const double f = tau - (double)i;
      const int64_t m = t - i;   // <= s - 1: written by an earlier block
      const double u0 = m >= 0 ? (double)ring[m & (CHO_RING - 1)] : 0.0;
      const double u1 = m >= 1 ? (double)ring[(m - 1) & (CHO_RING - 1)] : 0.0;
      v = fma(f, u1 - u0, u0);
      vb[j] = v;
    }
    __syncthreads();
    const double vprev = j == 0 ? vlast : (act ? vb[j - 1] : 0.0);
    vlast = vb[B - 1];   // read before the barrier below: the next block overwrites vb after it
    if (act) {
      ring[t & (CHO_RING - 1)] = (float)fma(-a.fb, vprev, xt);
      y[t] = (float)fma(a.wet, v, a.dry * xt);
    }
    __syncthreads();
  }
}

// 0 with *job filled, or the error of the first bad argument.  The same job feeds k_fx_chorus_ff (feedback == 0: job->a alone).
inline int chorus_prepare(const al_fx_mod_job &in, ChorusJob *job) {
  static const char *const names[] = {"fs", "rate_hz", "depth", "centre_delay_ms", "feedback", "mix"};
  const double vals[] = {in.fs, in.rate_hz, in.depth, in.centre, in.feedback, in.mix};
  if (int e = fx_check("al_fx_chorus", in.src, in.dst, in.n, names, vals, 6)) return e;
  const double tau_max = ceil(110.0 * in.fs / 1000.0);
  const double b_min = floor(in.fs / 1000.0);   // tau >= fs / 1000: the 1 ms floor of the delay
  if (!(b_min >= 1.0) || tau_max + b_min + 2.0 > (double)CHO_RING)
    return fail(AL_E_BADARG, "al_fx_chorus: fs out of range (1000 <= fs and ceil(0.11 fs) + floor(fs / 1000) + 2 <= 16384)");
  job->src = in.src;
  job->dst = in.dst;
  job->n = in.n;
  ChorusArgs &a = job->a;
  a.fs = in.fs;
  a.rate = in.rate_hz;
  a.depth10 = 10.0 * in.depth;
  a.centre_ms = in.centre;
  a.tau_max = tau_max;
  a.fb = in.feedback;
  const double m = in.mix < 1.0 ? in.mix : 1.0;   // JUCE's DryWetMixer clamps the proportion
  a.dry = 1.0 - m;
  a.wet = m;
  // B = floor of a lower bound of every tau_t, one sample short of it against rounding, never below the 1 ms floor
  const double lowest = fmin(fmax(1.0, in.centre - 10.0 * in.depth) * in.fs / 1000.0, tau_max);
  double b = floor(lowest) - 1.0;
  b = b > b_min ? b : b_min;
  b = b < (double)CHO_MAX_BLOCK ? b : (double)CHO_MAX_BLOCK;
  b = b < (double)CHO_RING - tau_max - 2.0 ? b : (double)CHO_RING - tau_max - 2.0;
  a.block = (int64_t)b;
  return AL_OK;
}

// ------------------------------------------------------------------ Phaser
constexpr int PH_THREADS = 512;    // runs; 8 trajectories x 7 float64 states per thread need the VGPRs of 2 waves per SIMD
constexpr int PH_BATCH = 128;      // runs whose maps sit in LDS at once for the carry chain (128 x 56 float64 = 56 KiB)
constexpr int PH_STAGES = 6;
constexpr int PH_DIM = PH_STAGES + 1;   // s1..s6, L

struct PhaserArgs {
  double fs, rate, half_depth, c, log_ratio, fb, dry, wet;   // c = log10(fc/20) / log10(fmax/20); log_ratio = ln(fmax/20)
};

// runs of a multiple of 4 samples
__host__ __device__ inline int64_t phaser_run_length(int64_t n) {
  const int64_t per = (n + PH_THREADS - 1) / PH_THREADS;
  return (per + 3) / 4 * 4;
}

// G of the all-passes for LFO tick k (samples 4k .. 4k + 3)
__device__ inline double phaser_gain(const PhaserArgs &a, int64_t k) {
  const double s = sin(2.0 * DFX_PI * a.rate * (double)(4 * k) / a.fs - DFX_PI);
  const double lfo = fmin(fmax(fma(a.half_depth, s, a.c), 0.0), 1.0);
  const double fk = 20.0 * exp(lfo * a.log_ratio);
  const double g = tan(DFX_PI * fk / a.fs);
  return g / (1.0 + g);
}

// one sample through the six TPT all-passes with feedback; st[PH_STAGES] = L.  Returns the wet sample.
__device__ inline double phaser_step(double *st, double G, double fb, double xin) {
  double in = xin - st[PH_STAGES];
#pragma unroll
  for (int i = 0; i < PH_STAGES; ++i) {
    const double v = G * (in - st[i]);
    const double lp = v + st[i];
    st[i] = lp + v;
    in = 2.0 * lp - in;
  }
  st[PH_STAGES] = fb * in;
  return in;
}

// One clip's launch: what al_fx_phaser derives from its arguments (one per workgroup of a batched launch).
struct PhaserJob {
  const float *src;
  float *dst;
  int64_t n, run;
  PhaserArgs a;
};

// Workgroup b takes job b: table[b], or `one` when table == nullptr (grid of 1); the same instantiation either way.
__global__ __launch_bounds__(PH_THREADS) void k_fx_phaser(const PhaserJob *__restrict__ table, PhaserJob one) {
  __shared__ double maps[PH_BATCH][PH_DIM * PH_DIM + PH_DIM];   // M row-major, then e; e is replaced by the entering state
  const PhaserJob *job = table ? table + blockIdx.x : nullptr;
  const float *x = job ? job->src : one.src;
  float *y = job ? job->dst : one.dst;
  const int64_t n = job ? job->n : one.n, run = job ? job->run : one.run;
  const PhaserArgs a = job ? job->a : one.a;
  const int tid = threadIdx.x;
  const int64_t lo = (int64_t)tid * run;
  const int64_t hi = lo + run < n ? lo + run : n;   // may be <= lo: an empty run (identity map)
  // 1. the run's affine map: trajectory c < 7 starts at basis vector c with x = 0, trajectory 7 at zero with x
  double tr[PH_DIM + 1][PH_DIM];
#pragma unroll
  for (int c = 0; c <= PH_DIM; ++c)
#pragma unroll
    for (int i = 0; i < PH_DIM; ++i) tr[c][i] = (c == i) ? 1.0 : 0.0;
  for (int64_t t4 = lo; t4 < hi; t4 += 4) {
    const double G = phaser_gain(a, t4 / 4);
    const int m = hi - t4 < 4 ? (int)(hi - t4) : 4;
    for (int q = 0; q < m; ++q) {
      const double xin = (double)x[t4 + q];
#pragma unroll
      for (int c = 0; c < PH_DIM; ++c) phaser_step(tr[c], G, a.fb, 0.0);
      phaser_step(tr[PH_DIM], G, a.fb, xin);
    }
  }
  // 2. carries S[j + 1] = M_j S[j] + e_j, in batches of PH_BATCH runs, by thread 0
  double S[PH_DIM];
#pragma unroll
  for (int i = 0; i < PH_DIM; ++i) S[i] = 0.0;
  double entry[PH_DIM];
  for (int b = 0; b < PH_THREADS / PH_BATCH; ++b) {
    const bool mine = tid / PH_BATCH == b;
    double *row = maps[tid % PH_BATCH];
    if (mine) {
#pragma unroll
      for (int r = 0; r < PH_DIM; ++r) {
#pragma unroll
        for (int c = 0; c < PH_DIM; ++c) row[r * PH_DIM + c] = tr[c][r];
        row[PH_DIM * PH_DIM + r] = tr[PH_DIM][r];
      }
    }
    __syncthreads();
    if (tid == 0) {
      for (int jj = 0; jj < PH_BATCH; ++jj) {
        double *mp = maps[jj];
        double nxt[PH_DIM];
#pragma unroll
        for (int r = 0; r < PH_DIM; ++r) {
          double acc = mp[PH_DIM * PH_DIM + r];
#pragma unroll
          for (int c = 0; c < PH_DIM; ++c) acc = fma(mp[r * PH_DIM + c], S[c], acc);
          nxt[r] = acc;
        }
#pragma unroll
        for (int r = 0; r < PH_DIM; ++r) {
          mp[PH_DIM * PH_DIM + r] = S[r];
          S[r] = nxt[r];
        }
      }
    }
    __syncthreads();
    if (mine) {
#pragma unroll
      for (int r = 0; r < PH_DIM; ++r) entry[r] = row[PH_DIM * PH_DIM + r];
    }
    __syncthreads();
  }
  // 3. the run from its true entering state
  for (int64_t t4 = lo; t4 < hi; t4 += 4) {
    const double G = phaser_gain(a, t4 / 4);
    const int m = hi - t4 < 4 ? (int)(hi - t4) : 4;
    for (int q = 0; q < m; ++q) {
      const double xin = (double)x[t4 + q];
      const double wet = phaser_step(entry, G, a.fb, xin);
      y[t4 + q] = (float)fma(a.wet, wet, a.dry * xin);
    }
  }
}

// 0 with *job filled, or the error of the first bad argument
inline int phaser_prepare(const al_fx_mod_job &in, PhaserJob *job) {
  static const char *const names[] = {"fs", "rate_hz", "depth", "centre_frequency_hz", "feedback", "mix"};
  const double vals[] = {in.fs, in.rate_hz, in.depth, in.centre, in.feedback, in.mix};
  if (int e = fx_check("al_fx_phaser", in.src, in.dst, in.n, names, vals, 6)) return e;
  if (!(0.49 * in.fs > 20.0)) return fail(AL_E_BADARG, "al_fx_phaser: fs out of range (0.49 fs must exceed 20 Hz)");
  const double fmax_hz = fmin(20000.0, 0.49 * in.fs);
  job->src = in.src;
  job->dst = in.dst;
  job->n = in.n;
  job->run = phaser_run_length(in.n);
  PhaserArgs &a = job->a;
  a.fs = in.fs;
  a.rate = in.rate_hz;
  a.half_depth = 0.5 * in.depth;
  a.c = log10(in.centre / 20.0) / log10(fmax_hz / 20.0);   // -inf at fc = 0: the LFO clamps it to 0
  a.log_ratio = log(fmax_hz / 20.0);
  a.fb = in.feedback;
  const double m = in.mix < 1.0 ? in.mix : 1.0;
  a.dry = 1.0 - m;
  a.wet = m;
  return AL_OK;
}

}  // namespace al
