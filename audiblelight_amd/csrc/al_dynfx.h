// Dynamics FX (A14: Compressor, Limiter; audiblelight/augmentation.py:663-743, 871-924).  The definitions (JUCE's dsp::Compressor,
// dsp::BallisticsFilter in peak mode and dsp::Limiter as pedalboard 0.9.17 wraps them and as this project reads them, pinned by
// definition and NOT checked against a running pedalboard) are in DESIGN.md "Dynamics FX" and in include/audiblelight_hip.h; every
// state starts at zero and the output has the input's length.  Out of place; no workgroup waits on another.
//
// A stage (T, ratio, cA, cR):  a = |x|,  e <- a + c (e - a) with c = cA when a > e, else cR,  g = 1 when e < T, else
// (e / T)^(1/ratio - 1),  y = g x.  The coefficient depends on the state, so the recursion is no affine scan (DESIGN.md "why no
// scan"): the time axis is walked serially and the parallelism is over clips (one workgroup each) and over stages.
//
// k_fx_dynamics  one wave per clip, tiles of DYN_TILE samples.  Per tile: all lanes load x and write the walk's operands to LDS;
//              lane s < n_stages walks stage s's envelope (lane 0 stage 1 on tile k, lane 1 stage 2 on tile k - 1: a one-tile skew,
//              so a Limiter costs one walk per sample); all lanes do the pointwise work (gains, the second stage's input, the store).
//              The walk is  z <- max(cR z + p, cA z + q)  with p = s (1 - cR) a, q = s (1 - cA) a, z = s e and s = +1 when
//              cA <= cR, -1 otherwise (then the max is the min of the definition): equal to the compare / select form in exact
//              arithmetic, with a dependent chain of one fma and one max.
// The __syncthreads() between the phases order LDS traffic only: with one wave per workgroup hipcc emits no barrier instruction.
// All arithmetic and state are float64.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "al_common.h"
#include "al_delayfx.h"   // fx_check
#include "al_status.h"

namespace al {

constexpr int DYN_LANES = 64;
constexpr int DYN_TILE = 1024;   // samples per tile ; 60 bytes of LDS per sample
constexpr int DYN_PER_LANE = DYN_TILE / DYN_LANES;
constexpr int DYN_UNROLL = 8;    // walk operands read ahead of the dependent chain

struct DynStage {
  double T, invT, slope, cA, cR;   // threshold (linear), 1 / T, 1 / ratio - 1, attack and release coefficients
};

// One clip's launch: what al_fx_compressor / al_fx_limiter derive from their arguments (one per workgroup of a batched launch).
struct DynJob {
  const float *src;
  float *dst;
  int64_t n;
  int32_t n_stages, reserved;   // 1: Compressor, 2: Limiter
  DynStage st[2];
  double out_gain, ceiling;     // y = clamp(out_gain * y_last, -ceiling, ceiling); a Compressor: 1, +inf
};

struct alignas(16) DynPair {
  double p, q;   // s (1 - cR) a, s (1 - cA) a
};

// g(e) of a stage
__device__ inline double dyn_gain(const DynStage &st, double e) { return e < st.T ? 1.0 : exp(st.slope * log(e * st.invT)); }

// the instruction scheduler may not move anything across this point (device code only)
#if defined(__HIP_DEVICE_COMPILE__)
#define DYN_KEEP_ORDER() __builtin_amdgcn_sched_barrier(0)
#else
#define DYN_KEEP_ORDER() ((void)0)
#endif

// DYN_UNROLL operands of a walk into registers
__device__ inline void dyn_read(DynPair *o, const DynPair *from) {
#pragma unroll
  for (int u = 0; u < DYN_UNROLL; ++u) o[u] = from[u];
}

__device__ inline void dyn_store(double *to, const double *r) {
#pragma unroll
  for (int u = 0; u < DYN_UNROLL; ++u) to[u] = r[u];
}

// DYN_UNROLL steps of z <- max(cR z + p, cA z + q) into r; returns z.  `lds` runs after the first step: the LDS traffic of the
// neighbouring groups is issued there, so that the wait for THIS group's operands (a full one: hipcc waits for every LDS
// operation in flight) comes before it and the rest of the walk covers its latency.
template <class F>
__device__ inline double dyn_walk(const DynPair *o, double *r, double cR, double cA, double z, F &&lds) {
  z = fmax(fma(cR, z, o[0].p), fma(cA, z, o[0].q));
  r[0] = z;
  DYN_KEEP_ORDER();
  lds();
  DYN_KEEP_ORDER();
#pragma unroll
  for (int u = 1; u < DYN_UNROLL; ++u) {
    z = fmax(fma(cR, z, o[u].p), fma(cA, z, o[u].q));
    r[u] = z;
  }
  return z;
}

// Workgroup b takes job b: table[b], or `one` when table == nullptr (grid of 1); the same instantiation either way.
__global__ __launch_bounds__(64) void k_fx_dynamics(const DynJob *__restrict__ table, DynJob one) {
  __shared__ DynPair ops[2][DYN_TILE + DYN_UNROLL];   // the walk's operands, per stage; the tail: a read-ahead past the tile stays inside
  __shared__ double env[2][DYN_TILE];    // z = s e, per stage
  __shared__ double y1s[DYN_TILE];       // the first stage's output (two stages)
  __shared__ float xs[DYN_TILE];
  const DynJob *job = table ? table + blockIdx.x : nullptr;
  const float *x = job ? job->src : one.src;
  float *y = job ? job->dst : one.dst;
  const int64_t n = job ? job->n : one.n;
  const int stages = job ? job->n_stages : one.n_stages;
  const DynStage s0 = job ? job->st[0] : one.st[0], s1 = job ? job->st[1] : one.st[1];
  const double out_gain = job ? job->out_gain : one.out_gain, ceiling = job ? job->ceiling : one.ceiling;
  const int lane = threadIdx.x;
  const double sg0 = s0.cA <= s0.cR ? 1.0 : -1.0, sg1 = s1.cA <= s1.cR ? 1.0 : -1.0;
  const double p0 = sg0 * (1.0 - s0.cR), q0 = sg0 * (1.0 - s0.cA), p1 = sg1 * (1.0 - s1.cR), q1 = sg1 * (1.0 - s1.cA);
  // the walker's own stage
  const bool walker = lane < stages;
  const double wR = lane == 1 ? s1.cR : s0.cR, wA = lane == 1 ? s1.cA : s0.cA;
  const DynPair *wops = ops[lane == 1 ? 1 : 0];
  double *wenv = env[lane == 1 ? 1 : 0];
  double z = 0.0;

  const int64_t tiles = (n + DYN_TILE - 1) / DYN_TILE;
  float xr[DYN_PER_LANE];   // the next tile of x, in flight during the walk
#pragma unroll
  for (int j = 0; j < DYN_PER_LANE; ++j) {
    const int64_t t = (int64_t)j * DYN_LANES + lane;
    xr[j] = t < n ? x[t] : 0.f;
  }
  for (int64_t k = 0; k < tiles + (stages == 2 ? 1 : 0); ++k) {
    const int64_t rest = n - k * DYN_TILE, prev = n - (k - 1) * DYN_TILE;
    const int len = rest <= 0 ? 0 : rest < DYN_TILE ? (int)rest : DYN_TILE;             // tile k (0 in the drain iteration)
    const int len_prev = k == 0 ? 0 : prev < DYN_TILE ? (int)prev : DYN_TILE;            // tile k - 1
    // 1. tile k of x -> LDS, with the first stage's operands; tile k + 1 -> registers
#pragma unroll
    for (int j = 0; j < DYN_PER_LANE; ++j) {
      const int i = j * DYN_LANES + lane;
      if (i < len) {
        const double a = fabs((double)xr[j]);
        xs[i] = xr[j];
        ops[0][i] = DynPair{p0 * a, q0 * a};
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < DYN_PER_LANE; ++j) {
      const int64_t t = (k + 1) * DYN_TILE + (int64_t)j * DYN_LANES + lane;
      xr[j] = t < n ? x[t] : 0.f;
    }
    // 2. the walks: lane 0 over tile k, lane 1 over tile k - 1
    if (walker) {
      const int wlen = lane == 1 ? len_prev : len;
      // groups of DYN_UNROLL samples, two sets of registers in turns: while group g is walked, the results of group g - 1 go to
      // LDS and the operands of group g + 1 come from it.  The read-ahead is unconditional: past wlen it reads what is never
      // walked (the tail of `ops`)
      const int groups = wlen / DYN_UNROLL;
      int t = 0;
      if (groups > 0) {
        DynPair oa[DYN_UNROLL], ob[DYN_UNROLL];
        double ra[DYN_UNROLL], rb[DYN_UNROLL];
        dyn_read(oa, wops);
        z = dyn_walk(oa, ra, wR, wA, z, [&] { dyn_read(ob, wops + DYN_UNROLL); });
        int g = 1;   // ob holds the operands of group g, ra the results of group g - 1
        for (; g + 1 < groups; g += 2) {
          z = dyn_walk(ob, rb, wR, wA, z, [&] {
            dyn_store(wenv + (g - 1) * DYN_UNROLL, ra);
            dyn_read(oa, wops + (g + 1) * DYN_UNROLL);
          });
          z = dyn_walk(oa, ra, wR, wA, z, [&] {
            dyn_store(wenv + g * DYN_UNROLL, rb);
            dyn_read(ob, wops + (g + 2) * DYN_UNROLL);
          });
        }
        dyn_store(wenv + (g - 1) * DYN_UNROLL, ra);
        if (g < groups) {
          z = dyn_walk(ob, rb, wR, wA, z, [] {});
          dyn_store(wenv + g * DYN_UNROLL, rb);
        }
        t = groups * DYN_UNROLL;
      }
      for (; t < wlen; ++t) {
        z = fmax(fma(wR, z, wops[t].p), fma(wA, z, wops[t].q));
        wenv[t] = z;
      }
    }
    __syncthreads();
    // 3a. tile k - 1 through the second stage's gain, the output gain and the ceiling
    if (stages == 2)
      for (int i = lane; i < len_prev; i += DYN_LANES) {
        const double v = out_gain * (dyn_gain(s1, sg1 * env[1][i]) * y1s[i]);
        y[(k - 1) * DYN_TILE + i] = (float)fmin(fmax(v, -ceiling), ceiling);
      }
    __syncthreads();
    // 3b. tile k through the first stage's gain: the output (one stage), or the second stage's input
    for (int i = lane; i < len; i += DYN_LANES) {
      const double v = dyn_gain(s0, sg0 * env[0][i]) * (double)xs[i];
      if (stages == 2) {
        const double a = fabs(v);
        y1s[i] = v;
        ops[1][i] = DynPair{p1 * a, q1 * a};
      } else {
        y[k * DYN_TILE + i] = (float)fmin(fmax(out_gain * v, -ceiling), ceiling);
      }
    }
    __syncthreads();
  }
}

// ---- host side: the checks both entries share, then the stages of each
constexpr double DYN_TWO_PI = 6.283185307179586476925286766559;

// cte(ms): the one-pole coefficient of a time constant, 0 below a microsecond (JUCE's BallisticsFilter)
inline double dyn_cte(double ms, double fs) { return ms < 1e-3 ? 0.0 : exp(-DYN_TWO_PI * 1000.0 / (ms * fs)); }

inline DynStage dyn_stage(double threshold_db, double ratio, double cA, double cR) {
  const double T = pow(10.0, threshold_db / 20.0);
  return DynStage{T, 1.0 / T, 1.0 / ratio - 1.0, cA, cR};
}

// 0 with the clip of `in` in a zeroed *job, or the error of the first bad argument
template <class Job>
inline int dyn_check(const char *fn, const Job &in, bool limiter, double ratio, double attack_ms, DynJob *job) {
  if (int e = fx_check(fn, in.src, in.dst, in.n, nullptr, nullptr, 0)) return e;
  const char *why = nullptr;
  if (!isfinite(in.fs) || !(in.fs > 0.0)) why = "fs must be finite and > 0";
  else if (!isfinite(in.threshold_db) || !(in.threshold_db > -200.0)) why = "threshold_db must be finite and > -200";
  else if (limiter && !(in.threshold_db < 100.0)) why = "threshold_db must be < 100";
  else if (!isfinite(ratio) || !(ratio >= 1.0)) why = "ratio must be finite and >= 1";
  else if (!isfinite(attack_ms) || attack_ms < 0.0) why = "attack_ms must be finite and >= 0";
  else if (!isfinite(in.release_ms) || in.release_ms < 0.0) why = "release_ms must be finite and >= 0";
  if (why) return fail_arg(fn, why);
  memset(job, 0, sizeof(*job));
  job->src = in.src;
  job->dst = in.dst;
  job->n = in.n;
  return AL_OK;
}

inline int compressor_prepare(const al_fx_compressor_job &in, DynJob *job) {
  if (int e = dyn_check("al_fx_compressor", in, false, in.ratio, in.attack_ms, job)) return e;
  job->n_stages = 1;
  job->st[0] = dyn_stage(in.threshold_db, in.ratio, dyn_cte(in.attack_ms, in.fs), dyn_cte(in.release_ms, in.fs));
  job->st[1] = job->st[0];   // not walked
  job->out_gain = 1.0;
  job->ceiling = INFINITY;
  return AL_OK;
}

// JUCE's dsp::Limiter: a fixed first compressor, the caller's second one (attack 0.001 ms: cA = 0), the make-up gain, the clamp
inline int limiter_prepare(const al_fx_limiter_job &in, DynJob *job) {
  if (int e = dyn_check("al_fx_limiter", in, true, 1000.0, 0.0, job)) return e;
  job->n_stages = 2;
  job->st[0] = dyn_stage(-10.0, 4.0, dyn_cte(2.0, in.fs), dyn_cte(200.0, in.fs));
  job->st[1] = dyn_stage(in.threshold_db, 1000.0, 0.0, dyn_cte(in.release_ms, in.fs));
  job->out_gain = pow(10.0, 10.0 * (1.0 - 1.0 / 4.0) / 40.0) * pow(10.0, -in.threshold_db / 20.0);
  job->ceiling = 1.0;
  return AL_OK;
}

}  // namespace al
