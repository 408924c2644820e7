// Cascades of second-order IIR sections (A14 filter FX: LowpassFilter, HighpassFilter, LowShelfFilter, HighShelfFilter and the
// peak bands of MultibandEqualizer; audiblelight/augmentation.py:303-660) as ONE workgroup-wide chunked linear-recurrence scan.
//
// Section k (normalised by a0) in transposed direct form II, state s = (s1, s2):
//   y = b0 x + s1,   s1' = b1 x - a1 y + s2,   s2' = b2 x - a2 y
// i.e. s' = A s + B x with A = [[-a1, 1], [-a2, 0]].  The clip is cut into 1024 contiguous runs of `run` samples (a multiple
// of SOS_SEG), one per thread.  Per section:
//   1. every run's zero-state end state e[j] (fused into the previous section's output sweep, or a read-only sweep for k = 0);
//   2. the carries S[0] = 0, S[j+1] = Phi S[j] + e[j], Phi = A^run (computed on the host in float64 by al_fx_sos), as a
//      Hillis-Steele scan over the 1024 runs with Phi^(2^l) squared on the fly: 10 levels;
//   3. every run re-filtered from its true entering state S[j]; the output is written, and the NEXT section's zero-state
//      end state is accumulated on it in the same sweep.
// So K sections cost K + 1 reads and K writes of the clip in one launch.  Coefficients and state are float64 throughout
// (float32 state misses the 1e-4 contract at low shelf frequencies: DESIGN.md "Filter FX"); input and output are float32.
// Global memory is staged through LDS in tiles of SOS_SEG samples per run, so a wave's loads and stores are 64-B segments
// instead of 64 scattered words; the LDS pitch is odd so that a thread's walk down its own segment is conflict-free.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "al_common.h"
#include "al_status.h"

namespace al {

constexpr int SOS_THREADS = 1024;   // runs (= threads of the one workgroup)
constexpr int SOS_SEG = 16;         // samples per run per staged tile
constexpr int SOS_PITCH = SOS_SEG + 1;

struct SosArgs {
  double c[AL_SOS_MAX_SECTIONS][5];    // b0 b1 b2 a1 a2, divided by a0
  double phi[AL_SOS_MAX_SECTIONS][4];  // A^run, row-major
  int32_t n_sections;
};

// samples per run: ceil(n / SOS_THREADS) rounded up to a whole number of tiles
__host__ __device__ inline int64_t sos_run_length(int64_t n) {
  const int64_t per = (n + SOS_THREADS - 1) / SOS_THREADS;
  return (per + SOS_SEG - 1) / SOS_SEG * SOS_SEG;
}

// One sweep over the clip.  Each thread filters its run through section `cur` from state (s1, s2), updating it in place.
// write: the output goes to `out`; nxt != nullptr: section `nxt` is run from zero state on that output, its end state left in
// (t1, t2).  Every thread takes the same number of barriers.
__device__ inline void sos_sweep(const float *in, float *out, int64_t n, int64_t run, const double *cur, double &s1,
                                 double &s2, const double *nxt, double &t1, double &t2, bool write, float *tile) {
  const int tid = threadIdx.x;
  const int64_t lo = (int64_t)tid * run;
  const int64_t tiles = ((run < n ? run : n) + SOS_SEG - 1) / SOS_SEG;
  const double b0 = cur[0], b1 = cur[1], b2 = cur[2], a1 = cur[3], a2 = cur[4];
  const bool fuse = nxt != nullptr;
  const double c0 = fuse ? nxt[0] : 0.0, c1 = fuse ? nxt[1] : 0.0, c2 = fuse ? nxt[2] : 0.0, d1 = fuse ? nxt[3] : 0.0,
               d2 = fuse ? nxt[4] : 0.0;
  for (int64_t c = 0; c < tiles; ++c) {
    for (int f = tid; f < SOS_THREADS * SOS_SEG; f += SOS_THREADS) {
      const int t = f / SOS_SEG, i = f - t * SOS_SEG;
      const int64_t pos = (int64_t)t * run + c * SOS_SEG + i;
      if (pos < n) tile[t * SOS_PITCH + i] = in[pos];
    }
    __syncthreads();
    const int64_t left = n - (lo + c * SOS_SEG);
    const int m = left <= 0 ? 0 : (left < SOS_SEG ? (int)left : SOS_SEG);
    float *mine = tile + tid * SOS_PITCH;
    for (int i = 0; i < m; ++i) {
      const double x = (double)mine[i];
      const double y = fma(b0, x, s1);
      s1 = fma(-a1, y, fma(b1, x, s2));
      s2 = fma(-a2, y, b2 * x);
      if (write) mine[i] = (float)y;
      if (fuse) {
        const double v = (double)(float)y;   // the next section filters what is stored
        const double z = fma(c0, v, t1);
        t1 = fma(-d1, z, fma(c1, v, t2));
        t2 = fma(-d2, z, c2 * v);
      }
    }
#ifndef AL_TEST_REVERT_SOS_BARRIER   // tests/shake.py `revert`: without it the copy-out below reads rows their owners still filter
    __syncthreads();
#endif
    if (write) {
      for (int f = tid; f < SOS_THREADS * SOS_SEG; f += SOS_THREADS) {
        const int t = f / SOS_SEG, i = f - t * SOS_SEG;
        const int64_t pos = (int64_t)t * run + c * SOS_SEG + i;
        if (pos < n) out[pos] = tile[t * SOS_PITCH + i];
      }
      __syncthreads();
    }
  }
}

// (e1, e2): this run's zero-state end state on entry, the state ENTERING this run on return.
__device__ inline void sos_carry(double &e1, double &e2, const double *phi, double *carry) {
  const int tid = threadIdx.x;
  double p00 = phi[0], p01 = phi[1], p10 = phi[2], p11 = phi[3];
  double w1 = e1, w2 = e2;
  for (int d = 1; d < SOS_THREADS; d <<= 1) {   // w[j] += Phi^d w[j - d]
    carry[2 * tid] = w1;
    carry[2 * tid + 1] = w2;
    __syncthreads();
    if (tid >= d) {
      const double v1 = carry[2 * (tid - d)], v2 = carry[2 * (tid - d) + 1];
      w1 = fma(p00, v1, fma(p01, v2, w1));
      w2 = fma(p10, v1, fma(p11, v2, w2));
    }
    __syncthreads();
    const double q00 = fma(p00, p00, p01 * p10), q01 = fma(p00, p01, p01 * p11);
    const double q10 = fma(p10, p00, p11 * p10), q11 = fma(p10, p01, p11 * p11);
    p00 = q00; p01 = q01; p10 = q10; p11 = q11;
  }
  carry[2 * tid] = w1;   // w[j] = state leaving run j
  carry[2 * tid + 1] = w2;
  __syncthreads();
  e1 = tid > 0 ? carry[2 * (tid - 1)] : 0.0;
  e2 = tid > 0 ? carry[2 * (tid - 1) + 1] : 0.0;
  __syncthreads();
}

// One clip's launch: what al_fx_sos derives from its arguments.  A batched launch (al_fx_batch_launch) reads one per workgroup
// from a table in device memory, a single-clip launch carries it by value.
struct SosJob {
  const float *src;
  float *dst;
  int64_t n, run;
  SosArgs a;
};

// {b0 b1 b2 a1 a2, Phi} per section into LDS.  Constant indices only: a job passed by value stays out of scratch.
__device__ __forceinline__ void sos_stage_coef(const SosArgs &a, double *coef) {
#pragma unroll
  for (int i = 0; i < AL_SOS_MAX_SECTIONS * 5; ++i) coef[i / 5 * 9 + i % 5] = a.c[i / 5][i % 5];
#pragma unroll
  for (int i = 0; i < AL_SOS_MAX_SECTIONS * 4; ++i) coef[i / 4 * 9 + 5 + i % 4] = a.phi[i / 4][i % 4];
}

// Workgroup b filters the clip of job b: table[b], or `one` when table == nullptr (grid of 1).  The same instantiation either
// way, so a batch renders the bits of the single-clip launches.  src may equal dst: every tile is read completely before any
// of it is written back.
__global__ __launch_bounds__(1024) void k_fx_sos(const SosJob *__restrict__ table, SosJob one) {
  __shared__ float tile[SOS_THREADS * SOS_PITCH];
  __shared__ double carry[2 * SOS_THREADS];
  __shared__ double coef[AL_SOS_MAX_SECTIONS * 9];   // {b0 b1 b2 a1 a2, Phi} per section
  const SosJob *job = table ? table + blockIdx.x : nullptr;
  const float *src = job ? job->src : one.src;
  float *dst = job ? job->dst : one.dst;
  const int64_t n = job ? job->n : one.n, run = job ? job->run : one.run;
  const int n_sections = job ? job->a.n_sections : one.a.n_sections;
  if (threadIdx.x == 0) {
    if (job) sos_stage_coef(job->a, coef);
    else sos_stage_coef(one.a, coef);
  }
  __syncthreads();
  double s1 = 0.0, s2 = 0.0, t1 = 0.0, t2 = 0.0;
  sos_sweep(src, dst, n, run, coef, s1, s2, nullptr, t1, t2, false, tile);   // zero-state end states of section 0
  for (int k = 0; k < n_sections; ++k) {
    sos_carry(s1, s2, coef + 9 * k + 5, carry);
    t1 = t2 = 0.0;
    sos_sweep(k == 0 ? src : dst, dst, n, run, coef + 9 * k, s1, s2, k + 1 < n_sections ? coef + 9 * (k + 1) : nullptr, t1,
              t2, true, tile);
    s1 = t1;
    s2 = t2;
  }
}

// ---- host side (al_fx_sos, al_fx_batch_pack): Phi = A^run in float64 by repeated squaring
inline void sos_transition_power(double a1, double a2, int64_t p, double out[4]) {
  double r[4] = {1.0, 0.0, 0.0, 1.0}, m[4] = {-a1, 1.0, -a2, 0.0};
  while (p > 0) {
    if (p & 1) {
      const double t[4] = {r[0] * m[0] + r[1] * m[2], r[0] * m[1] + r[1] * m[3], r[2] * m[0] + r[3] * m[2],
                           r[2] * m[1] + r[3] * m[3]};
      for (int i = 0; i < 4; ++i) r[i] = t[i];
    }
    const double t[4] = {m[0] * m[0] + m[1] * m[2], m[0] * m[1] + m[1] * m[3], m[2] * m[0] + m[3] * m[2],
                         m[2] * m[1] + m[3] * m[3]};
    for (int i = 0; i < 4; ++i) m[i] = t[i];
    p >>= 1;
  }
  for (int i = 0; i < 4; ++i) out[i] = r[i];
}

// 0 with *job filled (every section divided by its a0, with its Phi), or the error of the first bad argument
inline int sos_prepare(const al_fx_sos_job &in, SosJob *job) {
  if (!in.src || !in.dst || !in.sos) return fail(AL_E_BADARG, "al_fx_sos: null pointer");
  if (in.n < 1) return fail(AL_E_BADARG, "al_fx_sos: n must be >= 1");
  if (in.n_sections < 1 || in.n_sections > AL_SOS_MAX_SECTIONS)
    return fail(AL_E_BADARG, "al_fx_sos: n_sections must be in 1..AL_SOS_MAX_SECTIONS (16); split longer cascades");
  const int64_t run = sos_run_length(in.n);
  memset(job, 0, sizeof(*job));
  job->src = in.src;
  job->dst = in.dst;
  job->n = in.n;
  job->run = run;
  SosArgs &a = job->a;
  a.n_sections = in.n_sections;
  char msg[160];
  for (int k = 0; k < in.n_sections; ++k) {
    const double *row = in.sos + 6 * k;
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
    sos_transition_power(c[3], c[4], run, a.phi[k]);
  }
  return AL_OK;
}

}  // namespace al
