// Level scalars of a render, one value per emitter, event or clip, reduced on the device in float64: emitter gains
// (normalize_irs), event levels (apply_snr o db_to_multiplier) and clip scales (peak normalisation with the folded FX scalars).
// A kernel belongs here when it turns statistics into a multiplier; the kernels that apply one to samples are in al_rows.h.
#pragma once
#include <hip/hip_runtime.h>

#include "al_common.h"

namespace al {

// ------------------------------------------------------------------ 2. emitter gains (normalize_irs)
// one wave per emitter: g = 1 / mean_c( sqrt(sum_t h^2) + tiny(float64) )   (synthesize.py:425-428)
// mode 0: g (single GPU); 1: emitter_gain[n] := sum over THIS rank's capsules of the norms (to be all-reduced);
// 2: emitter_gain[n] := total_capsules / emitter_gain[n] (the reduced sum), for capsule-sharded scenes
// An IR whose gain would not fit float32 (mean norm below 3e-39: every capsule's IR all zeros, or float32 denormals) gets gain 0:
// the reference divides its zeros by tiny and keeps zeros; a saturated gain would overflow the signal spectra it multiplies.
__device__ __forceinline__ float emitter_gain_of(double capsules, double norm_sum) {
  const double g = capsules / norm_sum;
  return (g <= 3.4028234663852886e38 || g != g) ? (float)g : 0.0f;   // NaN (a NaN in the IR) stays NaN and fails the finite check
}

__global__ __launch_bounds__(64) void k_emitter_gains(al_batch b, int mode, int total_capsules) {
  const int n = b.emitter0 + blockIdx.x, lane = threadIdx.x;
  if (mode == 2) {
    if (lane == 0)
      b.emitter_gain[n] = (b.flags & AL_FLAG_NO_IR_NORM) ? 1.0f : emitter_gain_of((double)total_capsules, (double)b.emitter_gain[n]);
    return;
  }
  double acc = 0.0;
  for (int c = lane; c < b.n_capsules; c += 64) {
    const float *e = b.ir_energy + ((int64_t)n * b.n_capsules + c) * b.n_partitions;
    double sum = 0.0;
    for (int p = 0; p < b.n_partitions; ++p) sum += (double)e[p];
    acc += sqrt(sum) + 2.2250738585072014e-308;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (lane == 0) {
    if (mode == 1) b.emitter_gain[n] = (float)acc;
    else b.emitter_gain[n] = (b.flags & AL_FLAG_NO_IR_NORM) ? 1.0f : emitter_gain_of((double)b.n_capsules, acc);
  }
}

// ------------------------------------------------------------------ 6. event levels
// Composite of apply_snr (synthesize.py:40-49) and db_to_multiplier (synthesize.py:52-68) as chained
// at synthesize.py:594-599, evaluated in float64 from the deterministic partial statistics.
// mode 0: reduce + law (single GPU); 1: reduce only; 2: law only, from event_stats, with `total_capsules` rows
__global__ __launch_bounds__(64) void k_event_levels(al_batch b, int mode, int total_capsules) {
  const int e = b.event0 + blockIdx.x;
  const al_event ev = b.events[e];
  const int lane = threadIdx.x;
  double *o = b.event_stats + 4 * (int64_t)e;
  double sum = 0.0, bad = 0.0;
  float mx = 0.f;
  if (mode != 2) {
    const int n = b.n_capsules * ev.n_blocks;
    const float *pp = b.partials + 4 * (int64_t)ev.part_base;
    for (int i = lane; i < n; i += 64) {
      sum += (double)pp[4 * i];
      mx = fmaxf(mx, pp[4 * i + 1]);
      bad += (double)pp[4 * i + 2];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      sum += __shfl_down(sum, off, 64);
      mx = fmaxf(mx, __shfl_down(mx, off, 64));
      bad += __shfl_down(bad, off, 64);
    }
  }
  if (lane == 0) {
    if (mode == 2) {
      sum = o[0];
      mx = (float)o[1];
      bad = o[2];
    }
    if (mode == 1) {
      o[0] = sum;
      o[1] = (double)mx;
      o[2] = bad;
      o[3] = 0.0;
      return;
    }
    const double rows = mode == 2 ? (double)total_capsules : (double)b.n_capsules;
    const double snr = (double)ev.snr;
    const double peak = fmax((double)mx, 1e-15);
    const double s1 = snr / peak;                                   // apply_snr
    const double mean_abs = fabs(s1) * sum / (rows * (double)ev.len);
    const double s2 = pow(10.0, ((double)ev.ref_db + snr) / 20.0) / (mean_abs + 2.2250738585072014e-308);
    o[0] = sum;
    o[1] = (double)mx;
    o[2] = bad;
    o[3] = s2;
    // a silent render (sum|x| = 0: zero clip or zero IRs) has s2 = 10^(dB/20) / tiny: the reference multiplies its zeros by it
    b.event_scale[e] = finite_f32(s1 * s2);
  }
}

// ------------------------------------------------------------------ clip scales (A13 peak normalisation, folded FX scalars)
// scale = s / (|s| * max|x| + tiny(float32)): peak normalisation `a / max(|a| + tiny)` (event.py:535-536) of the clip
// s * x, where s is the product of the scalar FX in front of it (Gain, Invert); one workgroup per clip.
__device__ __forceinline__ float peak_scale_of(const float *__restrict__ x, int64_t n, float s, float *red) {
  float mx = 0.f, z0 = 0.f, z1 = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += 1024) mx = fmaxf(mx, fabsf(x[i]));
  block_reduce3(z0, mx, z1, red, threadIdx.x, 1024);
  return finite_f32((double)s / ((double)fabsf(s) * (double)mx + 1.17549435e-38));   // a silent clip under a gain of +12 dB or more: finite
}

// mode[e] 0: clip_scale[e] = prescale[e]; 1: the peak-normalising scale of clip e (events table gives offset / length)
__global__ __launch_bounds__(1024) void k_clip_scales(al_batch b, const float *__restrict__ prescale,
                                                      const int32_t *__restrict__ mode, float *__restrict__ out) {
  __shared__ float red[48];
  const int e = b.event0 + blockIdx.x;
  const al_event ev = b.events[e];
  const float s = prescale[e];
  if (mode[e] == 0) {
    if (threadIdx.x == 0) out[e] = s;
    return;
  }
  const float v = peak_scale_of(b.audio + ev.audio_off, ev.len, s, red);
  if (threadIdx.x == 0) out[e] = v;
}

__global__ __launch_bounds__(1024) void k_peak_scale(const float *__restrict__ x, int64_t n, float s, float *__restrict__ out) {
  __shared__ float red[48];
  const float v = peak_scale_of(x, n, s, red);
  if (threadIdx.x == 0) *out = v;
}

}  // namespace al
