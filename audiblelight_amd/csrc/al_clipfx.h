// Sample-wise clip operations (A13/A14): the pointwise FX (gain, invert, reverse, fade, clip, tanh, bitcrush, pre-emphasis), the
// de-emphasis scan and the frame shuffle of the TimeWarp family.  FX with filter or delay state are in al_sos.h / al_delayfx.h.
#pragma once
#include <hip/hip_runtime.h>

#include "al_common.h"
#include "al_status.h"

namespace al {

// ------------------------------------------------------------------ sample-wise clip operations (A13/A14)
__device__ __forceinline__ float fade_in_curve(int shape, float r) {  // augmentation.py:1490-1508
  switch (shape) {
    case AL_FADE_EXPONENTIAL: return exp2f(r - 1.f) * r;
    case AL_FADE_LOGARITHMIC: return log10f(0.1f + r) + 1.f;
    case AL_FADE_QUARTER_SINE: return sinpif(0.5f * r);
    case AL_FADE_HALF_SINE: return 0.5f * sinpif(r - 0.5f) + 0.5f;
    default: return r;
  }
}
__device__ __forceinline__ float fade_out_curve(int shape, float r) {  // augmentation.py:1510-1528
  switch (shape) {
    case AL_FADE_EXPONENTIAL: return exp2f(-r) * (1.f - r);
    case AL_FADE_LOGARITHMIC: return log10f(1.1f - r) + 1.f;
    case AL_FADE_QUARTER_SINE: return sinpif(0.5f * r + 0.5f);
    case AL_FADE_HALF_SINE: return 0.5f * sinpif(r + 0.5f) + 0.5f;
    default: return 1.f - r;
  }
}

struct FxArgs {
  int op;
  float p0;
  int n_in, n_out, shape_in, shape_out;
};

__global__ __launch_bounds__(256) void k_fx_pointwise(const float *src, float *dst, int64_t n, FxArgs a) {
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
    float x = src[a.op == AL_FX_REVERSE ? n - 1 - t : t];
    switch (a.op) {
      case AL_FX_GAIN: x *= a.p0; break;
      case AL_FX_INVERT: x = -x; break;
      case AL_FX_CLIP: x = fminf(fmaxf(x, -a.p0), a.p0); break;
      case AL_FX_TANH: x = tanhf(a.p0 * x); break;
      case AL_FX_BITCRUSH: x = rintf(x * a.p0) / a.p0; break;
      case AL_FX_FADE: {
        float g = 1.f;
        if (a.n_in > 0 && a.shape_in != AL_FADE_NONE && t < a.n_in) {
          const float r = a.n_in > 1 ? (float)t / (float)(a.n_in - 1) : 0.f;  // np.linspace(0, 1, n_in)
          g *= fminf(fmaxf(fade_in_curve(a.shape_in, r), 0.f), 1.f);
        }
        if (a.n_out > 0 && a.shape_out != AL_FADE_NONE && t >= n - a.n_out) {
          const float r = a.n_out > 1 ? (float)(t - (n - a.n_out)) / (float)(a.n_out - 1) : 0.f;
          g *= fminf(fmaxf(fade_out_curve(a.shape_out, r), 0.f), 1.f);
        }
        x *= g;
      } break;
      case AL_FX_PREEMPH: {
        if (t == 0) x = x + (2.f * x - (n > 1 ? src[1] : x));
        else x = fmaf(-a.p0, src[t - 1], x);
      } break;
      default: break;
    }
    dst[t] = x;
  }
}

// y[n] = x[n] + c*y[n-1] minus the extrapolation correction: one workgroup, each thread owns a
// contiguous run; carries are chained by thread 0 (1024 runs), then folded back in.
struct DeemphJob {
  const float *src;
  float *dst;
  int64_t n;
  float c;
};

// Workgroup b takes job b: table[b] of a batched launch (al_fx_batch_launch), or `one` when table == nullptr (grid of 1); the
// same instantiation either way.
__global__ __launch_bounds__(1024) void k_fx_deemph(const DeemphJob *__restrict__ table, DeemphJob one) {
  __shared__ float tail[1024], decay[1024], carry[1024];
  const DeemphJob *job = table ? table + blockIdx.x : nullptr;
  const float *src = job ? job->src : one.src;
  float *dst = job ? job->dst : one.dst;
  const int64_t n = job ? job->n : one.n;
  const float c = job ? job->c : one.c;
  const int tid = threadIdx.x;
  const int64_t run = (n + 1023) / 1024;
  const int64_t lo = (int64_t)tid * run, hi = lo + run < n ? lo + run : n;
  float y = 0.f, d = 1.f;
  for (int64_t t = lo; t < hi; ++t) {
    y = fmaf(c, y, src[t]);
    d *= c;
    dst[t] = y;
  }
  tail[tid] = y;
  decay[tid] = d;
  __syncthreads();
  if (tid == 0) {
    float acc = 0.f;
    for (int i = 0; i < 1024; ++i) {
      carry[i] = acc;  // state entering run i
      acc = fmaf(decay[i], acc, tail[i]);
    }
  }
  __syncthreads();
  const float x0 = src[0], x1 = n > 1 ? src[1] : src[0];
  const float corr = ((2.f - c) * x0 - x1) / (3.f - c);
  float pw = c;                      // c^(t - lo + 1)
  float cn = powf(c, (float)lo);     // c^t
  const float cin = carry[tid];
  for (int64_t t = lo; t < hi; ++t) {
    dst[t] = fmaf(cin, pw, dst[t]) - corr * cn;
    pw *= c;
    cn *= c;
  }
}

// ---- host side: al_fx_apply's checks of its clip arguments, and the de-emphasis job of a clip that passes them
inline int fx_apply_check(int op, const float *src, const float *dst, int64_t n) {
  if (!src || !dst || n <= 0) return fail(AL_E_BADARG, "bad fx arguments");
  if (op < AL_FX_GAIN || op > AL_FX_DEEMPH) return fail(AL_E_UNSUPPORTED, "unknown fx op");
  const bool out_of_place = (op == AL_FX_REVERSE || op == AL_FX_PREEMPH || op == AL_FX_DEEMPH);
  if (out_of_place && src == dst) return fail(AL_E_BADARG, "this fx op needs dst != src");
  if ((op == AL_FX_PREEMPH || op == AL_FX_DEEMPH) && n < 2) return fail(AL_E_BADARG, "emphasis filters need n >= 2");
  return AL_OK;
}

inline int deemph_prepare(const al_fx_deemph_job &in, DeemphJob *job) {
  if (int rc = fx_apply_check(AL_FX_DEEMPH, in.src, in.dst, in.n)) return rc;
  *job = DeemphJob{in.src, in.dst, in.n, in.coef};
  return AL_OK;
}

__global__ __launch_bounds__(256) void k_frame_shuffle(const float *src, float *dst, int64_t n, int frame_len,
                                                       int row_len, const int32_t *rows, int n_rows) {
  const int64_t total = (int64_t)n_rows * row_len;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
    const int64_t u = t % total;
    const int q = (int)(u / row_len), j = (int)(u - (int64_t)q * row_len);
    const int r = rows[2 * q], mode = rows[2 * q + 1];
    const int jj = mode == 2 ? row_len - 1 - j : j;
    dst[t] = mode == 1 ? 0.f : src[r + (int64_t)frame_len * jj];
  }
}

}  // namespace al
