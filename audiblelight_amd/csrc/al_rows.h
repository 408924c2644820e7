// Row-wise helpers over plain (rows, cols) float32 buffers: scaling by a device scalar, axpy, per-row statistics and the
// ambience multipliers made from them.  Streaming kernels with no knowledge of events or spectra belong here.
#pragma once
#include <hip/hip_runtime.h>

#include "al_common.h"

namespace al {

__global__ __launch_bounds__(256) void k_scale(float *x, int64_t n, const float *scale) {
  const float s = *scale;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) x[i] *= s;
}

__global__ __launch_bounds__(256) void k_scale_d(float *x, int64_t n, const double *scale) {
  const float s = finite_f32(*scale);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) x[i] *= s;
}

__global__ __launch_bounds__(256) void k_axpy(float *y, const float *x, const float *a, int64_t n) {
  const float s = *a;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    y[i] = fmaf(s, x[i], y[i]);
}

// y[r, :] += a[r] * x[r, :]: an ambience with its per-channel scale (second and further ambiences of a scene)
__global__ __launch_bounds__(256) void k_axpy_rows(float *y, const float *x, const float *a, int64_t cols) {
  const float s = a[blockIdx.y];
  const int64_t base = (int64_t)blockIdx.y * cols;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cols; i += (int64_t)gridDim.x * 256)
    y[base + i] = fmaf(s, x[base + i], y[base + i]);
}

// Per-channel multiplier of an ambience from its row statistics {sum|x|, max|x|, ...} (al_row_stats), one wave, float64:
// the per-channel peak normalisation ch / max(|ch| + tiny) (ambience.py:211-214) and db_to_multiplier(ref_db, mean|normalised|)
// (synthesize.py:350-356) as ONE scalar per channel, so the noise is neither rescaled in place nor read by the host.
__global__ __launch_bounds__(64) void k_ambience_scales(const double *__restrict__ stats, int rows, int64_t cols, float ref_db,
                                                        int normalize, float *__restrict__ scales) {
  const int lane = threadIdx.x;
  double acc = 0.0;
  for (int c = lane; c < rows; c += 64) {
    const double inv = normalize ? 1.0 / (stats[4 * c + 1] + 2.2250738585072014e-308) : 1.0;
    acc += stats[4 * c] * inv;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  __shared__ double total;
  if (lane == 0) total = acc;
  __syncthreads();
  const double mean_abs = total / ((double)rows * (double)cols);
  const double mult = pow(10.0, (double)ref_db / 20.0) / (mean_abs + 2.2250738585072014e-308);
  for (int c = lane; c < rows; c += 64) {
    const double inv = normalize ? 1.0 / (stats[4 * c + 1] + 2.2250738585072014e-308) : 1.0;
    scales[c] = finite_f32(normalize == 2 ? inv : mult * inv);   // 2: the peak normalisation alone; a silent channel stays silent
  }
}

constexpr int ROW_CHUNK = 16384;  // samples per partial of k_row_stats

__global__ __launch_bounds__(256) void k_row_stats(const float *x, int64_t cols, float *partials) {
  __shared__ float red[48];
  const int nchunks = (int)((cols + ROW_CHUNK - 1) / ROW_CHUNK);
  const int chunk = blockIdx.x % nchunks, r = blockIdx.x / nchunks;  // rows may exceed the 65535 limit of grid.y
  const int64_t lo = (int64_t)chunk * ROW_CHUNK, hi = lo + ROW_CHUNK < cols ? lo + ROW_CHUNK : cols;
  const float *row = x + (int64_t)r * cols;
  float asum = 0.f, amax = 0.f, bad = 0.f, sq = 0.f;
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
    const float v = row[i];
    asum += fabsf(v);
    amax = fmaxf(amax, fabsf(v));
    bad += isfinite(v) ? 0.f : 1.f;
    sq = fmaf(v, v, sq);
  }
  block_reduce3(asum, amax, bad, red, threadIdx.x, 256);
  __syncthreads();
  float z0 = 0.f, z1 = 0.f;
  block_reduce3(sq, z0, z1, red, threadIdx.x, 256);
  if (threadIdx.x == 0) {
    float *pp = partials + 4 * ((int64_t)r * nchunks + chunk);
    pp[0] = asum;
    pp[1] = amax;
    pp[2] = bad;
    pp[3] = sq;
  }
}

__global__ __launch_bounds__(64) void k_row_stats_final(const float *partials, int nchunks, double *out) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const float *pp = partials + 4 * (int64_t)r * nchunks;
  double sum = 0.0, bad = 0.0, sq = 0.0;
  float mx = 0.f;
  for (int i = lane; i < nchunks; i += 64) {
    sum += (double)pp[4 * i];
    mx = fmaxf(mx, pp[4 * i + 1]);
    bad += (double)pp[4 * i + 2];
    sq += (double)pp[4 * i + 3];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    sum += __shfl_down(sum, off, 64);
    mx = fmaxf(mx, __shfl_down(mx, off, 64));
    bad += __shfl_down(bad, off, 64);
    sq += __shfl_down(sq, off, 64);
  }
  if (lane == 0) {
    out[4 * r + 0] = sum;
    out[4 * r + 1] = (double)mx;
    out[4 * r + 2] = bad;
    out[4 * r + 3] = sq;
  }
}

__global__ __launch_bounds__(256) void k_scale_matrix_rows(float *x, int64_t cols, const float *scale) {
  const float s = scale[blockIdx.y];
  float *row = x + (int64_t)blockIdx.y * cols;  // rows = channels of an ambience: far below grid.y's limit
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cols; i += (int64_t)gridDim.x * 256) row[i] *= s;
}

}  // namespace al
