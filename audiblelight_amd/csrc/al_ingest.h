// What prepares a render's inputs and carries its output away: the twiddle table, IR packing (dense and ragged), polyphase
// resampling, the wrap copy of a tiled clip and the encoding of a scene into interleaved frames.  Format and layout conversions
// with no arithmetic on the audio beyond rounding belong here.
#pragma once
#include <hip/hip_runtime.h>

#include "al_common.h"

namespace al {

// ------------------------------------------------------------------ twiddle table
__global__ void k_twiddle_init(float2 *tw, int m) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < m) {
    double s, c;
    sincospi(-(double)k / (double)m, &s, &c);
    tw[k] = make_float2((float)c, (float)s);
  }
}

template <class T>
__global__ __launch_bounds__(256) void k_pack_irs(const T *src, float *dst, int len, int pitch) {
  const T *row = src + (int64_t)blockIdx.x * len;   // one workgroup per row: rows = C*N may exceed grid.y's 65535
  float *out = dst + (int64_t)blockIdx.x * pitch;
  for (int t = threadIdx.x; t < pitch; t += 256) out[t] = t < len ? (float)row[t] : 0.f;
}

// Ragged IRs (one 1-D array per (capsule, source), worldstate.py:2196-2253) -> zero-padded float32 rows of `pitch`.
template <class T>
__global__ __launch_bounds__(256) void k_pack_ragged(const T *__restrict__ src, const int64_t *__restrict__ offsets,
                                                     const int32_t *__restrict__ lens, float *__restrict__ dst, int pitch) {
  const int64_t row = blockIdx.x;
  const T *in = src + offsets[row];
  const int n = lens[row];
  float *out = dst + row * pitch;
  for (int t = threadIdx.x; t < pitch; t += 256) out[t] = t < n ? (float)in[t] : 0.f;
}

// Polyphase FIR resampling by up/down (scipy.signal.resample_poly semantics: zero-stuff by `up`, filter with h of
// 2*half+1 taps already scaled by `up`, keep every `down`-th sample): out[m] = sum_j x[j] * h[m*down - j*up + half].
__global__ __launch_bounds__(256) void k_resample_poly(const float *__restrict__ x, int64_t n_in, const float *__restrict__ h,
                                                       int half, int up, int down, float *__restrict__ out, int64_t n_out,
                                                       int64_t out_pitch) {
  const float *row = x + (int64_t)blockIdx.y * n_in;
  float *dst = out + (int64_t)blockIdx.y * out_pitch;
  for (int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x; m < out_pitch; m += (int64_t)gridDim.x * 256) {
    float acc = 0.f;
    if (m < n_out) {
      const int64_t c = m * down;  // position on the up-sampled grid
      // taps with 0 <= c - j*up + half <= 2*half  <=>  (c - half)/up <= j <= (c + half)/up
      int64_t j_lo = (c - half + up - 1) / up, j_hi = (c + half) / up;
      if (c - half < 0) j_lo = 0;
      if (j_hi > n_in - 1) j_hi = n_in - 1;
      for (int64_t j = j_lo; j <= j_hi; ++j) acc = fmaf(row[j], h[c - j * up + half], acc);
    }
    dst[m] = acc;
  }
}

// float -> PCM_16 as python-soundfile writes it: it enables SFC_SET_CLIPPING on every file it opens, so libsndfile converts
// with f2s_clip_array: scaled = x * 0x8000 (float); >= 0x7FFF -> 0x7FFF, <= -0x8000 -> -0x8000, else lrintf(scaled)
// (round half to even).  (Without clipping libsndfile scales by 0x7FFF instead; round 2 encoded that.)  soundfile is not in
// the build container, so this follows libsndfile's source, not a golden file: parity unpinned by definition.
__device__ __forceinline__ int16_t pcm16_of(float x) {
  const float scaled = x * 32768.0f;
  if (scaled >= 32767.0f) return (int16_t)32767;
  if (scaled <= -32768.0f) return (int16_t)-32768;
  return (int16_t)rintf(scaled);   // NaN never reaches here: non-finite scenes are refused before encoding
}

// (C, T) float32 scene -> (T, C) interleaved frames, the layout soundfile.write(audio.T) puts on disk (core.py:1840-1847).
// One workgroup per tile of 32 capsules x 64 samples through LDS: reads run along t, writes along c.
template <bool PCM16>
__global__ __launch_bounds__(256) void k_encode_frames(const float *__restrict__ scene, int n_capsules, int64_t n_samples,
                                                       void *__restrict__ out) {
  __shared__ float tile[32][65];
  const int64_t t0 = (int64_t)blockIdx.x * 64;
  const int c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < 32; r += 4) {
    const int c = c0 + r + ty;
    tile[r + ty][tx] = (c < n_capsules && t0 + tx < n_samples) ? scene[(int64_t)c * n_samples + t0 + tx] : 0.f;
  }
  __syncthreads();
  // 16 bytes per store where the capsule count allows it (the destination may be page-locked HOST memory: every store
  // is then a PCIe write, and 2- or 4-byte stores make 64 / 128-byte packets)
  if (PCM16 && (n_capsules & 7) == 0) {
    const int tl = threadIdx.x >> 2, cg = (threadIdx.x & 3) * 8;   // one frame's 8 consecutive capsules
    const int64_t t = t0 + tl;
    if (t < n_samples && c0 + cg < n_capsules) {
      int16_t q[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) q[i] = pcm16_of(tile[cg + i][tl]);
      struct alignas(16) Frames8 { uint32_t w[4]; } v;
#pragma unroll
      for (int i = 0; i < 4; ++i) v.w[i] = (uint32_t)(uint16_t)q[2 * i] | ((uint32_t)(uint16_t)q[2 * i + 1] << 16);
      *reinterpret_cast<Frames8 *>(reinterpret_cast<int16_t *>(out) + t * n_capsules + c0 + cg) = v;
    }
    return;
  }
  if (!PCM16 && (n_capsules & 3) == 0) {
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int j = threadIdx.x + 256 * pass, tl = j >> 3, cg = (j & 7) * 4;   // one frame's 4 consecutive capsules
      const int64_t t = t0 + tl;
      if (t < n_samples && c0 + cg < n_capsules)
        *reinterpret_cast<float4 *>(reinterpret_cast<float *>(out) + t * n_capsules + c0 + cg) =
            make_float4(tile[cg][tl], tile[cg + 1][tl], tile[cg + 2][tl], tile[cg + 3][tl]);
    }
    return;
  }
  const int cl = threadIdx.x & 31, tl = threadIdx.x >> 5;
#pragma unroll
  for (int tt = 0; tt < 64; tt += 8) {
    const int64_t t = t0 + tt + tl;
    const int c = c0 + cl;
    if (c < n_capsules && t < n_samples) {
      const float x = tile[cl][tt + tl];
      if (PCM16) {
        reinterpret_cast<int16_t *>(out)[t * n_capsules + c] = pcm16_of(x);
      } else {
        reinterpret_cast<float *>(out)[t * n_capsules + c] = x;
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_wrap_copy(const float *src, int64_t m, float *dst, int64_t n) {
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) dst[t] = src[t % m];
}

}  // namespace al
