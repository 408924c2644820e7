// The scene mixdown (generate_scene_audio_from_events): every event's scaled spatial audio, and optionally the ambience, added
// into the (C, T) scene buffer in one pass.  Kernels that write the scene from event audio belong here.
#pragma once
#include <hip/hip_runtime.h>

#include "al_common.h"

namespace al {

// ------------------------------------------------------------------ 7. mixdown
// One workgroup per (capsule, tile of m.tile = 4096 samples).  A thread owns 4 runs of 4 consecutive
// samples (16 accumulators); events that overlap the tile are walked in insertion order with their slot
// scalars in SGPRs, each adding scale * x with dword-aligned 16-byte loads (an event starts at an
// arbitrary sample, so its rows are not 16-byte aligned against the scene).
struct __attribute__((packed, aligned(4))) f4u {
  float x, y, z, w;
};

__global__ __launch_bounds__(256) void k_mixdown(al_mix m) {
  const int tile = blockIdx.x, c = blockIdx.y;
  const int lo = m.tile_ptr[tile], hi = m.tile_ptr[tile + 1];
  const int t_begin = tile * m.tile;
  float *row = m.scene + (int64_t)c * m.n_samples;
  constexpr int RUNS = 4;                       // m.tile == 4 * 256 * RUNS
  float4 acc[RUNS];
  const bool whole = (t_begin + m.tile <= m.n_samples) && ((m.n_samples & 3) == 0);  // workgroup-uniform
  const float amb_scale = m.ambience ? m.ambience_scale[c] : 0.f;   // per capsule: peak normalisation x noise-floor multiplier
  const float *amb = m.ambience ? m.ambience + (int64_t)c * m.n_samples : row;
#pragma unroll
  for (int r = 0; r < RUNS; ++r) {
    const int t = t_begin + 4 * (threadIdx.x + 256 * r);
    acc[r] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (m.ambience) {   // the reference adds the ambience to the zeroed float32 buffer first (synthesize.py:335-356)
      if (whole) {
        const float4 nz = *reinterpret_cast<const float4 *>(amb + t);
        acc[r] = make_float4(amb_scale * nz.x, amb_scale * nz.y, amb_scale * nz.z, amb_scale * nz.w);
      } else {
        if (t < m.n_samples) acc[r].x = amb_scale * amb[t];
        if (t + 1 < m.n_samples) acc[r].y = amb_scale * amb[t + 1];
        if (t + 2 < m.n_samples) acc[r].z = amb_scale * amb[t + 2];
        if (t + 3 < m.n_samples) acc[r].w = amb_scale * amb[t + 3];
      }
    }
    if (m.accumulate) {
      if (whole) {
        acc[r] = *reinterpret_cast<const float4 *>(row + t);
      } else {
        if (t < m.n_samples) acc[r].x = row[t];
        if (t + 1 < m.n_samples) acc[r].y = row[t + 1];
        if (t + 2 < m.n_samples) acc[r].z = row[t + 2];
        if (t + 3 < m.n_samples) acc[r].w = row[t + 3];
      }
    }
  }
  for (int q = lo; q < hi; ++q) {
    const int sl = m.tile_events[q];
    if (c >= m.slot_rows[sl]) continue;
    const int start = m.slot_start[sl], count = m.slot_count[sl];
    const float scale = m.event_scale[m.slot_event[sl]];
    const float *x = m.spatial + m.slot_src[sl] + (int64_t)c * m.slot_len[sl];
#pragma unroll
    for (int r = 0; r < RUNS; ++r) {
      const int rel = t_begin + 4 * (threadIdx.x + 256 * r) - start;
      if (rel >= 0 && rel + 3 < count) {
        const f4u v = *reinterpret_cast<const f4u *>(x + rel);
        acc[r].x = fmaf(scale, v.x, acc[r].x);
        acc[r].y = fmaf(scale, v.y, acc[r].y);
        acc[r].z = fmaf(scale, v.z, acc[r].z);
        acc[r].w = fmaf(scale, v.w, acc[r].w);
      } else if (rel > -4 && rel < count) {  // run straddles the start or the end of the slot
        if (rel >= 0 && rel < count) acc[r].x = fmaf(scale, x[rel], acc[r].x);
        if (rel + 1 >= 0 && rel + 1 < count) acc[r].y = fmaf(scale, x[rel + 1], acc[r].y);
        if (rel + 2 >= 0 && rel + 2 < count) acc[r].z = fmaf(scale, x[rel + 2], acc[r].z);
        if (rel + 3 >= 0 && rel + 3 < count) acc[r].w = fmaf(scale, x[rel + 3], acc[r].w);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < RUNS; ++r) {
    const int t = t_begin + 4 * (threadIdx.x + 256 * r);
    if (whole) {
      stream_store<64>(reinterpret_cast<float4 *>(row + t), acc[r]);
    } else {
      if (t < m.n_samples) row[t] = acc[r].x;
      if (t + 1 < m.n_samples) row[t + 1] = acc[r].y;
      if (t + 2 < m.n_samples) row[t + 2] = acc[r].z;
      if (t + 3 < m.n_samples) row[t + 3] = acc[r].w;
    }
  }
}

}  // namespace al
