// Shoebox room impulse responses at CAPSULES ON A RIGID SPHERE (al_ism_shoebox_sphere; DESIGN.md "Shoebox IRs: rigid-sphere
// receivers"): an Eigenmike-like array, or the two ears of a spherical head.  The sphere has centre o and radius a > 0, capsule c the
// unit direction n_c in room axes.  Images are taken relative to the CENTRE (R = image - o, d = |R|, u = R / d, tau = d fs / c) and
// each reaches the sphere as a plane wave from u; its pressure at the capsule is a Legendre series in mu = clamp(n_c . u, -1, 1):
//   P_0 = 1, P_1 = mu, P_{l+1} = ((2 l + 1) mu P_l - l P_{l-1}) / (l + 1)        float64, in exactly this order,
//   y_l[s] = sum_images A P_l(mu) tap(s - tau)    at every integer s in [-half, y_end + half), l = 0 .. n_orders - 1,
//   y(t)   = sum_l sum_{j = -half .. half} b_l[j] y_l[t - j]                     float64, l ascending, then j ascending,
// rounded to float32 once, with A the amplitude of al_ism.h (walls, source pattern, air) and b_l the radial FIR of order l
// (shoebox.sphere_filters: the table is the definition the kernels are handed; the radius lives in it and nowhere else).  A capsule
// row is thus a "band" row of al_ism_bands.h whose bands are Legendre orders: order l has one gain per image and one FIR.
//   k_ism_sphere<NB, SRC>  ism_gather (al_ism.h) over the shifted axis with the variant IsmSphere<NB>: a list entry carries the
//     gains P_l(mu) of the NB <= 4 orders [order0, order0 + NB) (the recurrence runs from 0 to the group's top order for every
//     image; the walls' one bit says which images are dead), one workgroup of ONE WAVE per (pair, tile of W), float64 order rows
//     written into the workspace [pair in pass][n_orders][W] by ism_workspace_rows, the body of k_ism_bands; ceil(n_orders / 4)
//     launches per pass (ism_rows_passes).  Every order keeps its own accumulator and the canonical order of the images, so the grouping cannot change bits.
//     The receiver position of the gather is the centre for every capsule: the kernel puts it into LDS and hands the gather a job
//     whose one "capsule" is that LDS triple.  SRC: the source's pattern and the air in the common amplitude, as IsmOmniSrc.
//   k_ism_band_combine<false> (al_ism_bands.h, as it is)  the rows without a tail: it indexes by n_bands alone, here n_orders.
//   k_ism_sphere_combine  the tiles below the split of a row with a tail: k_ism_band_combine<true>'s structure over the n_orders
//     rows, with ONE noise FIR in place of one per band: n(t) = ((1 - p) e_k + p e_{k+1}) sum_j psi_d[j] g(t - j), psi_d the
//     diffuse-field filter (shoebox.sphere_diffuse_filter), e the source's knots (ln_env (N, n_knots): the omni law).
//   k_ism_band_tail<HCAP> (al_ism_bands.h, as it is)  every sample at or past the split, launched with one band whose filter is
//     psi_d and a knot table per source.
// One wave per workgroup everywhere: the __syncthreads() order LDS traffic only, no barrier instruction, no atomics, no scratch.
#pragma once
#include "al_ism_bands.h"

namespace al {

constexpr int ISM_SPHERE_MAX_ORDERS = 64;
constexpr int ISM_SPHERE_MAX_HALF = ISM_BAND_TAIL_MAX_HALF;   // 1024, with and without a tail

struct IsmSphereJob {
  IsmBandJob bj;              // n_bands: the orders; band0: the first order of a launch of k_ism_sphere; filters: b (n_orders, 2 half + 1)
  const double *directions;   // (C, 3) unit vectors, device
  const double *diffuse;      // psi_d (2 half + 1), device; read with a tail only
  double centre[3];
};

// the sphere variant: P_l(mu) of the NB orders [order0, order0 + NB) beside the image seen from the centre
template <int NB>
struct IsmSphere : IsmWalls {
  static constexpr int NG = NB, LIST = ISM_DIR_LIST;
  using Entry = IsmDirEntry<NB>;
  const double *dir;   // the capsule's direction; uniform over the wave
  int order0;
  __device__ __forceinline__ void gains(Entry &e, const IsmImage &im) const {
    const double ux = im.Rx / im.d, uy = im.Ry / im.d, uz = im.Rz / im.d;   // the direction the plane wave arrives from
    double mu = dir[0] * ux + dir[1] * uy + dir[2] * uz;
    mu = mu < -1.0 ? -1.0 : mu > 1.0 ? 1.0 : mu;
    double below = 1.0, p = mu;   // P_{l-1}, P_l at l = 1
    if (order0 == 0) e.gain[0] = 1.0;
    const int top = order0 + NB - 1;
    for (int l = 1; l <= top; ++l) {
      if (l >= order0) e.gain[l - order0] = p;   // the list is LDS: an indexed store, no register array
      const double next = ((double)(2 * l + 1) * mu * p - (double)l * below) / (double)(l + 1);
      below = p;
      p = next;
    }
  }
  __device__ __forceinline__ void fill(Entry &e, const IsmImage &im) const {
    gains(e, im);   // to the list before the common part is formed: neither is live while the other is computed
    ism_park();
    ism_fill_shape(e, im, amplitude(im));
  }
};

// IsmSphere with a source pattern and air
template <int NB>
struct IsmSphereSrc : IsmSphere<NB> {
  using Entry = IsmDirEntry<NB>;
  IsmSource src;
  __device__ __forceinline__ void fill(Entry &e, const IsmImage &im) const {
    this->gains(e, im);
    e.a = src.gain(im);   // parked in the list and read back below: not live while the wall gain's exp is evaluated
    ism_park();
    ism_fill_shape(e, im, ism_air_amplitude(this->job, im) * e.a);
  }
};

// (waves per SIMD: asked for four, NB = 3 comes down from 130 VGPRs to 128 without scratch; NB = 4 (134 and 138 VGPRs, three waves)
// spills 16 and 40 bytes per lane to scratch when asked, so it is left at the default.)
template <int NB, bool SRC>
__global__ __launch_bounds__(ISM_THREADS) ISM_WAVES_PER_SIMD(NB == 3 ? 4 : 1) void k_ism_sphere(IsmSphereJob sj) {
  __shared__ double centre[3];
  const IsmBandJob &bj = sj.bj;
  int n, cap;
  ism_pass_pair(bj, bj.n_ws_tiles, n, cap);
  if (threadIdx.x < 3) centre[threadIdx.x] = sj.centre[threadIdx.x];
  __syncthreads();   // one wave: orders the LDS traffic
  IsmJob job = bj.base;   // uniform over the wave: scalar values, no vector register and no scratch holds the copy (hipcc parks
                          // 83 to 101 of the kernel's scalars in VGPR lanes, as it parks 60 to 76 in k_ism_bands<4>)
  job.capsules = centre;  // the gather's receiver 0 is the centre of the sphere, whatever the capsule
  const double *dir = sj.directions + 3 * (int64_t)cap;
  if constexpr (SRC)
    ism_workspace_rows(bj, job, IsmSphereSrc<NB>{{{job}, dir, bj.band0}, ism_source(job, n)}, n, 0);
  else
    ism_workspace_rows(bj, job, IsmSphere<NB>{{job}, dir, bj.band0}, n, 0);
}

// out[t] = float32(w_e sum_l sum_j b_l[j] y_l[t - j] + w_l n(t)) for the tiles below the split of a row with a tail; grid, lanes and
// LDS as k_ism_band_combine.  Pass b < n_orders stages order row b and its FIR; the pass after the last one (tiles with a sample past
// M only) stages the draws and psi_d.
__global__ __launch_bounds__(ISM_THREADS) void k_ism_sphere_combine(IsmSphereJob sj) {
  __shared__ double seg[2 * ISM_BAND_CHUNK], tap[ISM_BAND_CHUNK];
  const IsmBandJob &bj = sj.bj;
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
  const bool noisy = (int64_t)t_lo + ISM_TILE - 1 > job.tail.mix;   // does a sample of this tile carry noise?  (uniform)
  const int n_taps = 2 * bj.half + 1;
  double acc[ISM_PER_LANE] = {}, acc_g[ISM_PER_LANE] = {};   // the image part; sum_j psi_d[j] g(t - j)
  for (int b = 0; b < bj.n_bands + (noisy ? 1 : 0); ++b) {
    const bool draws = b == bj.n_bands;   // uniform
    const double *y = bj.workspace + (local * bj.n_bands + (draws ? 0 : b)) * (int64_t)bj.W;
    const double *phi = draws ? sj.diffuse : bj.filters + (int64_t)b * n_taps;
    for (int c0 = 0; c0 < n_taps; c0 += ISM_BAND_CHUNK) {
      // taps j = -half + c0 + i, i < ISM_BAND_CHUNK: output t_lo + o reads word t - j + half = first + (ISM_BAND_CHUNK - 1) + o - i
      const int first = t_lo + 2 * bj.half - c0 - (ISM_BAND_CHUNK - 1);
      __syncthreads();   // the reads of the chunk before are over
      for (int k = tid; k < 2 * ISM_BAND_CHUNK - 1; k += ISM_THREADS) {
        const int idx = first + k;   // below 0 only under taps past the last one, at or past W only under outputs past y_end
        if (draws)
          seg[k] = (double)ism_band_draw(job, idx - bj.half, n, cap);   // word idx holds sample idx - half
        else
          seg[k] = idx >= 0 && idx < bj.W ? y[idx] : 0.0;
      }
      for (int k = tid; k < ISM_BAND_CHUNK; k += ISM_THREADS) tap[k] = c0 + k < n_taps ? phi[c0 + k] : 0.0;
      __syncthreads();
      const int m = min(ISM_BAND_CHUNK, n_taps - c0);
      const double *mine = seg + (ISM_BAND_CHUNK - 1) + tid;
      if (draws) {
        for (int i = 0; i < m; ++i) {
          const double w = tap[i];
#pragma unroll
          for (int s = 0; s < ISM_PER_LANE; ++s) acc_g[s] += w * mine[s * ISM_THREADS - i];
        }
      } else {
        for (int i = 0; i < m; ++i) {
          const double w = tap[i];
#pragma unroll
          for (int s = 0; s < ISM_PER_LANE; ++s) acc[s] += w * mine[s * ISM_THREADS - i];
        }
      }
    }
  }
  const double *ln_env = ism_tail_table(job.tail, 0, n);   // the source's knots
#pragma unroll
  for (int s = 0; s < ISM_PER_LANE; ++s) {
    const int ts = t + s * ISM_THREADS;
    if (ts >= job.pitch) continue;
    double v = acc[s];
    if (ts > job.tail.mix && ts < job.ir_len) {   // at or below M: w_e = 1, w_l = 0, the image part as it is
      const int k = ts / ISM_TILE, r = ts % ISM_TILE;
      const double p = (double)r / (double)ISM_TILE;
      const double e = r == 0 ? exp(ln_env[k]) : (1.0 - p) * exp(ln_env[k]) + p * exp(ln_env[k + 1]);
      const double noise = e * acc_g[s];
      const double x = ((double)ts - (double)job.tail.mix) / (double)job.tail.fade;
      if (x < 1.0) {
        double w_e, w_l;
        sincospi(0.5 * x, &w_l, &w_e);
        v = w_e * acc[s] + w_l * noise;
      } else {
        v = noise;
      }
    }
    row[ts] = ts < job.ir_len ? (float)v : 0.f;
  }
}

// al_ism_shoebox_sphere's arguments as the kernels' job: 0 with *sj filled, or the error of the first bad argument.  mix < 0: no
// tail, and the tail's arguments are not looked at
inline int ism_sphere_prepare(const double *sources, int32_t n_sources, const double *source_patterns, const double *centre,
                              const double *directions, int32_t n_capsules, const double *L, const double *beta, double air,
                              const double *filters, int32_t n_orders, int32_t half, const double *diffuse, double c, double fs,
                              int32_t max_order, int32_t ir_len, int32_t pitch, int64_t mix, int64_t fade, uint64_t seed, int64_t source_id0,
                              int64_t capsule_id0, const double *ln_env, int32_t n_knots, void *workspace, int64_t workspace_bytes, float *out,
                              IsmSphereJob *sj) {
  IsmBandJob *bj = &sj->bj;
  if (int rc = ism_rows_range("al_ism_shoebox_sphere", "n_orders", n_orders, ISM_SPHERE_MAX_ORDERS, half, ISM_SPHERE_MAX_HALF)) return rc;
  if (!centre) return fail(AL_E_BADARG, "al_ism_shoebox: null pointer");
  if (!filters) return fail(AL_E_BADARG, "al_ism_shoebox_sphere: null filter table");
  if (mix >= 0 && !diffuse) return fail(AL_E_BADARG, "al_ism_shoebox_sphere: null diffuse-field filter");
  // ism_prepare refuses what al_ism_shoebox refuses; the "capsules" it counts are the directions' rows
  if (int rc = ism_prepare(sources, n_sources, directions, n_capsules, L, beta, c, fs, max_order, ir_len, pitch, out, &bj->base)) return rc;
  for (int i = 0; i < 3; ++i) {
    if (!isfinite(centre[i])) return fail(AL_E_BADARG, "al_ism_shoebox_sphere: the centre must be finite");
    sj->centre[i] = centre[i];
  }
  if (int rc = ism_source_prepare(source_patterns, air, &bj->base)) return rc;
  for (int b = 0; b < ISM_MAX_BANDS; ++b) {   // the band tables are not read: the walls are the job's one column
    bj->air[b] = 0.0;
    for (int i = 0; i < 6; ++i) bj->ln_beta[b][i] = 0.0, bj->beta_zero[b][i] = 0;
  }
  bj->filters = filters;
  bj->n_bands = n_orders;
  bj->half = half;
  sj->directions = directions;
  sj->diffuse = diffuse;
  if (int rc = ism_rows_prepare("al_ism_shoebox_sphere", L, workspace, workspace_bytes, mix, fade, seed, source_id0, capsule_id0, ln_env, n_knots, bj))
    return rc;
  if (mix >= 0) {
    if ((int64_t)n_knots * n_sources > 0xffffffffll) return fail(AL_E_BADARG, "al_ism_shoebox_sphere: n_knots x n_sources must be below 2^32");
    bj->base.tail.env_src_stride = (uint32_t)n_knots;   // (N, n_knots): a table per source, one law for every capsule
  }
  return AL_OK;
}

// THE LAUNCH: the passes over the workspace (ism_rows_passes), then with a tail the samples past the split
inline void launch_ism_shoebox_sphere(const IsmSphereJob &job, bool with_tail, hipStream_t stream) {
  const bool src = job.bj.base.source_patterns != nullptr || job.bj.base.air != 0.0;   // null and 0: the kernels without the source side
  IsmSphereJob sj = job;
  const dim3 block(ISM_THREADS);
  ism_rows_passes(
      sj.bj,
      [&](auto nb, dim3 grid) {
        if (src)
          hipLaunchKernelGGL((k_ism_sphere<decltype(nb)::value, true>), grid, block, 0, stream, sj);
        else
          hipLaunchKernelGGL((k_ism_sphere<decltype(nb)::value, false>), grid, block, 0, stream, sj);
      },
      [&](dim3 grid) {
        if (with_tail)
          hipLaunchKernelGGL(k_ism_sphere_combine, grid, block, 0, stream, sj);
        else
          hipLaunchKernelGGL(k_ism_band_combine<false>, grid, block, 0, stream, sj.bj);
      });
  if (with_tail) {   // k_ism_band_tail as it stands: one band, whose filter is psi_d, under the source's knots
    IsmBandJob tj = job.bj;
    tj.n_bands = 1;
    tj.filters = job.diffuse;
    launch_ism_band_tail(tj, stream);
  }
}

}  // namespace al
