// The frequency-domain accumulate Y[k] = sum_p X[k-p] * H[p] of the partitioned convolution: the tile kernels, the capsule-loop
// kernels for static events (register, LDS-staged, LDS-DMA), the sliding-window kernel for moving events, and the one table
// (MAC_ROWS / plan_mac) that says which instantiation takes a batch.  A new accumulate instantiation is a new row of that table.
#pragma once
#include <hip/hip_runtime.h>

#include "al_common.h"
#include "al_fft.h"

namespace al {

// ------------------------------------------------------------------ 4. frequency-domain accumulate
// Y[k] = sum_p X[k-p] * H[p] is a Toeplitz product per frequency bin.  One thread owns one bin and
// walks (k-tile x p-tile) pairs: the KT accumulators and PT partition spectra of the pair stay in
// registers and the KT+PT-1 signal blocks on its anti-diagonals are loaded ONCE each, so a pair
// costs KT+2*PT-1 loads for KT*PT complex FMAs (static register indices throughout).
// Bin 0 packs (DC, Nyquist): two independent real products.
// VB = bins per thread (1: float2 accesses, 2: float4 accesses of two adjacent bins).
// a += x * h (complex) as TWO v_pk_fma_f32 whose operand halves are picked by op_sel / negated by neg_lo: no swizzled
// copies of x or h exist in registers (left to itself hipcc keeps (x.x, x.x) and (-x.y, x.y) for every resident spectrum,
// doubling its register cost: profiles/r01_mac_variants.txt).
__device__ __forceinline__ void cfma_packed(float2 &a, const float2 &x, const float2 &h) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef float v2f __attribute__((ext_vector_type(2)));
  v2f av = {a.x, a.y};
  const v2f xv = {x.x, x.y}, hv = {h.x, h.y};
  // lo: x.x*h.x + a.x          hi: x.x*h.y + a.y
  asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[0,1,1]" : "+v"(av) : "v"(xv), "v"(hv));
  // lo: -x.y*h.y + a.x         hi: x.y*h.x + a.y
  asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]" : "+v"(av) : "v"(xv), "v"(hv));
  a = make_float2(av.x, av.y);
#else
  cfma(a, x, h);
#endif
}

template <int VB> struct BinVec;
template <> struct BinVec<1> {
  float2 a;
  __device__ __forceinline__ static BinVec zero() { return BinVec{make_float2(0.f, 0.f)}; }
  __device__ __forceinline__ static BinVec load(const float2 *p) { return BinVec{*p}; }
  __device__ __forceinline__ void store(float2 *p) const { stream_store<1>(p, a); }
  __device__ __forceinline__ void scale(float g) { a.x *= g; a.y *= g; }
  // BIN0: this wave may hold bin 0 (packed DC/Nyquist: two real products); every other wave takes the plain path
  template <bool BIN0>
  __device__ __forceinline__ void fma(const BinVec &x, const BinVec &h, bool packed) {
    if (BIN0 && packed) { a.x = fmaf(x.a.x, h.a.x, a.x); a.y = fmaf(x.a.y, h.a.y, a.y); } else cfma(a, x.a, h.a);
  }
};
template <> struct BinVec<2> {
  float2 a, c;
  __device__ __forceinline__ static BinVec zero() { return BinVec{make_float2(0.f, 0.f), make_float2(0.f, 0.f)}; }
  __device__ __forceinline__ static BinVec load(const float2 *p) {
    const float4 v = *reinterpret_cast<const float4 *>(p);
    return BinVec{make_float2(v.x, v.y), make_float2(v.z, v.w)};
  }
  __device__ __forceinline__ void store(float2 *p) const { stream_store<1>(reinterpret_cast<float4 *>(p), make_float4(a.x, a.y, c.x, c.y)); }
  __device__ __forceinline__ void scale(float g) { a.x *= g; a.y *= g; c.x *= g; c.y *= g; }
  template <bool BIN0>
  __device__ __forceinline__ void fma(const BinVec &x, const BinVec &h, bool packed) {
    if (BIN0 && packed) { a.x = fmaf(x.a.x, h.a.x, a.x); a.y = fmaf(x.a.y, h.a.y, a.y); } else cfma(a, x.a, h.a);
    cfma(c, x.c, h.c);
  }
  template <bool BIN0>
  __device__ __forceinline__ void fma_packed(const BinVec &x, const BinVec &h, bool packed) {
    if (BIN0 && packed) { a.x = fmaf(x.a.x, h.a.x, a.x); a.y = fmaf(x.a.y, h.a.y, a.y); } else cfma_packed(a, x.a, h.a);
    cfma_packed(c, x.c, h.c);
  }
};

// k_spectral_mac_static takes the one-emitter events when the flag is set and the partitions fit one register tile
__host__ __device__ __forceinline__ bool static_mac_active(const al_batch &b) {
  // up to 21 partitions through the LDS-DMA kernel (it reads the rows past an odd partition count from the all-zero block),
  // up to 16 through the register-staged one when the caller gave no zero block.  22..24 stay on the tile kernels: three
  // units of 8 fit (ends of the 35-block window in LDS) but only tie them at C = 32 and lose 5 % on cfg5 (profiles/r03_p24_ab.txt)
  return (b.flags & AL_FLAG_STATIC_MAC) && b.n_partitions <= (b.hspec_zero_block >= 0 ? 21 : 16) && b.log2_block >= 9;
}

// KSPLIT: every k-tile is its own workgroup (blockIdx.y = c * n_ktiles + tile) instead of a loop inside the thread.
// Workgroups of one bin tile share blockIdx.x, hence (round-robin dispatch) an XCD and its L2, and the tiles of one
// (event, capsule) are adjacent in dispatch order: the second..n-th read of the partition spectra hits L2.
template <int KT, int PT, int VB, bool KSPLIT, bool BIN0>
__device__ __forceinline__ void spectral_mac_body(const al_batch &b) {
  using V = BinVec<VB>;
  const int M = 1 << b.log2_block;
  const int f = (blockIdx.x * 256 + threadIdx.x) * VB;
  const int n_ktiles = KSPLIT ? (b.max_blocks + KT - 1) / KT : 1;
  const int c = blockIdx.y / n_ktiles;
  const al_event ev = b.events[b.event0 + blockIdx.z];
  if (ev.n_streams <= 0) return;
  if (ev.n_streams > 1 && ev.reserved == 1 && b.n_partitions <= AL_SPARSE_MAX_PARTITIONS) return;  // k_spectral_mac_moving
  if (ev.n_streams == 1 && static_mac_active(b)) return;     // k_spectral_mac_static
  const float2 *__restrict__ X = reinterpret_cast<const float2 *>(b.xspec);
  const float2 *__restrict__ H = reinterpret_cast<const float2 *>(b.hspec);
  float2 *__restrict__ Y = reinterpret_cast<float2 *>(b.yspec);
  const int K = ev.n_blocks, P = b.n_partitions;
  const bool packed = (f == 0);  // bin 0 holds (DC, Nyquist): two independent real products
  const int k_first = KSPLIT ? (blockIdx.y % n_ktiles) * KT : 0;
  const int k_limit = KSPLIT ? min(K, k_first + KT) : K;

  for (int k0 = k_first; k0 < k_limit; k0 += KT) {
    V acc[KT];
#pragma unroll
    for (int kk = 0; kk < KT; ++kk) acc[kk] = V::zero();
    for (int l = 0; l < ev.n_streams; ++l) {
      const al_stream st = b.streams[ev.stream0 + l];
      const int jlo = st.j_lo, jhi = st.j_lo + st.n_j;  // non-zero signal blocks [jlo, jhi)
      if (jhi <= jlo) continue;
      // partitions that can meet this k-tile: k0+kk-p in [jlo, jhi)
      const int plo = max(0, k0 - jhi + 1), phi = min(P - 1, k0 + KT - 1 - jlo);
      if (plo > phi) continue;
      const float g = b.emitter_gain[st.emitter];
      const float2 *hp = H + (((int64_t)(st.emitter - b.emitter0) * b.n_capsules + c) * P) * M + f;
      const float2 *xp = X + (int64_t)(st.xspec_base - b.xspec_block0 - jlo) * M + f;
      for (int p0 = plo; p0 <= phi; p0 += PT) {
        V h[PT];
#pragma unroll
        for (int pp = 0; pp < PT; ++pp) {
          // unconditional load at a clamped partition, zeroed by the select: keeps all PT loads in flight
          h[pp] = V::load(hp + (int64_t)min(p0 + pp, phi) * M);
          h[pp].scale((p0 + pp <= phi) ? g : 0.f);
        }
        const int jbase = k0 - p0 - (PT - 1);  // signal block of anti-diagonal jj is jbase + jj
        // The KT+PT-1 signal blocks are fetched in groups of XG, one group ahead of the FMAs that
        // consume them (explicit double buffer): the loads are L2 hits with ~1 us latency under load,
        // and a wave that waits for them one by one is latency-bound, not bandwidth-bound.
        constexpr int XG = 8 / VB, NJ = KT + PT - 1, NG = (NJ + XG - 1) / XG;
        auto fetch = [&](int jj) -> V {
          const int j = jbase + jj;
          V x = V::load(xp + (int64_t)min(max(j, jlo), jhi - 1) * M);  // clamped, unconditional
          x.scale((j >= jlo && j < jhi) ? 1.f : 0.f);
          return x;
        };
        V xa[XG], xb[XG];
        static_for<XG>([&](auto i_c) {
          constexpr int i = decltype(i_c)::value;
          if constexpr (i < NJ) xa[i] = fetch(i);
        });
        static_for<NG>([&](auto g_c) {
          constexpr int g_ = decltype(g_c)::value;
          static_for<XG>([&](auto i_c) {  // prefetch group g+1
            constexpr int i = decltype(i_c)::value;
            if constexpr ((g_ + 1) * XG + i < NJ) xb[i] = fetch((g_ + 1) * XG + i);
          });
          static_for<XG>([&](auto i_c) {  // consume group g
            constexpr int i = decltype(i_c)::value;
            constexpr int jj = g_ * XG + i;
            if constexpr (jj < NJ) {
              static_for<KT>([&](auto kk_c) {
                constexpr int kk = decltype(kk_c)::value;
                constexpr int pp = kk + (PT - 1) - jj;
                if constexpr (pp >= 0 && pp < PT) acc[kk].template fma<BIN0>(xa[i], h[pp], packed);
              });
            }
          });
          static_for<XG>([&](auto i_c) {
            constexpr int i = decltype(i_c)::value;
            if constexpr ((g_ + 1) * XG + i < NJ) xa[i] = xb[i];
          });
        });
      }
    }
#pragma unroll
    for (int kk = 0; kk < KT; ++kk)
      if (k0 + kk < K) acc[kk].store(Y + ((int64_t)(ev.yspec_base - b.yspec_block0) + (int64_t)c * K + k0 + kk) * M + f);
  }
}

// Bin 0 needs two real products instead of a complex one.  Only the first wave of the first bin tile can hold it:
// that wave runs the BIN0 instantiation (per-lane select), every other wave the plain complex path -- folding the
// select into the common path costs two extra FMAs and two v_cndmask per product for EVERY bin (measured: 43 % of
// the kernel's vector instructions).
template <int KT, int PT, int VB, bool KSPLIT = false>
__global__ __launch_bounds__(256) void k_spectral_mac(al_batch b) {
  if (blockIdx.x == 0 && threadIdx.x < 64) spectral_mac_body<KT, PT, VB, KSPLIT, true>(b);
  else spectral_mac_body<KT, PT, VB, KSPLIT, false>(b);
}

// ------------------------------------------------------------------ 4a. accumulate for static events, capsule loop
// A static event has ONE stream, so the signal blocks a (k-tile, bin tile) needs -- the KT+PT-1 blocks on its anti-
// diagonals -- are the same for every capsule.  One workgroup therefore owns (event, k-tile, bin tile) and LOOPS over the
// capsules with that window held in registers (loaded once, already multiplied by the emitter gain and zeroed where
// k - p leaves the clip: no per-capsule masks or gain multiplies).  What this buys over one workgroup per capsule
// (profiles/r02_mac.txt): the signal spectra leave L2 once instead of C times, the workgroup start-up (three dependent
// table reads) and the dispatch of 32x as many workgroups disappear, and because nothing waits on X any more the
// partition spectrum h[p] of the NEXT capsule is requested the moment the last product with h[p] of this one has been
// issued -- the H stream, the FMAs and the Y stores of consecutive capsules overlap inside one wave.
// PT is the batch's partition count itself (one instantiation per P = 1..12): every h[pp] is a real partition, nothing in the
// loop is masked.  (A 12-wide tile with the missing partitions zeroed by a multiply, selected from a zero block or skipped by
// a uniform branch spilled 104-192 B per lane and ran 25-70 % slower than the tile kernels at P = 10, profiles/r02_mac.txt.)
// NKTW: k-tiles per workgroup (256 threads each).  Two k-tiles of one (event, bin tile) read the SAME partition spectra;
// in one workgroup, kept in step by a barrier per capsule, the second read of every line is an L1 hit on the same CU
// instead of a second trip to L2 / HBM by another workgroup that may have drifted away.
// The capsule-loop kernels' bin tile: blockIdx.x rotated by blockIdx.z.  Workgroup ids are dealt round-robin over the 8 XCDs and the
// grids are 16 (or 32) bin tiles wide, so with the plain index an XCD would only ever touch two of the sixteen 4 KB columns of every
// spectrum block; rotated, every XCD sees every column: -3 % on the accumulate of cfg2, cfg4 and cfg5
// (profiles/r04z_rotated_ids_mac_synth_ab.txt).  (The tile kernel k_spectral_mac keeps the plain index: it WANTS the k-tiles of one
// bin tile on one XCD, for the L2 hits on H; the sliding-window kernel is 3.5 % slower rotated, r04z_rotated_ids_moving_ab.txt.)
__device__ __forceinline__ int rotated_bin_tile() { return (int)((blockIdx.x + blockIdx.z) % gridDim.x); }

template <int KT, int PT, bool BIN0, int NKTW>
__device__ __forceinline__ void spectral_mac_static_body(const al_batch &b, int bx) {
  using V = BinVec<2>;
  constexpr int NJ = KT + PT - 1;
  const int M = 1 << b.log2_block;
  const int lane256 = threadIdx.x & 255, sub = threadIdx.x >> 8;
  const int f = (bx * 256 + lane256) * 2;
  const int n_cs = gridDim.z / b.n_events;                      // capsule ranges per event (small batches)
  const int e = blockIdx.z / n_cs, cs = blockIdx.z % n_cs;
  const al_event ev = b.events[b.event0 + e];
  if (ev.n_streams != 1) return;                                // moving events: k_spectral_mac / k_spectral_mac_moving
  const int K = ev.n_blocks, P = b.n_partitions, C = b.n_capsules;
  const int k0 = (blockIdx.y * NKTW + sub) * KT;
  if (NKTW == 1 && k0 >= K) return;
  const bool active = k0 < K;                                   // NKTW > 1: an idle half still joins the barriers
  const int c_begin = (int)((int64_t)cs * C / n_cs), c_end = (int)((int64_t)(cs + 1) * C / n_cs);
  const al_stream st = b.streams[ev.stream0];
  const int jlo = st.j_lo, jhi = st.j_lo + st.n_j;
  const int plo = max(0, k0 - jhi + 1), phi = min(P - 1, k0 + KT - 1 - jlo);
  const bool packed = (f == 0);
  const float2 *__restrict__ X = reinterpret_cast<const float2 *>(b.xspec) + (int64_t)(st.xspec_base - b.xspec_block0 - jlo) * M + f;
  const float2 *__restrict__ H = reinterpret_cast<const float2 *>(b.hspec) + ((int64_t)(st.emitter - b.emitter0) * C * P) * M + f;
  float2 *__restrict__ Y = reinterpret_cast<float2 *>(b.yspec) + ((int64_t)(ev.yspec_base - b.yspec_block0) + k0) * M + f;
  const float g = b.emitter_gain[st.emitter];
  const bool single = phi - plo < PT;                           // one partition tile: the window survives the capsule loop
  // (plo > phi cannot happen for a static event, whose signal blocks are [0, K): plo = 0 <= phi)

  V xw[NJ];
  auto load_window = [&](int p0) {                              // xw[jj] = g * X[k0 - p0 - (PT-1) + jj], 0 outside the clip
    const int jbase = k0 - p0 - (PT - 1);
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
      const int j = jbase + jj;
      xw[jj] = V::load(X + (int64_t)min(max(j, jlo), jhi - 1) * M);
      xw[jj].scale((j >= jlo && j < jhi) ? g : 0.f);
    }
  };
  auto h_load = [&](int c, int p) { return V::load(H + ((int64_t)c * P + min(p, P - 1)) * M); };
  V h[PT];
  if (single && active) {
    load_window(plo);
#pragma unroll
    for (int pp = 0; pp < PT; ++pp) h[pp] = h_load(c_begin, plo + pp);
  }
  for (int c = c_begin; c < c_end; ++c) {
    if (NKTW > 1) __syncthreads();                              // both k-tiles start the capsule together
    if (!active) continue;
    const int cn = min(c + 1, c_end - 1);                       // capsule whose spectra are requested during this one
    V acc[KT];
#pragma unroll
    for (int kk = 0; kk < KT; ++kk) acc[kk] = V::zero();
    for (int p0 = plo; p0 <= phi; p0 += PT) {
      if (!single) {
        load_window(p0);
#pragma unroll
        for (int pp = 0; pp < PT; ++pp) h[pp] = h_load(c, p0 + pp);
      }
      static_for<PT>([&](auto pp_c) {
        constexpr int pp = decltype(pp_c)::value;
        static_for<KT>([&](auto kk_c) {
          constexpr int kk = decltype(kk_c)::value;
          acc[kk].template fma_packed<BIN0>(xw[kk + (PT - 1) - pp], h[pp], packed);   // X[k0 + kk - (p0 + pp)]
        });
        if (single) h[pp] = h_load(cn, plo + pp);                // h[pp] is free: fetch the next capsule's
      });
    }
#pragma unroll
    for (int kk = 0; kk < KT; ++kk)
      if (k0 + kk < K) acc[kk].store(Y + ((int64_t)c * K + kk) * M);
  }
}

template <int KT, int PT, int NKTW>
__global__ __launch_bounds__(256 * NKTW, 2) void k_spectral_mac_static(al_batch b) {
  const int bx = rotated_bin_tile();
  if (bx == 0 && (threadIdx.x & 255) < 64) spectral_mac_static_body<KT, PT, true, NKTW>(b, bx);
  else spectral_mac_static_body<KT, PT, false, NKTW>(b, bx);
}

// Variant of the two-k-tile workgroup for clips of more than 24 blocks (several workgroups per (event, bin tile), all reading
// the same partition spectra): the 512 threads copy the (PT x 512 slot) tile of capsule c+2 into a ring of three LDS stages
// while capsule c is multiplied, so H enters the CU once instead of twice (the second k-tile's L1 hit) and no partition
// spectrum waits in registers.  Equal to the register version at K <= 24, 8-10 % faster beyond (profiles/r02_mac.txt 10).
template <int KT, int PT, int UNITS, bool BIN0>
__device__ __forceinline__ void spectral_mac_static_lds_body(const al_batch &b, float4 *hbuf, int bx) {
  // UNITS = 2: 13..16 partitions as two units of PT = ceil(P / 2) per capsule (the pipeline step is a unit; for odd P the
  // last unit's missing partition is stored as zeros in its LDS stage, so nothing in the products is masked)
  using V = BinVec<2>;
  constexpr int PALL = UNITS * PT, NJ = KT + PALL - 1, STAGE = PT * 256, PER = (STAGE + 511) / 512;
  const int M = 1 << b.log2_block;
  const int lane256 = threadIdx.x & 255, sub = threadIdx.x >> 8;
  const int f = (bx * 256 + lane256) * 2;
  const int n_cs = gridDim.z / b.n_events;
  const int e = blockIdx.z / n_cs, cs = blockIdx.z % n_cs;
  const al_event ev = b.events[b.event0 + e];
  if (ev.n_streams != 1) return;
  const int K = ev.n_blocks, P = b.n_partitions, C = b.n_capsules;
  const int k0 = (blockIdx.y * 2 + sub) * KT;
  const bool active = k0 < K;
  const int c_begin = (int)((int64_t)cs * C / n_cs), c_end = (int)((int64_t)(cs + 1) * C / n_cs);
  const al_stream st = b.streams[ev.stream0];
  const int jlo = st.j_lo, jhi = st.j_lo + st.n_j;
  const bool packed = (f == 0);
  const float2 *__restrict__ X = reinterpret_cast<const float2 *>(b.xspec) + (int64_t)(st.xspec_base - b.xspec_block0 - jlo) * M + f;
  const float2 *__restrict__ Htile = reinterpret_cast<const float2 *>(b.hspec) + ((int64_t)(st.emitter - b.emitter0) * C * P) * M + bx * 512;
  float2 *__restrict__ Y = reinterpret_cast<float2 *>(b.yspec) + ((int64_t)(ev.yspec_base - b.yspec_block0) + k0) * M + f;
  const float g = b.emitter_gain[st.emitter];
  V xw[NJ];
  if (active) {
    const int jbase = k0 - (PALL - 1);
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
      const int j = jbase + jj;
      xw[jj] = V::load(X + (int64_t)min(max(j, jlo), jhi - 1) * M);
      xw[jj].scale((j >= jlo && j < jhi) ? g : 0.f);
    }
  }
  static_assert(PER <= 6, "staging registers are named, not indexed (an indexed array stayed in scratch memory)");
  float4 g0, g1, g2, g3, g4, g5;
  g0 = g1 = g2 = g3 = g4 = g5 = make_float4(0.f, 0.f, 0.f, 0.f);
  const int n_units = UNITS * (c_end - c_begin);
  // unit n = (capsule c_begin + n / UNITS, partitions [(n % UNITS) * PT, +PT)); row r of the copy is partition p0 + r
#define AL_FETCH1(R, I, C_, P0_)                                                                                             \
  if ((I) < PER && (STAGE % 512 == 0 || (int)threadIdx.x + 512 * (I) < STAGE)) {                                             \
    const int q_ = (int)threadIdx.x + 512 * (I), p_ = (P0_) + (q_ >> 8);                                                     \
    R = (UNITS == 1 || p_ < P) ? *reinterpret_cast<const float4 *>(Htile + ((int64_t)(C_) * P + min(p_, P - 1)) * M + (q_ & 255) * 2) \
                               : make_float4(0.f, 0.f, 0.f, 0.f);                                                            \
  }
#define AL_FETCH(UNIT)                                                                                                       \
  { const int n_ = min((UNIT), n_units - 1), cc_ = c_begin + n_ / UNITS, p0_ = (n_ % UNITS) * PT;                            \
    AL_FETCH1(g0, 0, cc_, p0_) AL_FETCH1(g1, 1, cc_, p0_) AL_FETCH1(g2, 2, cc_, p0_) AL_FETCH1(g3, 3, cc_, p0_)               \
    AL_FETCH1(g4, 4, cc_, p0_) AL_FETCH1(g5, 5, cc_, p0_) }
#define AL_STASH1(R, I, S)                                                                                                   \
  if ((I) < PER && (STAGE % 512 == 0 || (int)threadIdx.x + 512 * (I) < STAGE)) hbuf[(S) * STAGE + threadIdx.x + 512 * (I)] = R;
#define AL_STASH(STAGE_INDEX)                                                                                                \
  { const int ss_ = (STAGE_INDEX); AL_STASH1(g0, 0, ss_) AL_STASH1(g1, 1, ss_) AL_STASH1(g2, 2, ss_) AL_STASH1(g3, 3, ss_)   \
    AL_STASH1(g4, 4, ss_) AL_STASH1(g5, 5, ss_) }
  AL_FETCH(0)
  AL_STASH(0)
  AL_FETCH(1)
  AL_STASH(1)
  int n = 0;                                                    // unit being multiplied
  for (int c = c_begin; c < c_end; ++c) {
    V acc[KT];
#pragma unroll
    for (int kk = 0; kk < KT; ++kk) acc[kk] = V::zero();
    static_for<UNITS>([&](auto u_c) {
      constexpr int u = decltype(u_c)::value;
      const int cur = n % 3, nxt = (n + 2) % 3;
      AL_FETCH(n + 2)                                           // in flight during this unit's products (past the end the last
                                                                // unit is fetched again: unconditional code)
      __syncthreads();                                          // stage `cur` is complete, stage `nxt` is no longer read
      if (active) {
        const float4 *hs = hbuf + cur * STAGE + lane256;
        float4 hv = hs[0], hn = hv;
        static_for<PT>([&](auto pp_c) {
          constexpr int pp = decltype(pp_c)::value;
          if constexpr (pp + 1 < PT) {                          // the next partition's LDS read is issued before this one's
            hn = hs[(pp + 1) * 256];                            // products, not a few instructions before its first use
#if defined(__HIP_DEVICE_COMPILE__)
            __builtin_amdgcn_sched_barrier(0);
#endif
          }
          const V h{make_float2(hv.x, hv.y), make_float2(hv.z, hv.w)};
          static_for<KT>([&](auto kk_c) {
            constexpr int kk = decltype(kk_c)::value;
            acc[kk].template fma_packed<BIN0>(xw[kk + (PALL - 1) - (u * PT + pp)], h, packed);
          });
          hv = hn;
        });
      }
      AL_STASH(nxt)
      ++n;
    });
    if (active) {
#pragma unroll
      for (int kk = 0; kk < KT; ++kk)
        if (k0 + kk < K) acc[kk].store(Y + ((int64_t)c * K + kk) * M);
    }
  }
#undef AL_FETCH
#undef AL_STASH
#undef AL_FETCH1
#undef AL_STASH1
}

template <int KT, int PT, int UNITS = 1>
__global__ __launch_bounds__(512, 2) void k_spectral_mac_static_lds(al_batch b) {
  __shared__ float4 hbuf[3 * PT * 256];
  const int bx = rotated_bin_tile();
  if (bx == 0 && (threadIdx.x & 255) < 64) spectral_mac_static_lds_body<KT, PT, UNITS, true>(b, hbuf, bx);
  else spectral_mac_static_lds_body<KT, PT, UNITS, false>(b, hbuf, bx);
}

// ------------------------------------------------------------------ 4a'. capsule loop fed by LDS-DMA
// The same loop with the partition spectra brought into the LDS ring by LDS-DMA (global_load_lds_dwordx4: the data never
// passes through a VGPR and the instruction returns at once).  A wave has only two register sets' worth of room, so the
// register versions request capsule c+1's spectra WHILE capsule c is multiplied -- one iteration (a few microseconds) of
// flight time, less than the latency of a loaded HBM (profiles/r02_mac.txt 9).  Here the request for unit n+2 is issued at the
// start of unit n and retired by a COUNTED s_waitcnt at the start of unit n+2: two iterations in flight, no staging
// registers, no ds_write pass.  Protocol per unit n (cdna_hip_programming.md section 5, "Pipelining across barriers"):
//     s_waitcnt vmcnt(N)   this wave's DMA pieces of unit n have landed (N = the VMEM operations it issued after them:
//                          the pieces of unit n+1 and the Y stores in between; VMEM operations of a wave retire in order)
//     s_barrier            ... and so have every other wave's; everybody is done reading the stage unit n+2 will overwrite
//     issue DMA of unit n+2 -> stage (n+2) % 3;   multiply unit n out of stage n % 3;   store Y at the end of a capsule
// The DMA is inline asm (hipcc would drain every outstanding one with vmcnt(0) before the first LDS read it knows to depend
// on it); the waits are therefore counted by hand.  Every wave issues the same number of pieces (the last piece is fetched
// again where PT * 4 is not a multiple of 8) and every half issues exactly its own number of stores per capsule.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "k_spectral_mac_static_glds counts stores in vmcnt and uses global_load_lds_dwordx4: gfx950 only (a target with a separate store counter would read stale LDS)"
#endif
#if defined(__HIP_DEVICE_COMPILE__)
// 64 lanes x 16 B from (uniform base in SGPRs) + (lane offset in ONE VGPR shared by every piece) into LDS at lds_dst + lane * 16:
// all the address arithmetic of a piece is scalar
__device__ __forceinline__ void glds16(const void *sbase, unsigned voff, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
  al::shake(105);   // (test builds only, al_common.h: no memory operation, so the counted waits below are not disturbed)
}
template <int N>
__device__ __forceinline__ void wait_vm() {
  al::shake(106);
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
#endif

// NL: the NL signal blocks at EACH end of the window live in LDS instead of registers.  Block jj of the window meets
// min(jj + 1, NJ - jj, KT) products per capsule, so the ends are the cheap ones to re-read: NL = 3 costs 12 extra
// ds_read_b128 per capsule and frees 24 VGPRs, which is what the 32-block window of 19..21 partitions (NL = 2) needs to stay
// out of scratch memory (a spill reload would also drain the LDS-DMA in flight: hipcc waits vmcnt(0) for it).
template <int KT, int PT, int UNITS, bool BIN0, bool ZERO_ROWS = (UNITS > 1), int NL = 0, int NKTW = 2>
__device__ __forceinline__ void spectral_mac_static_glds_body(const al_batch &b, float4 *hbuf, float4 *xbuf, int bx) {
  using V = BinVec<2>;
  constexpr int NWAVES = 4 * NKTW;      // NKTW k-tiles of 256 threads per workgroup
  constexpr int PALL = UNITS * PT, NJ = KT + PALL - 1, STAGE = PT * 256, PIECES = PT * 4, PER_WAVE = (PIECES + NWAVES - 1) / NWAVES;
  const int M = 1 << b.log2_block;
  const int lane256 = threadIdx.x & 255, sub = threadIdx.x >> 8, lane = threadIdx.x & 63;
  const int f = (bx * 256 + lane256) * 2;
  const int n_cs = gridDim.z / b.n_events;
  const int e = blockIdx.z / n_cs, cs = blockIdx.z % n_cs;
  const al_event ev = b.events[b.event0 + e];
  if (ev.n_streams != 1) return;
  const int K = ev.n_blocks, P = b.n_partitions, C = b.n_capsules;
  const int k0 = (blockIdx.y * NKTW + sub) * KT;
  const bool active = k0 < K;
  const int n_stores = active ? min(KT, K - k0) : 0;            // Y stores this half issues per capsule (workgroup-half uniform)
  const int c_begin = (int)((int64_t)cs * C / n_cs), c_end = (int)((int64_t)(cs + 1) * C / n_cs);
  const al_stream st = b.streams[ev.stream0];
  const int jlo = st.j_lo, jhi = st.j_lo + st.n_j;
  const bool packed = (f == 0);
  const float2 *__restrict__ X = reinterpret_cast<const float2 *>(b.xspec) + (int64_t)(st.xspec_base - b.xspec_block0 - jlo) * M + f;
  const float2 *__restrict__ Htile = reinterpret_cast<const float2 *>(b.hspec) + ((int64_t)(st.emitter - b.emitter0) * C * P) * M + bx * 512;
  const float2 *__restrict__ Hzero = reinterpret_cast<const float2 *>(b.hspec) + (int64_t)max(b.hspec_zero_block, 0) * M;   // rows past P (odd P in units)
  float2 *__restrict__ Y = reinterpret_cast<float2 *>(b.yspec) + ((int64_t)(ev.yspec_base - b.yspec_block0) + k0) * M + f;
  const float g = b.emitter_gain[st.emitter];
  V xw[NJ - 2 * NL];                                            // window blocks [NL, NJ - NL); the ends are in xbuf
  if (active) {
    const int jbase = k0 - (PALL - 1);
    static_for<NJ>([&](auto jj_c) {
      constexpr int jj = decltype(jj_c)::value;
      const int j = jbase + jj;
      V x = V::load(X + (int64_t)min(max(j, jlo), jhi - 1) * M);
      x.scale((j >= jlo && j < jhi) ? g : 0.f);
      if constexpr (jj < NL) xbuf[jj * (256 * NKTW) + threadIdx.x] = make_float4(x.a.x, x.a.y, x.c.x, x.c.y);
      else if constexpr (jj >= NJ - NL) xbuf[(jj - (NJ - 2 * NL)) * (256 * NKTW) + threadIdx.x] = make_float4(x.a.x, x.a.y, x.c.x, x.c.y);
      else xw[jj - NL] = x;
    });
  }
  auto window = [&](auto jj_c) -> V {                          // a thread reads back only what it wrote: no barrier needed
    constexpr int jj = decltype(jj_c)::value;
    if constexpr (jj < NL || jj >= NJ - NL) {
      const float4 v = xbuf[(jj < NL ? jj : jj - (NJ - 2 * NL)) * (256 * NKTW) + threadIdx.x];
      return V{make_float2(v.x, v.y), make_float2(v.z, v.w)};
    } else {
      return xw[jj - NL];
    }
  };
  const int n_units = UNITS * (c_end - c_begin);
#if defined(__HIP_DEVICE_COMPILE__)
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  __attribute__((address_space(3))) float4 *hbuf_lds = (__attribute__((address_space(3))) float4 *)hbuf;
  const unsigned lds_base = (unsigned)(uintptr_t)hbuf_lds;      // byte offset of the ring inside the workgroup's LDS
#else
  const int wave = (int)(threadIdx.x >> 6);
#endif
  // unit n = (capsule c_begin + n / UNITS, partitions [(n % UNITS) * PT, +PT)); piece q of row r = 1 KB = 64 lanes x 16 B
  auto issue = [&](int n) {
    const int n_ = min(n, n_units - 1), cc = c_begin + n_ / UNITS, p0 = (n_ % UNITS) * PT, stage = n % 3;
#pragma unroll
    for (int i = 0; i < PER_WAVE; ++i) {
      const int piece = min(wave + NWAVES * i, PIECES - 1), r = piece >> 2, q = piece & 3, p = p0 + r;
      const float2 *src = ((!ZERO_ROWS || p < P) ? Htile + ((int64_t)cc * P + p) * M : Hzero) + q * 128;   // wave-uniform
#if defined(__HIP_DEVICE_COMPILE__)
      glds16(src, (unsigned)lane * 16u, lds_base + (unsigned)(stage * STAGE + r * 256 + q * 64) * 16u);
#else
      hbuf[stage * STAGE + r * 256 + q * 64 + lane] = *reinterpret_cast<const float4 *>(src + lane * 2);
#endif
    }
  };
  // N of the counted wait in front of unit n: VMEM operations issued after the pieces of unit n, i.e. the pieces of unit
  // n+1 and the stores that fell between them; exact for UNITS == 1 (a capsule per unit: the stores of the two previous
  // capsules), the pieces alone otherwise (stricter than needed when a capsule ended in between: still correct)
  auto wait_unit = [&](int unit) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (UNITS == 1) {
      switch (min(unit, 2) * n_stores) {     // the first two capsules have fewer stores behind them
#define AL_WAIT_CASE(S) case S: wait_vm<PER_WAVE + S>(); break;
        AL_WAIT_CASE(0) AL_WAIT_CASE(1) AL_WAIT_CASE(2) AL_WAIT_CASE(3) AL_WAIT_CASE(4) AL_WAIT_CASE(5) AL_WAIT_CASE(6)
        AL_WAIT_CASE(7) AL_WAIT_CASE(8) AL_WAIT_CASE(9) AL_WAIT_CASE(10) AL_WAIT_CASE(11) AL_WAIT_CASE(12) AL_WAIT_CASE(14)
        AL_WAIT_CASE(16) AL_WAIT_CASE(18) AL_WAIT_CASE(20) AL_WAIT_CASE(22) AL_WAIT_CASE(24)
#undef AL_WAIT_CASE
        default: wait_vm<PER_WAVE>(); break;
      }
    } else {
      wait_vm<PER_WAVE>();
    }
    __builtin_amdgcn_s_barrier();
#else
    __syncthreads();
#endif
  };
  static_assert(KT <= 12, "the counted waits enumerate at most 12 stores per capsule");
  static_assert(PER_WAVE + 24 <= 63, "vmcnt is a 6-bit counter: the pieces of a unit plus two capsules' stores must fit it");
  issue(0);
  issue(1);
  int n = 0;
  for (int c = c_begin; c < c_end; ++c) {
    V acc[KT];
#pragma unroll
    for (int kk = 0; kk < KT; ++kk) acc[kk] = V::zero();
    static_for<UNITS>([&](auto u_c) {
      constexpr int u = decltype(u_c)::value;
      wait_unit(n);                                             // unit n is in stage n % 3; stage (n + 2) % 3 is no longer read
      issue(n + 2);
      if (active) {
        const float4 *hs = hbuf + (n % 3) * STAGE + lane256;
        float4 hv = hs[0], hn = hv;
        static_for<PT>([&](auto pp_c) {
          constexpr int pp = decltype(pp_c)::value;
          if constexpr (pp + 1 < PT) {
            hn = hs[(pp + 1) * 256];
#if defined(__HIP_DEVICE_COMPILE__)
            __builtin_amdgcn_sched_barrier(0);
#endif
          }
          const V h{make_float2(hv.x, hv.y), make_float2(hv.z, hv.w)};
          static_for<KT>([&](auto kk_c) {
            constexpr int kk = decltype(kk_c)::value;
            acc[kk].template fma_packed<BIN0>(window(std::integral_constant<int, kk + (PALL - 1) - (u * PT + pp)>{}), h, packed);
          });
          hv = hn;
        });
      }
      ++n;
    });
    if (active) {
#pragma unroll
      for (int kk = 0; kk < KT; ++kk)
        if (kk < n_stores) acc[kk].store(Y + ((int64_t)c * K + kk) * M);
    }
  }
#if defined(__HIP_DEVICE_COMPILE__)
  wait_vm<0>();   // the two re-fetched units past the end must have landed before the LDS goes back to the next workgroup
#endif
}

// ZERO_ROWS: the partition count is not a multiple of UNITS * PT, the missing rows of the last unit come from the all-zero block
template <int KT, int PT, int UNITS = 1, bool ZERO_ROWS = (UNITS > 1), int NL = 0, int NKTW = 2>
__global__ __launch_bounds__(256 * NKTW, NKTW) void k_spectral_mac_static_glds(al_batch b) {
  __shared__ float4 hbuf[3 * PT * 256];
  __shared__ float4 xbuf[NL > 0 ? 2 * NL * 256 * NKTW : 1];
  const int bx = rotated_bin_tile();
  if (bx == 0 && (threadIdx.x & 255) < 64) spectral_mac_static_glds_body<KT, PT, UNITS, true, ZERO_ROWS, NL, NKTW>(b, hbuf, xbuf, bx);
  else spectral_mac_static_glds_body<KT, PT, UNITS, false, ZERO_ROWS, NL, NKTW>(b, hbuf, xbuf, bx);
}

// ------------------------------------------------------------------ 4b. accumulate for moving events
// A moving event is N streams (one per IR) whose clips are only a few blocks long (the cross-fade window of
// that IR) and whose first blocks j_lo are non-decreasing.  One thread owns one bin (pair) of one capsule and
// walks the streams in order with a SLIDING window of W = NJW + PT - 1 output accumulators anchored at the
// current stream's j_lo: blocks that fall behind the window are complete and are written out once.  Every H,
// X and Y value moves exactly once and every register index is static.
template <int NJW, int PT, int VB, bool BIN0>
__device__ __forceinline__ void spectral_mac_moving_body(const al_batch &b, int4 *tab, float *gains) {
  using V = BinVec<VB>;
  constexpr int W = NJW + PT - 1;
  const int M = 1 << b.log2_block;
  const int f = (blockIdx.x * 256 + threadIdx.x) * VB;
  const int c = blockIdx.y;
  const al_event ev = b.events[b.event0 + blockIdx.z];
  if (ev.n_streams <= 1 || ev.reserved != 1) return;  // static / dense events: k_spectral_mac
  const float2 *__restrict__ X = reinterpret_cast<const float2 *>(b.xspec);
  const float2 *__restrict__ H = reinterpret_cast<const float2 *>(b.hspec);
  float2 *__restrict__ Y = reinterpret_cast<float2 *>(b.yspec) + ((int64_t)(ev.yspec_base - b.yspec_block0) + (int64_t)c * ev.n_blocks) * M + f;
  const int K = ev.n_blocks, P = b.n_partitions;
  const bool packed = (f == 0);
  V acc[W];
#pragma unroll
  for (int w = 0; w < W; ++w) acc[w] = V::zero();
  int kbase = 0;  // output block held in acc[0]
  for (int l0 = 0; l0 < ev.n_streams; l0 += 64) {
    __syncthreads();
    if (threadIdx.x < 64 && l0 + (int)threadIdx.x < ev.n_streams) {
      const al_stream st = b.streams[ev.stream0 + l0 + threadIdx.x];
      tab[threadIdx.x] = make_int4(st.j_lo, st.n_j, st.emitter - b.emitter0, st.xspec_base - b.xspec_block0);
      gains[threadIdx.x] = b.emitter_gain[st.emitter];
    }
    __syncthreads();
    const int nl = min(64, ev.n_streams - l0);
    for (int l = 0; l < nl; ++l) {
      const int4 t = tab[l];
      const int jlo = t.x, nj = t.y;
      if (nj <= 0) continue;
      // retire the blocks before this stream's first block
      while (kbase < jlo) {
        if (kbase < K) acc[0].store(Y + (int64_t)kbase * M);
#pragma unroll
        for (int w = 0; w + 1 < W; ++w) acc[w] = acc[w + 1];
        acc[W - 1] = V::zero();
        ++kbase;
      }
      // partitions of this IR that reach a block the event keeps (pad_or_truncate, synthesize.py:590, drops everything from
      // block K on): partition p of a stream that starts at block j_lo only feeds blocks >= j_lo + p.  The others are not read.
      const int pl = min(P, K - jlo);
      if (pl <= 0) continue;
      const float g = gains[l];
      const float2 *hp = H + (((int64_t)t.z * b.n_capsules + c) * P) * M + f;
      const float2 *xp = X + (int64_t)t.w * M + f;
      V h[PT], x[NJW];
#pragma unroll
      for (int pp = 0; pp < PT; ++pp) {
        h[pp] = V::load(hp + (int64_t)min(pp, pl - 1) * M);
        h[pp].scale(pp < pl ? g : 0.f);
      }
#pragma unroll
      for (int jj = 0; jj < NJW; ++jj) {
        x[jj] = V::load(xp + (int64_t)min(jj, nj - 1) * M);
        x[jj].scale(jj < nj ? 1.f : 0.f);
      }
#pragma unroll
      for (int jj = 0; jj < NJW; ++jj)
#pragma unroll
        for (int pp = 0; pp < PT; ++pp) acc[jj + pp].template fma<BIN0>(x[jj], h[pp], packed);
    }
  }
#pragma unroll
  for (int w = 0; w < W; ++w)
    if (kbase + w < K) acc[w].store(Y + (int64_t)(kbase + w) * M);
  // blocks beyond the last window (no stream reaches them) are zero
  for (int k = kbase + W; k < K; ++k) V::zero().store(Y + (int64_t)k * M);
}

template <int NJW, int PT, int VB>
__global__ __launch_bounds__(256) void k_spectral_mac_moving(al_batch b) {
  __shared__ int4 tab[64];    // {j_lo, n_j, emitter - emitter0, xspec_base - xspec_block0}
  __shared__ float gains[64];
  // both instantiations run the same barriers in the same order, so splitting the workgroup by wave is safe
  if (blockIdx.x == 0 && threadIdx.x < 64) spectral_mac_moving_body<NJW, PT, VB, true>(b, tab, gains);
  else spectral_mac_moving_body<NJW, PT, VB, false>(b, tab, gains);
}

// ------------------------------------------------------------------ 4c. dispatch
// ONE description of what al_spectral_mac launches for a batch: every accumulate instantiation the library ships is a row of
// MAC_ROWS, plan_mac picks rows, al_spectral_mac launches them and al_spectral_mac_variant reports them, so the parity tests'
// "which instantiation ran" assertion cannot drift from the launcher.  Codes (include/audiblelight_hip.h, al_spectral_mac_variant):
// tile kernel k_spectral_mac<KT,PT,VB,KSPLIT> = 1000000*KSPLIT + 10000*KT + 100*PT + VB; capsule-loop kernels 3120000 + 100*P + D,
// D = 1: k_spectral_mac_static<12,P,1> (clips of at most 12 blocks), 2: <12,P,2> (13..24 blocks), 3: the partition spectra staged
// through LDS by registers, k_spectral_mac_static_lds<12,P> (more than 24 blocks) or <12,ceil(P/2),2> (13..16 partitions without
// hspec_zero_block), 4: staged by LDS-DMA, k_spectral_mac_static_glds (13..21 partitions as two or three units per capsule, any
// clip length, needs hspec_zero_block >= 0; at most 12 partitions only under AL_FLAG_MAC_LDS_DMA); sliding-window kernel
// k_spectral_mac_moving<6,PT,1> = 600 + PT.
struct MacRow {
  void (*kernel)(al_batch);
  int threads;         // workgroup size; the capsule-loop kernels hold threads / 256 k-tiles per workgroup
  int code;            // what al_spectral_mac_variant reports; capsule-loop rows: 3120000 + D, reported with 100 * P added
  int p_lo, p_hi;      // capsule-loop rows: the partition counts this instantiation serves (0, 0: any)
  int kt, vb, ksplit;  // k-tile, bins per thread, one workgroup per k-tile: what the grid rule needs
};
#define AL_TILE(KT, PT, VB, KS) {k_spectral_mac<KT, PT, VB, KS>, 256, 1000000 * KS + 10000 * KT + 100 * PT + VB, 0, 0, KT, VB, KS},
#define AL_LOOP(NKTW, D, P_LO, P_HI, ...) {__VA_ARGS__, 256 * NKTW, 3120000 + D, P_LO, P_HI, 12, 2, 0},
#define AL_MOVING(PT) {k_spectral_mac_moving<AL_SPARSE_MAX_NJ, PT, 1>, 256, 100 * AL_SPARSE_MAX_NJ + PT, 0, 0, 0, 1, 0},
// the partition tile IS the partition count for at most 12 partitions: no masked partitions in the loop
#define AL_P1_12(ROW) ROW(1) ROW(2) ROW(3) ROW(4) ROW(5) ROW(6) ROW(7) ROW(8) ROW(9) ROW(10) ROW(11) ROW(12)
#define AL_REGS_ONE(P) AL_LOOP(1, 1, P, P, k_spectral_mac_static<12, P, 1>)
#define AL_REGS_PAIR(P) AL_LOOP(2, 2, P, P, k_spectral_mac_static<12, P, 2>)
#define AL_LDS_RING(P) AL_LOOP(2, 3, P, P, k_spectral_mac_static_lds<12, P>)
#define AL_LDS_DMA(P) AL_LOOP(2, 4, P, P, k_spectral_mac_static_glds<12, P>)
static const MacRow MAC_ROWS[] = {
    // tile shapes: accumulators for up to 24 output blocks, 4 or 12 partition spectra in registers
    // (sweep of other shapes: profiles/r01_mac_variants.txt)
    AL_TILE(12, 12, 2, true) AL_TILE(8, 12, 1, false) AL_TILE(24, 4, 1, false) AL_TILE(8, 4, 1, false)
    AL_P1_12(AL_REGS_ONE) AL_P1_12(AL_REGS_PAIR) AL_P1_12(AL_LDS_RING) AL_P1_12(AL_LDS_DMA)
    // 13..16 partitions: two units of ceil(P/2) per capsule, 17..21: three units of ceil(P/3); always through LDS, always two
    // k-tiles per workgroup
    AL_LOOP(2, 3, 13, 14, k_spectral_mac_static_lds<12, 7, 2>) AL_LOOP(2, 3, 15, 16, k_spectral_mac_static_lds<12, 8, 2>)
    AL_LOOP(2, 4, 13, 14, k_spectral_mac_static_glds<12, 7, 2>) AL_LOOP(2, 4, 15, 16, k_spectral_mac_static_glds<12, 8, 2>)
    AL_LOOP(2, 4, 17, 18, k_spectral_mac_static_glds<12, 6, 3>) AL_LOOP(2, 4, 19, 21, k_spectral_mac_static_glds<12, 7, 3, true, 2>)
    AL_MOVING(12) AL_MOVING(AL_SPARSE_MAX_PARTITIONS)
};
#undef AL_TILE
#undef AL_LOOP
#undef AL_MOVING
#undef AL_P1_12
#undef AL_REGS_ONE
#undef AL_REGS_PAIR
#undef AL_LDS_RING
#undef AL_LDS_DMA

// the row reported under `code` (capsule-loop rows: 3120000 + D) that serves P partitions; nullptr: the library ships none
inline const MacRow *mac_row(int code, int P) {
  for (const MacRow &r : MAC_ROWS)
    if (r.code == code && (r.p_lo == 0 || (r.p_lo <= P && P <= r.p_hi))) return &r;
  return nullptr;
}

struct MacPlan {
  const MacRow *statics;   // capsule-loop kernel that takes the one-emitter events (nullptr: the tile kernel does)
  const MacRow *tile;      // k_spectral_mac instantiation (nullptr: not launched)
  const MacRow *moving;    // k_spectral_mac_moving instantiation (nullptr: not launched)
  dim3 static_grid, tile_grid, moving_grid;
  int static_code;         // what al_spectral_mac_variant reports for one-emitter events
};

inline MacPlan plan_mac(const al_batch *b) {
  MacPlan m{};
  const bool wide_k = b->max_blocks > 8, wide_p = b->n_partitions > 4;
  const int bins = 1 << b->log2_block, P = b->n_partitions;
  m.tile = mac_row(wide_k && wide_p && bins >= 512 ? 1121202 : wide_k ? 240401 : wide_p ? 81201 : 80401, P);
  m.tile_grid = dim3(bins / (256 * m.tile->vb), b->n_capsules * (m.tile->ksplit ? (b->max_blocks + m.tile->kt - 1) / m.tile->kt : 1),
                     b->n_events);
  // moving events flagged by the planner (al_event.reserved == 1: every stream has n_j <= AL_SPARSE_MAX_NJ)
  if (b->n_streams > b->n_events && P <= AL_SPARSE_MAX_PARTITIONS)
    m.moving = mac_row(100 * AL_SPARSE_MAX_NJ + (P <= 12 ? 12 : AL_SPARSE_MAX_PARTITIONS), P);
  m.moving_grid = dim3(bins / 256, b->n_capsules, b->n_events);
  m.static_code = m.tile->code;
  if (static_mac_active(*b)) {
    // enough workgroups to fill the chip: split the capsule loop for small batches
    const int n_ktiles = (b->max_blocks + 11) / 12, base = (bins / 512) * n_ktiles * b->n_events;
    int n_cs = 1;
    while (n_cs < b->n_capsules && base * n_cs < 1024) n_cs *= 2;
    if (n_cs > b->n_capsules) n_cs = b->n_capsules;
    const bool pair = n_ktiles > 1 && !(b->flags & AL_FLAG_MAC_ONE_KTILE);
    const int n_pairs = (n_ktiles + 1) / 2;
    int digit;   // D of the code
    // 13..21 partitions: fed by LDS-DMA (k_spectral_mac_static_glds: no staging registers, so the 32-block signal window
    // of 21 partitions fits; profiles/r03_p24_ab.txt) when the batch has an all-zero block for the rows past an odd count,
    // else (13..16 only) by the register-staged ring of k_spectral_mac_static_lds.
    if (P > 12) digit = b->hspec_zero_block >= 0 ? 4 : 3;
    else if (pair && n_pairs > 1 && !(b->flags & AL_FLAG_MAC_NO_LDS_RING)) digit = 3;
    else digit = pair ? 2 : 1;
    // at most 12 partitions through the LDS-DMA kernel too (2 % slower there than the register / register-staged versions:
    // the accumulate of short IRs is not short of flight time, profiles/r03_p24_ab.txt)
    if ((b->flags & AL_FLAG_MAC_LDS_DMA) && P <= 12 && digit >= 2) digit = 4;
    m.statics = mac_row(3120000 + digit, P);
    if (m.statics) {
      const int nktw = m.statics->threads / 256;   // k-tiles per workgroup
      m.static_grid = dim3(bins / 512, (n_ktiles + nktw - 1) / nktw, b->n_events * n_cs);
    }
    m.static_code = 3120000 + 100 * P + digit;
    if (b->flags & AL_FLAG_ONLY_STATIC) m.tile = m.moving = nullptr;   // no event is left for the other kernels
  }
  return m;
}

}  // namespace al
