// Shoebox room impulse responses by the image-source method (Allen & Berkley 1979), generated in HBM in the (C, N, pitch) layout
// Renderer.prepare reads.  The definition is in DESIGN.md "Shoebox IRs" and in include/audiblelight_hip.h (al_ism_shoebox).
//
// Per axis an image is numbered by one integer q = 2 m - p (p = q & 1): image q lies in mirror cell q, its coordinate grows with q,
// and it has been reflected |q| times (k0 = |m - p| times by the wall at 0, k1 = |m| times by the wall at L).  The CANONICAL ORDER of
// the images of a (capsule, source) pair is lexicographic in (qx, qy, qz); every output sample is the float64 sum of its taps in
// that order, rounded to float32 once.  Nothing is scattered and nothing is atomic: the kernel GATHERS.
//
// ism_gather  THE ONE IMAGE GATHER, behind k_ism_shoebox, k_ism_shoebox_dir and k_ism_bands (al_ism_bands.h): one workgroup of ONE WAVE
//   per (pair or position, tile of ISM_TILE samples), ISM_PER_LANE samples per lane (lane, lane + 64, ...), the accumulators float64
//   registers.  (One wave: the __syncthreads() below order LDS traffic only, hipcc emits no barrier instruction for them, and no
//   wave can be out of step with another.)  A kernel decodes blockIdx, writes its pad or empty tiles, hands the gather its tile as
//   (s_lo, t_hi, s_end) with its LDS, and stores what the gather accumulated; a small VARIANT type says which images are dead, what a
//   list entry carries and how it is filled (IsmOmni, IsmDir<K>, IsmBands<NB>).
//   The images that can reach the tile lie in the shell d_lo < |R| < d_hi.  The wave walks the lattice COLUMNS (qx, qy) in
//   order, ISM_THREADS at a time, lane k taking column base + k:
//     1. the lane bounds the column's qz by the shell (at most two runs: below and above the inner sphere; a column wholly inside the
//        inner sphere, outside the outer one or beyond max_order has none) and counts the images of those runs that touch the tile
//        (the exact test, on the image's own rint(tau): the runs are only a superset);
//     2. an exclusive prefix sum of the counts over the wave (suffix sums by __shfl_down, the total through LDS);
//     3. the lane walks its runs again and writes its touching images to the LDS list at its offset: the list is in canonical order.
//        A list longer than the variant's window (ISM_LIST, ISM_DIR_LIST) goes in windows, in order;
//     4. every lane then adds the taps of the list's images that reach ITS samples, in list order.
//   The order of a sample's sum depends on the room and the pair alone, never on the grid, the other pairs or the list size.
// A tap costs one LDS entry, two table reads and a division: sin(pi (t - tau)) = -(-1)^j sin(pi f) and the window's cosine by the
// angle sum over a table of cos / sin(2 pi j / 81), with t0 = rint(tau), f = tau - t0 (exact) and j = t - t0.
// All geometry, tau, the tap weight and the accumulator are float64.
//
// THE DIFFUSE TAIL (al_ism_shoebox_tail; DESIGN.md "Shoebox IRs: the diffuse tail").  Past a mixing sample M the row continues as
// seeded Gaussian noise under an envelope e(t) read from a table of log-amplitude knots, one per ISM_TILE samples; between M and
// M + F the two are cross-faded with cos / sin(pi x / 2), x = (t - M) / F.  Sample t of row (c, n) draws normal t % 4 of the
// Philox-4x32-10 block with counter (t / 4, source_id0 + n, ISM_TAIL_TAG, capsule_id0 + c) and key (seed lo, seed hi): a pure
// function of the seed, the two ids and t, so a row's bits do not depend on the call it is generated in.  Two kernels share a row:
//   k_ism_shoebox<true>  the tiles below SPLIT = ceil((M + F) / ISM_TILE) * ISM_TILE.  The image search ends at min(ir_len, M + F)
//     (the images past it are never visited: that is the whole saving), the epilogue applies the fade and adds the noise term, a
//     Philox block per sample (at most F + ISM_TILE such samples per row).  A sample at or below M is the image sum alone
//     (w_e = 1, w_l = 0 exactly, no noise term formed): with M >= ir_len the bits are those of k_ism_shoebox<false>.
//   k_ism_tail  every sample at or past SPLIT, pad included: w_l = 1 there, so out = (float)(e(t) g(t)).  A lane takes four
//     consecutive samples (one Philox block, one knot interval since 4 divides ISM_TILE) and writes them with one 16-byte store;
//     a workgroup takes ISM_TAIL_SPAN consecutive samples of one row.  No LDS, no barrier, no atomics; the only global reads are
//     the two knots.  e(t) = exp((1 - p) ln_env[k] + p ln_env[k + 1]) in float64 (p == 0 reads knot k alone, so a table of -inf
//     gives zeros and not 0 * inf); the quad's later three samples are e(t) times powers of exp((ln_env[k + 1] - ln_env[k]) / 256),
//     two exp per quad instead of four (a few float64 ulp from the definition, ten orders below the draw's tolerance).
// Every output sample is written exactly once per call by exactly one of the two kernels; out is never read.
//
// THE SOURCE SIDE (al_ism_shoebox_src; DESIGN.md "Shoebox IRs: directional sources and air").  Source n may carry a first-order pattern
// spat[n] = (w, vx, vy, vz) in room axes and the call an air coefficient m >= 0 in Np/m: the amplitude of an image becomes
// a gs exp(-m d), gs = w + v . e, where e is the direction in which the ray LEAVES the real source: e_i = -(-1)^{q_i} R_i / d, since
// each of the |q_i| reflections on axis i flips component i and the direct path leaves along -R / d.  The kernels with SRC set take
// the source-aware variants (IsmOmniSrc, IsmDirSrc<K>; IsmBandsSrc<NB> in al_ism_bands.h), which differ from the plain ones in
// `fill` alone: gs from the parities of im.qx / qy / qz and R / d (one division: w + (v . (sigma R)) / d), through a pointer that is
// uniform over the wave (n comes from blockIdx), and -m d added to the exponent of the wall gain: no further exp.  Where an entry
// carries gains, gs is written to the entry's `a` and read back behind a compiler barrier (ism_park), so that it is not live while
// the exp is evaluated.  The omni pattern (or a null table) and m = 0 give gs = 1 + 0 / d = 1 and exp(x - 0) = exp(x): the bits of
// the plain kernels.  With a tail every (row, source) pair reads a knot table of its own
// (IsmTail::env_src_stride).  The instantiations without SRC are the kernels as they were.
//
// THE HOST SIDE.  The five point-receiver entries (al_ism_shoebox, _tail, _dir, _dir_tail, _src) share ism_images_prepare, which
// turns their arguments into the kernels' job (no pattern table: omni capsules; null source patterns and air 0: no source side;
// mix < 0: no tail), and launch_ism_images, which picks the image kernel by (patterns, K, TAIL, SRC) and adds k_ism_tail.  An entry
// states what it requires beyond that.  ism_prepare is the part every shoebox entry shares (al_ism_bands.h and al_ism_sphere.h call
// it too), ism_tail_prepare and ism_source_prepare the tail's and the source side's.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "al_common.h"
#include "al_rng.h"
#include "al_status.h"

namespace al {

constexpr int ISM_THREADS = 64;   // one wave
constexpr int ISM_PER_LANE = 4;
constexpr int ISM_TILE = ISM_THREADS * ISM_PER_LANE;   // samples per workgroup
constexpr int ISM_HALF = 40;      // taps on either side of rint(tau): |t - tau| < 40.5
constexpr int ISM_TAPS = 2 * ISM_HALF + 1;
constexpr int ISM_LIST = 128;     // images per LDS list window (48 bytes each)
constexpr double ISM_MAX_HALF_WIDTH = 1048576.0;   // mirror cells per axis and side al_ism_shoebox accepts
constexpr uint32_t ISM_TAIL_TAG = 4u;                 // third counter word of the tail's draws: 1, 2 and 3 are the ambience's (al_rng.h)
constexpr int ISM_TAIL_THREADS = 256;
constexpr int ISM_TAIL_QUADS = 4;                     // 16-byte stores per lane of k_ism_tail, ISM_TAIL_THREADS quads apart
constexpr int ISM_TAIL_SPAN = ISM_TAIL_THREADS * 4 * ISM_TAIL_QUADS;   // samples per workgroup of k_ism_tail
constexpr uint32_t ISM_CTAIL_TAG = 5u;                // low byte of the third counter word of the coherent tail's draws: 5 + 256 p for plane wave p
constexpr int ISM_CTAIL_MAX_WAVES = 256, ISM_CTAIL_MAX_TAPS = 32;
constexpr int ISM_CTAIL_REACH = 256;                  // every tap of a table reads s(t - d) with -256 <= d <= 256
constexpr int ISM_CTAIL_THREADS = 64;                 // one wave, as the image kernels: its __syncthreads() order LDS traffic only
constexpr int ISM_CTAIL_PER_LANE = 8;                 // consecutive samples of a lane: two 16-byte stores per row
constexpr int ISM_CTAIL_TILE = ISM_CTAIL_THREADS * ISM_CTAIL_PER_LANE;   // samples per workgroup of k_ism_ctail
constexpr int ISM_CTAIL_WINDOW = ISM_CTAIL_TILE + 2 * ISM_CTAIL_REACH;   // draws of one plane wave a tile can read
constexpr int ISM_CTAIL_PLANE = ISM_CTAIL_WINDOW / ISM_CTAIL_PER_LANE;   // words of one of the window's eight planes
constexpr int ISM_CTAIL_CHUNK = 4;                    // plane waves in LDS at a time: 4 x 1024 x 4 B = 16 KiB, ten workgroups per CU
constexpr int ISM_CTAIL_ROWS = 8;                     // rows of the group per workgroup: 64 float64 accumulators per lane

// the diffuse tail of a row (all zero for al_ism_shoebox)
struct IsmTail {
  const double *ln_env;   // n_knots log-amplitude knots (device), knot k at sample ISM_TILE k
  int64_t mix, fade;      // M, F
  int32_t y_end;          // min(ir_len, M + F): the image sum is needed below it only
  int32_t split;          // ceil((M + F) / ISM_TILE) * ISM_TILE, at most pitch rounded up to ISM_TILE: k_ism_tail owns [split, pitch)
  int32_t tail_blocks;    // workgroups of k_ism_tail per row
  uint32_t seed_lo, seed_hi, source_id0, capsule_id0;
  uint32_t env_stride;    // knots between the tables of two rows c (al_ism_shoebox_dir_tail: n_knots); 0: one table serves every row
  uint32_t env_src_stride;   // knots between the tables of two sources n (al_ism_shoebox_src: n_knots); 0: one table serves every source
  // the coherent tail (al_ism_shoebox_coherent; null and 0 for every other entry)
  const double *taps;        // (rows, n_waves, n_taps), device
  const int32_t *delays;     // (rows, n_waves), device
  int32_t n_waves, n_taps;   // P, J
  uint32_t group_id;
  int32_t ctail_blocks;      // workgroups of k_ism_ctail per (source, block of ISM_CTAIL_ROWS rows)
};

struct IsmJob {
  const double *sources, *capsules;   // (N, 3), (C, 3)
  float *out;                         // (C, N, pitch)
  int32_t n_sources, n_capsules, ir_len, pitch, max_order, n_tiles;
  double L[3], ln_beta[6];            // ln_beta: 0 where beta == 0 (see beta_zero)
  int32_t beta_zero[6];
  double c, fs;
  IsmTail tail;
  const double *source_patterns;   // (N, 4), device; null: omni sources.  Read by the SRC kernels only
  double air;                      // m of al_ism_shoebox_src, Np/m
};

struct alignas(16) IsmEntry {
  double f, g, a, c81, s81;   // tau - t0; -a sin(pi f) / (2 pi); amplitude; cos, sin(2 pi f / 81)
  int32_t t0, reserved;
};

// image q of an axis: m and p of the definition
__device__ __forceinline__ void ism_mp(int q, int &m, int &p) {
  p = q & 1;
  m = (q + p) / 2;   // q + p is even
}
__device__ __forceinline__ double ism_offset(int q, double s, double r, double L) {
  int m, p;
  ism_mp(q, m, p);
  return (double)(1 - 2 * p) * s + 2.0 * (double)m * L - r;
}
// reflections of image q of an axis by its wall at 0 and its wall at L
__device__ __forceinline__ void ism_counts(int q, int &k0, int &k1) {
  int m, p;
  ism_mp(q, m, p);
  k0 = abs(m - p);
  k1 = abs(m);
}
// k0 ln(beta0) + k1 ln(beta1) of an axis (ln_beta: the axis's two entries, 0 where beta == 0)
__device__ __forceinline__ double ism_log_gain(int q, const double *ln_beta) {
  int k0, k1;
  ism_counts(q, k0, k1);
  return (double)k0 * ln_beta[0] + (double)k1 * ln_beta[1];
}
// image q of an axis is alive unless it has hit a wall of beta == 0 (zero: the axis's two flags)
__device__ __forceinline__ bool ism_alive(int q, const int32_t *zero) {
  int k0, k1;
  ism_counts(q, k0, k1);
  return !((k0 > 0 && zero[0]) || (k1 > 0 && zero[1]));
}

// the qz of a column, as two runs [a1, b1] and [a2, b2] (empty when a > b)
struct IsmColumn {
  double rho2;
  int a1, b1, a2, b2;
};

// an image that touches the tile, as a variant's fill sees it
struct IsmImage {
  int qx, qy, qz;
  unsigned alive;   // the variant's mask of the image: alive(0, qx) & alive(1, qy) & alive(2, qz), never 0
  double Rx, Ry, Rz, d, tau;
  int t0;           // rint(tau)
};

__device__ __forceinline__ int ism_clamp(double v, int lo, int hi) { return v < (double)lo ? lo : v > (double)hi ? hi : (int)v; }

// e(t) of the tail: the knot table interpolated in the logarithm, float64
__device__ __forceinline__ double ism_envelope(const double *ln_env, int t) {
  const int k = t / ISM_TILE, r = t % ISM_TILE;
  if (r == 0) return exp(ln_env[k]);
  const double p = (double)r / (double)ISM_TILE;
  return exp((1.0 - p) * ln_env[k] + p * ln_env[k + 1]);
}
// the four normals of samples 4 q .. 4 q + 3 of row (cap, n)
__device__ __forceinline__ float4 ism_tail_normal4(const IsmTail &tail, int q, int n, int cap) {
  const Philox4 p = philox4x32_10((uint32_t)q, tail.source_id0 + (uint32_t)n, ISM_TAIL_TAG, tail.capsule_id0 + (uint32_t)cap, tail.seed_lo,
                                  tail.seed_hi);
  const float2 a = box_muller(p.x, p.y), b = box_muller(p.z, p.w);
  return make_float4(a.x, a.y, b.x, b.y);
}

// draw ts of row (cap, n): normal ts % 4 of the block of samples 4 (ts / 4) ..
__device__ __forceinline__ float ism_tail_normal(const IsmTail &tail, int ts, int n, int cap) {
  const float4 g4 = ism_tail_normal4(tail, ts >> 2, n, cap);
  return (ts & 2) ? ((ts & 1) ? g4.w : g4.z) : ((ts & 1) ? g4.y : g4.x);
}
// the fade weights of a sample ts > M: cos, sin(pi x / 2) with x = (ts - M) / F; (0, 1) from M + F on
__device__ __forceinline__ void ism_fade(const IsmTail &tail, int ts, double &w_e, double &w_l) {
  const double x = ((double)ts - (double)tail.mix) / (double)tail.fade;
  w_e = 0.0, w_l = 1.0;
  if (x < 1.0) sincospi(0.5 * x, &w_l, &w_e);
}

// THE COHERENT TAIL (al_ism_shoebox_coherent; DESIGN.md "Shoebox IRs: the coherent tail").  g(t) of row `row` and source n is a sum of
// P plane waves shared by the rows of the call: g = sum_p sum_j taps[row][p][j] s_{n,p}(t - delays[row][p] - j), p ascending outside,
// j ascending inside, one fma per term into a float64 accumulator that starts at 0.  s_{n,p}(m) is normal m & 3 of the Philox block
// ((uint32)(m >> 2), source_id0 + n, 5 + 256 p, group_id): m may be negative, and its counter word then wraps to one no sample index
// reaches.  Two paths form the same sum in the same order from the same float32 normals, so their bits agree:
//   ism_ctail_g   one sample, the blocks regenerated as it goes (the image kernels' epilogue: the faded samples below the split);
//   k_ism_ctail   every sample from the split on.  One workgroup of one wave per (source, tile of ISM_CTAIL_TILE samples, block of
//     ISM_CTAIL_ROWS rows): the draws of ISM_CTAIL_CHUNK plane waves over the tile's window go to LDS once and every row of the block
//     reads them, each lane sliding the n_taps + 7 words its eight samples need through registers.
// the four normals s(4 q) .. s(4 q + 3) of plane wave p for source n
__device__ __forceinline__ float4 ism_ctail_normal4(const IsmTail &tail, uint32_t q, int n, int p) {
  const Philox4 x = philox4x32_10(q, tail.source_id0 + (uint32_t)n, ISM_CTAIL_TAG + 256u * (uint32_t)p, tail.group_id, tail.seed_lo, tail.seed_hi);
  const float2 a = box_muller(x.x, x.y), b = box_muller(x.z, x.w);
  return make_float4(a.x, a.y, b.x, b.y);
}
__device__ __forceinline__ double ism_ctail_g(const IsmTail &tail, int row, int n, int t) {
  const int P = tail.n_waves, J = tail.n_taps;
  double g = 0.0;
  for (int p = 0; p < P; ++p) {
    const int64_t wave = (int64_t)row * P + p;
    const double *taps = tail.taps + wave * J;
    int64_t m = (int64_t)t - tail.delays[wave];
    int64_t have = m >> 2;
    float4 s4 = ism_ctail_normal4(tail, (uint32_t)have, n, p);
    for (int j = 0; j < J; ++j, --m) {
      if ((m >> 2) != have) {
        have = m >> 2;
        s4 = ism_ctail_normal4(tail, (uint32_t)have, n, p);
      }
      const float s = (m & 2) ? ((m & 1) ? s4.w : s4.z) : ((m & 1) ? s4.y : s4.x);
      g = fma(taps[j], (double)s, g);
    }
  }
  return g;
}

// what every list entry holds beside its gains: the tap's shape of an image of amplitude a
template <class Entry>
__device__ __forceinline__ void ism_fill_shape(Entry &e, const IsmImage &im, double a) {
  double sp, cp, s81, c81;
  const double f = im.tau - (double)im.t0;
  sincospi(f, &sp, &cp);
  sincospi(2.0 * f / (double)ISM_TAPS, &s81, &c81);
  e.t0 = im.t0;
  e.reserved = 0;
  e.f = f;
  e.a = a;
  e.g = -0.5 * a * sp / M_PI;
  e.s81 = s81;
  e.c81 = c81;
}

// THE GATHER: steps 1 to 4 of the header comment for the tile of samples [s_lo, s_lo + ISM_TILE) cut at s_end (t_hi: its last
// sample), of source n at receiver position pos.  s_lo may be negative (k_ism_bands).  Lane k adds into acc[s][g] the taps of
// sample s_lo + k + 64 s under gain g, in canonical order.  The variant V says what differs between the kernels:
//   V::NG, V::Entry, V::LIST   gains per image (0: none, the tap is added as it is), the list entry (f, g, a, c81, s81, t0 and
//                              gain[NG]) and the entries per list window;
//   v.alive(axis, q)           a bit mask, bit k clear when image q of the axis has hit a wall that is dead for gain k; an image
//                              whose three masks have no common bit is left out of the list;
//   v.fill(e, im)              list entry e of image im.
// list (V::LIST entries), win_c, win_s (ISM_TAPS each) and wave_total (2) are the kernel's LDS.
template <class V>
__device__ __forceinline__ void ism_gather(const IsmJob &job, const V &v, int n, int pos, int s_lo, int t_hi, int s_end,
                                           typename V::Entry *list, double *win_c, double *win_s, int *wave_total,
                                           double (&acc)[ISM_PER_LANE][V::NG > 0 ? V::NG : 1]) {
  constexpr int NG = V::NG, LIST = V::LIST;
  const int tid = threadIdx.x, lane = tid, t = s_lo + tid;
  // cos, sin(2 pi j / 81), j = -40 .. 40
  for (int i = tid; i < ISM_TAPS; i += ISM_THREADS) sincospi(2.0 * (double)(i - ISM_HALF) / (double)ISM_TAPS, &win_s[i], &win_c[i]);

  const double sx = job.sources[3 * n], sy = job.sources[3 * n + 1], sz = job.sources[3 * n + 2];
  const double rx = job.capsules[3 * pos], ry = job.capsules[3 * pos + 1], rz = job.capsules[3 * pos + 2];
  const double Lx = job.L[0], Ly = job.L[1], Lz = job.L[2];
  // the shell of this tile, a sample wider than the taps reach on either side
  const double d_hi = (double)(t_hi + ISM_HALF + 2) * job.c / job.fs, d_lo = (double)(s_lo - ISM_HALF - 2) * job.c / job.fs;
  const double hi2 = d_hi * d_hi, lo2 = d_lo > 0.0 ? d_lo * d_lo : 0.0;
  const int order = job.max_order;
  int Qx = ism_clamp(floor(d_hi / Lx) + 1.0, 0, (int)ISM_MAX_HALF_WIDTH), Qy = ism_clamp(floor(d_hi / Ly) + 1.0, 0, (int)ISM_MAX_HALF_WIDTH),
      Qz = ism_clamp(floor(d_hi / Lz) + 1.0, 0, (int)ISM_MAX_HALF_WIDTH);
  if (order >= 0) {
    Qx = min(Qx, order);
    Qy = min(Qy, order);
    Qz = min(Qz, order);
  }
  const int64_t ny = 2 * (int64_t)Qy + 1, n_columns = (2 * (int64_t)Qx + 1) * ny;

  // does image qz of column `col` touch the tile?  Rz, t0, tau and d of the image either way
  auto touches = [&](const IsmColumn &col, int qz, double &Rz, double &d, double &tau, int &t0) {
    Rz = ism_offset(qz, sz, rz, Lz);
    d = sqrt(col.rho2 + Rz * Rz);
    tau = d * job.fs / job.c;
    if (!(tau < 2.0e9) || !(d > 0.0)) return false;
    t0 = (int)rint(tau);
    return t0 + ISM_HALF >= s_lo && t0 - ISM_HALF <= t_hi;
  };

  int parity = 0;
  for (int64_t base = 0; base < n_columns; base += ISM_THREADS, parity ^= 1) {
    // 1. this lane's column
    const int64_t ci = base + tid;
    IsmColumn col;
    col.a1 = col.a2 = 0;
    col.b1 = col.b2 = -1;
    unsigned alive_xy = 0;   // the gains for which the column is alive
    if (ci < n_columns) {
      const int qx = (int)(ci / ny) - Qx, qy = (int)(ci % ny) - Qy;
      const int k_xy = abs(qx) + abs(qy);
      const double Rx = ism_offset(qx, sx, rx, Lx), Ry = ism_offset(qy, sy, ry, Ly);
      col.rho2 = Rx * Rx + Ry * Ry;
      if ((order < 0 || k_xy <= order) && col.rho2 < hi2) {
        alive_xy = v.alive(0, qx) & v.alive(1, qy);
        const int Kz = order < 0 ? Qz : min(Qz, order - k_xy);
        const double z_max = sqrt(hi2 - col.rho2);
        // image qz lies in (qz Lz, (qz + 1) Lz): one cell of margin on either side
        col.a1 = ism_clamp(floor((rz - z_max) / Lz) - 1.0, -Kz, Kz);
        const int top = ism_clamp(floor((rz + z_max) / Lz) + 1.0, -Kz, Kz);
        col.b1 = top;   // one run, unless the inner sphere cuts it in two
        if (lo2 > col.rho2) {   // the cells wholly inside the inner sphere are left out
          const double z_min = sqrt(lo2 - col.rho2);
          const double ea = ceil((rz - z_min) / Lz) + 1.0, eb = floor((rz + z_min) / Lz) - 2.0;
          if (ea <= eb) {
            col.b1 = ism_clamp(ea - 1.0, -Kz - 1, Kz);
            col.a2 = ism_clamp(eb + 1.0, -Kz, Kz + 1);
            col.b2 = top;
          }
        }
      }
    }
    int count = 0;
    if (alive_xy) {
      double Rz, d, tau;
      int t0;
      for (int run = 0; run < 2; ++run)
        for (int qz = run ? col.a2 : col.a1, end = run ? col.b2 : col.b1; qz <= end; ++qz)
          if ((alive_xy & v.alive(2, qz)) && touches(col, qz, Rz, d, tau, t0)) ++count;
    }
    // 2. exclusive prefix sum of the counts: suffix sums by shuffles, the total (lane 0's) through LDS
    int suffix = count;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int other = __shfl_down(suffix, off, 64);
      if (lane + off < 64) suffix += other;
    }
    if (lane == 0) wave_total[parity] = suffix;
    __syncthreads();
    const int total = wave_total[parity], offset = total - suffix;
    // 3. + 4. the list, a window of LIST at a time
    for (int w0 = 0; w0 < total; w0 += LIST) {
      if (count > 0 && offset < w0 + LIST && offset + count > w0) {
        IsmImage im;
        im.qx = (int)(ci / ny) - Qx, im.qy = (int)(ci % ny) - Qy;
        // the column's Rx, Ry again (not kept across the gather: registers)
        im.Rx = ism_offset(im.qx, sx, rx, Lx), im.Ry = ism_offset(im.qy, sy, ry, Ly);
        int at = offset;
        for (int run = 0; run < 2; ++run)
          for (int qz = run ? col.a2 : col.a1, end = run ? col.b2 : col.b1; qz <= end; ++qz) {
            im.qz = qz;
            im.alive = alive_xy & v.alive(2, qz);
            if (!im.alive || !touches(col, qz, im.Rz, im.d, im.tau, im.t0)) continue;
            if (at >= w0 && at < w0 + LIST) v.fill(list[at - w0], im);
            ++at;
          }
      }
      __syncthreads();
      const int n_list = min(LIST, total - w0);
      for (int i = 0; i < n_list; ++i) {
        const int j0 = t - list[i].t0;   // of the lane's first sample; the others are 64 apart, so at most two are in reach
        if (j0 > ISM_HALF || j0 + (ISM_PER_LANE - 1) * ISM_THREADS < -ISM_HALF) continue;
        const typename V::Entry e = list[i];
#pragma unroll
        for (int s = 0; s < ISM_PER_LANE; ++s) {
          const int j = j0 + s * ISM_THREADS;
          if (j < -ISM_HALF || j > ISM_HALF || t + s * ISM_THREADS >= s_end) continue;
          const double u = (double)j - e.f;
          if (!(fabs(u) < 0.5 * (double)ISM_TAPS)) continue;
          double shape = e.a;   // the tap of the image without its gains, formed once for the NG of them
          if (u != 0.0) {
            const double window = 1.0 + (win_c[j + ISM_HALF] * e.c81 + win_s[j + ISM_HALF] * e.s81);
            shape = ((j & 1) ? -e.g : e.g) * window / u;
          }
          if constexpr (NG == 0) {
            acc[s][0] += shape;
          } else {
#pragma unroll
            for (int k = 0; k < NG; ++k) acc[s][k] += shape * e.gain[k];
          }
        }
      }
      __syncthreads();
    }
  }
}

// the walls of a job with one column of reflection coefficients (IsmJob::ln_beta, beta_zero): one bit, one amplitude
struct IsmWalls {
  const IsmJob &job;
  __device__ __forceinline__ unsigned alive(int axis, int q) const { return ism_alive(q, job.beta_zero + 2 * axis) ? 1u : 0u; }
  __device__ __forceinline__ double amplitude(const IsmImage &im) const {
    const double ln_xy = ism_log_gain(im.qx, job.ln_beta) + ism_log_gain(im.qy, job.ln_beta + 2), ln_z = ism_log_gain(im.qz, job.ln_beta + 4);
    return exp(ln_xy + ln_z) / (4.0 * M_PI * im.d);
  }
};

// the omnidirectional variant: no gains, 48-byte entries
struct IsmOmni : IsmWalls {
  static constexpr int NG = 0, LIST = ISM_LIST;
  using Entry = IsmEntry;
  __device__ __forceinline__ void fill(Entry &e, const IsmImage &im) const { ism_fill_shape(e, im, amplitude(im)); }
};

// the source of a workgroup: its pattern (null: omni) behind a pointer that is uniform over the wave, so it lives in scalar registers
struct IsmSource {
  const double *spat;
  // gs = w + v . e, e_i = -(-1)^{q_i} R_i / d: the direction in which the image's ray leaves the real source
  __device__ __forceinline__ double gain(const IsmImage &im) const {
    if (!spat) return 1.0;
    const double sx = (im.qx & 1) ? im.Rx : -im.Rx, sy = (im.qy & 1) ? im.Ry : -im.Ry, sz = (im.qz & 1) ? im.Rz : -im.Rz;   // e d
    return spat[0] + (spat[1] * sx + spat[2] * sy + spat[3] * sz) / im.d;   // one division, not three
  }
  // the same from u = R / d, where a variant has formed it already
  __device__ __forceinline__ double gain(const IsmImage &im, double ux, double uy, double uz) const {
    if (!spat) return 1.0;
    return spat[0] + (spat[1] * ((im.qx & 1) ? ux : -ux) + spat[2] * ((im.qy & 1) ? uy : -uy) + spat[3] * ((im.qz & 1) ? uz : -uz));
  }
};
__device__ __forceinline__ IsmSource ism_source(const IsmJob &job, int n) {
  return IsmSource{job.source_patterns ? job.source_patterns + 4 * (int64_t)n : nullptr};
}
// IsmWalls::amplitude through air of coefficient m: exp(sum k ln beta - m d) / (4 pi d)
__device__ __forceinline__ double ism_air_amplitude(const IsmJob &job, const IsmImage &im) {
  const double ln_xy = ism_log_gain(im.qx, job.ln_beta) + ism_log_gain(im.qy, job.ln_beta + 2), ln_z = ism_log_gain(im.qz, job.ln_beta + 4);
  return exp((ln_xy + ln_z) - job.air * im.d) / (4.0 * M_PI * im.d);
}
// the list entry keeps a value that was written to it out of the registers until it is read back (a compiler barrier, no instruction)
__device__ __forceinline__ void ism_park() { asm volatile("" ::: "memory"); }

// IsmOmni with a source pattern and air
struct IsmOmniSrc : IsmWalls {
  static constexpr int NG = 0, LIST = ISM_LIST;
  using Entry = IsmEntry;
  IsmSource src;
  __device__ __forceinline__ void fill(Entry &e, const IsmImage &im) const { ism_fill_shape(e, im, ism_air_amplitude(job, im) * src.gain(im)); }
};

// the knot table of row c and source n (both strides 0: the one table of al_ism_shoebox_tail)
__device__ __forceinline__ const double *ism_tail_table(const IsmTail &tail, int c, int n) {
  return tail.ln_env + ((int64_t)c * tail.env_stride + (int64_t)n * tail.env_src_stride);
}

// COH: the noise term of the epilogue is the coherent tail's (TAIL and SRC set: al_ism_shoebox_coherent takes the arguments of _src)
template <bool TAIL, bool SRC = false, bool COH = false>
__global__ __launch_bounds__(ISM_THREADS) void k_ism_shoebox(IsmJob job) {
  __shared__ IsmEntry list[ISM_LIST];
  __shared__ double win_c[ISM_TAPS], win_s[ISM_TAPS];
  __shared__ int wave_total[2];
  const int tid = threadIdx.x;
  const int tile = (int)(blockIdx.x % (unsigned)job.n_tiles);
  const int64_t pair = blockIdx.x / (unsigned)job.n_tiles;   // c * N + n
  const int n = (int)(pair % job.n_sources), cap = (int)(pair / job.n_sources);
  const int t_lo = tile * ISM_TILE, t = t_lo + tid;
  // the image sum is needed below y_end only: past the fade the row is the tail's
  const int y_end = TAIL ? job.tail.y_end : job.ir_len;
  const int t_hi = min(t_lo + ISM_TILE, y_end) - 1;
  float *row = job.out + pair * (int64_t)job.pitch;
  if (t_lo >= job.ir_len) {   // a tile of pad samples only
    for (int s = 0; s < ISM_PER_LANE; ++s)
      if (t + s * ISM_THREADS < job.pitch) row[t + s * ISM_THREADS] = 0.f;
    return;
  }
  double acc[ISM_PER_LANE][1] = {};
  if constexpr (SRC)
    ism_gather(job, IsmOmniSrc{{job}, ism_source(job, n)}, n, cap, t_lo, t_hi, y_end, list, win_c, win_s, wave_total, acc);
  else
    ism_gather(job, IsmOmni{{job}}, n, cap, t_lo, t_hi, y_end, list, win_c, win_s, wave_total, acc);
#pragma unroll
  for (int s = 0; s < ISM_PER_LANE; ++s) {
    const int ts = t + s * ISM_THREADS;
    if (ts >= job.pitch) continue;
    double v = acc[s][0];
    if constexpr (TAIL) {
      if (ts > job.tail.mix && ts < job.ir_len) {   // at or below M: w_e = 1, w_l = 0, the image sum as it is
        double w_e, w_l;
        ism_fade(job.tail, ts, w_e, w_l);
        const double *ln_env = SRC ? ism_tail_table(job.tail, cap, n) : job.tail.ln_env;   // SRC: a table per pair
        if constexpr (COH)
          v = w_e * v + w_l * ism_envelope(ln_env, ts) * ism_ctail_g(job.tail, cap, n, ts);
        else
          v = w_e * v + w_l * ism_envelope(ln_env, ts) * (double)ism_tail_normal(job.tail, ts, n, cap);
      }
    }
    row[ts] = ts < job.ir_len ? (float)v : 0.f;
  }
}

// the samples [split, pitch) of every row: envelope times noise, pad zeros; grid: tail_blocks workgroups per pair
__global__ __launch_bounds__(ISM_TAIL_THREADS) void k_ism_tail(IsmJob job) {
  const int block = (int)(blockIdx.x % (unsigned)job.tail.tail_blocks);
  const int64_t pair = blockIdx.x / (unsigned)job.tail.tail_blocks;
  const int n = (int)(pair % job.n_sources), cap = (int)(pair / job.n_sources);
  float *row = job.out + pair * (int64_t)job.pitch;
  const int64_t t_first = (int64_t)job.tail.split + (int64_t)block * ISM_TAIL_SPAN + 4 * (int)threadIdx.x;
#pragma unroll
  for (int i = 0; i < ISM_TAIL_QUADS; ++i) {
    const int64_t t64 = t_first + (int64_t)i * (4 * ISM_TAIL_THREADS);
    if (t64 >= job.pitch) return;   // pitch is a multiple of 4: a quad is inside the row or outside it
    const int t = (int)t64;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t < job.ir_len) {
      const float4 g = ism_tail_normal4(job.tail, t >> 2, n, cap);
      const int k = t / ISM_TILE, r = t % ISM_TILE;   // r + 3 < ISM_TILE: the quad lies in one knot interval
      const double *ln_env = ism_tail_table(job.tail, cap, n);   // the row's own table, the source's with al_ism_shoebox_src
      const double a = ln_env[k], b = ln_env[k + 1];
      const double inv = 1.0 / (double)ISM_TILE, p = (double)r * inv, step = (b - a) * inv;
      const double e0 = exp(r == 0 ? a : (1.0 - p) * a + p * b);
      double e1, e2, e3;
      if (fabs(step) < 1.0) {   // ln e is linear in t between two knots: one more exp serves the quad, e(t + 1) = e(t) exp(step)
        const double q = exp(step);
        e1 = e0 * q;
        e2 = e1 * q;
        e3 = e2 * q;
      } else {   // a knot of -inf, a table that is not finite or one that leaps: every sample as the definition has it
        const double p1 = (double)(r + 1) * inv, p2 = (double)(r + 2) * inv, p3 = (double)(r + 3) * inv;
        e1 = exp((1.0 - p1) * a + p1 * b);
        e2 = exp((1.0 - p2) * a + p2 * b);
        e3 = exp((1.0 - p3) * a + p3 * b);
      }
      v.x = (float)(e0 * (double)g.x);
      if (t + 1 < job.ir_len) v.y = (float)(e1 * (double)g.y);
      if (t + 2 < job.ir_len) v.z = (float)(e2 * (double)g.z);
      if (t + 3 < job.ir_len) v.w = (float)(e3 * (double)g.w);
    }
    *reinterpret_cast<float4 *>(row + t) = v;
  }
}

// one (row, plane wave) of k_ism_ctail: the lane's eight accumulators take the J taps tp[0 .. J) in order.  planes: the plane wave's
// window, word u at planes[(u & 7) * PLANE + (u >> 3)]; first: the word of s(t - D) of the lane's first sample WITHOUT the lane's
// 8 lane (uniform over the wave, so the plane and the offset of every word are scalar and the lanes read consecutive LDS words: no
// bank conflict).  The n_taps + 7 words slide through eight float64 registers, each converted once: a tap costs one LDS word, one
// conversion and eight fma.  JT: n_taps when it is known at compile time (the loop unrolls and the taps come in one scalar load),
// 0: J of the call.
template <int JT>
__device__ __forceinline__ void ism_ctail_wave(const float *planes, const double *__restrict__ tp, int first, int J, int lane,
                                               double (&acc)[ISM_CTAIL_PER_LANE]) {
  auto word = [&](int u) { return (double)planes[(u & 7) * ISM_CTAIL_PLANE + (u >> 3) + lane]; };
  double x[ISM_CTAIL_PER_LANE];
#pragma unroll
  for (int i = 0; i < ISM_CTAIL_PER_LANE; ++i) x[i] = word(first + i);
  const int n_taps = JT ? JT : J;
#pragma unroll
  for (int j = 0; j < n_taps; ++j) {
    const double a = tp[j];
#pragma unroll
    for (int i = 0; i < ISM_CTAIL_PER_LANE; ++i) acc[i] = fma(a, x[i], acc[i]);
#pragma unroll
    for (int i = ISM_CTAIL_PER_LANE - 1; i > 0; --i) x[i] = x[i - 1];
    if (j + 1 < n_taps) x[0] = word(first - (j + 1));
  }
}

// the samples [split, pitch) of every row under the coherent tail: envelope times g(t), pad zeros.  grid: ctail_blocks tiles per
// (source, block of ISM_CTAIL_ROWS rows), ONE WAVE each (the __syncthreads() below order LDS traffic only, as in ism_gather).  The
// window of plane wave p holds s_{n,p}(m) for m in [tile - 256, tile + 512 + 256): every m a table within its contract can ask for,
// word u = m - (tile - 256) in plane u & 7 (eight planes of WINDOW / 8 words: a lane owns eight consecutive samples for its 16-byte
// stores, and the planes keep the lanes' reads of one word apart by one LDS word, not eight).
__global__ __launch_bounds__(ISM_CTAIL_THREADS) void k_ism_ctail(IsmJob job) {
  __shared__ float win[ISM_CTAIL_CHUNK][ISM_CTAIL_PER_LANE][ISM_CTAIL_PLANE];
  const IsmTail &tail = job.tail;
  const int lane = threadIdx.x;
  const int tile = (int)(blockIdx.x % (unsigned)tail.ctail_blocks);
  const int64_t rest = blockIdx.x / (unsigned)tail.ctail_blocks;   // row block * N + n
  const int n = (int)(rest % job.n_sources), row0 = (int)(rest / job.n_sources) * ISM_CTAIL_ROWS;
  const int n_rows = min(ISM_CTAIL_ROWS, job.n_capsules - row0);
  const int P = tail.n_waves, J = tail.n_taps;
  const int64_t t_tile = (int64_t)tail.split + (int64_t)tile * ISM_CTAIL_TILE, t64 = t_tile + ISM_CTAIL_PER_LANE * lane;
  const int64_t w0 = t_tile - ISM_CTAIL_REACH;   // a multiple of 8: the split is one of ISM_TILE
  // the draws a sample below ir_len can read end REACH past the last of them
  const int64_t live = min((int64_t)ISM_CTAIL_TILE, (int64_t)job.ir_len - t_tile);
  const int n_quads = live > 0 ? (int)((live + 2 * ISM_CTAIL_REACH + 3) / 4) : 0;
  const bool mine = t64 < job.ir_len;   // the lane has a sample of the row (ir_len < 2^31: t64 fits an int then)
  const double *__restrict__ taps = tail.taps;
  const int32_t *__restrict__ delays = tail.delays;
  double acc[ISM_CTAIL_ROWS][ISM_CTAIL_PER_LANE] = {};
  for (int p0 = 0; p0 < P && n_quads > 0; p0 += ISM_CTAIL_CHUNK) {
    const int n_p = min(ISM_CTAIL_CHUNK, P - p0);
    for (int i = lane; i < n_p * n_quads; i += ISM_CTAIL_THREADS) {
      const int pp = i / n_quads, q = i % n_quads;   // words 4 q .. 4 q + 3: planes 4 (q & 1) .., offset q >> 1
      const float4 s4 = ism_ctail_normal4(tail, (uint32_t)((w0 >> 2) + q), n, p0 + pp);
      float *w = &win[pp][4 * (q & 1)][q >> 1];
      w[0] = s4.x;
      w[ISM_CTAIL_PLANE] = s4.y;
      w[2 * ISM_CTAIL_PLANE] = s4.z;
      w[3 * ISM_CTAIL_PLANE] = s4.w;
    }
    __syncthreads();
    if (mine) {
      for (int pp = 0; pp < n_p; ++pp) {
#pragma unroll
        for (int r = 0; r < ISM_CTAIL_ROWS; ++r) {
          if (r >= n_rows) continue;
          const int64_t wave = (int64_t)(row0 + r) * P + (p0 + pp);
          const int first = ISM_CTAIL_REACH - delays[wave];   // >= n_taps - 1 and <= 512 by the tables' contract
          if (J == 8)
            ism_ctail_wave<8>(&win[pp][0][0], taps + wave * 8, first, 8, lane, acc[r]);
          else
            ism_ctail_wave<0>(&win[pp][0][0], taps + wave * J, first, J, lane, acc[r]);
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int h = 0; h < ISM_CTAIL_PER_LANE / 4; ++h) {
    const int64_t tq = t64 + 4 * h;
    if (tq >= job.pitch) break;   // pitch is a multiple of 4: a quad is inside the row or outside it
    const int t = (int)tq;
#pragma unroll
    for (int r = 0; r < ISM_CTAIL_ROWS; ++r) {
      if (r >= n_rows) continue;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (t < job.ir_len) {
        const double *ln_env = ism_tail_table(tail, row0 + r, n);
        v.x = (float)(ism_envelope(ln_env, t) * acc[r][4 * h]);
        if (t + 1 < job.ir_len) v.y = (float)(ism_envelope(ln_env, t + 1) * acc[r][4 * h + 1]);
        if (t + 2 < job.ir_len) v.z = (float)(ism_envelope(ln_env, t + 2) * acc[r][4 * h + 2]);
        if (t + 3 < job.ir_len) v.w = (float)(ism_envelope(ln_env, t + 3) * acc[r][4 * h + 3]);
      }
      *reinterpret_cast<float4 *>(job.out + ((int64_t)(row0 + r) * job.n_sources + n) * (int64_t)job.pitch + t) = v;
    }
  }
}

// al_ism_shoebox's arguments as the kernel's job: 0 with *job filled, or the error of the first bad argument
inline int ism_prepare(const double *sources, int32_t n_sources, const double *capsules, int32_t n_capsules, const double *L,
                       const double *beta, double c, double fs, int32_t max_order, int32_t ir_len, int32_t pitch, float *out,
                       IsmJob *job) {
  if (!sources || !capsules || !L || !beta || !out) return fail(AL_E_BADARG, "al_ism_shoebox: null pointer");
  if (n_sources < 1 || n_capsules < 1) return fail(AL_E_BADARG, "al_ism_shoebox: n_sources and n_capsules must be >= 1");
  if (ir_len < 1) return fail(AL_E_BADARG, "al_ism_shoebox: ir_len must be >= 1");
  if (pitch < ir_len || (pitch & 3)) return fail(AL_E_BADARG, "al_ism_shoebox: pitch must be >= ir_len and a multiple of 4");
  if (max_order < -1) return fail(AL_E_BADARG, "al_ism_shoebox: max_order must be >= 0, or -1 for none");
  if (!isfinite(c) || !(c > 0.0) || !isfinite(fs) || !(fs > 0.0)) return fail(AL_E_BADARG, "al_ism_shoebox: c and fs must be finite and positive");
  for (int i = 0; i < 3; ++i) {
    if (!isfinite(L[i]) || !(L[i] > 0.0)) return fail(AL_E_BADARG, "al_ism_shoebox: room dimensions must be finite and positive");
    if (!(c * ((double)ir_len + 42.0) / fs / L[i] + 2.0 <= ISM_MAX_HALF_WIDTH))
      return fail(AL_E_BADARG, "al_ism_shoebox: c (ir_len + 42) / fs spans more than 2^20 mirror cells of the room");
    job->L[i] = L[i];
  }
  for (int i = 0; i < 6; ++i) {
    if (!(beta[i] >= 0.0 && beta[i] <= 1.0)) return fail(AL_E_BADARG, "al_ism_shoebox: reflection coefficients must be in [0, 1]");
    job->beta_zero[i] = beta[i] == 0.0;
    job->ln_beta[i] = beta[i] == 0.0 ? 0.0 : log(beta[i]);
  }
  job->n_tiles = (pitch + ISM_TILE - 1) / ISM_TILE;
  if ((int64_t)job->n_tiles * n_sources * n_capsules > 0x7fffffff)
    return fail(AL_E_BADARG, "al_ism_shoebox: more than 2^31 - 1 workgroups (tiles of 256 samples x pairs): split the call");
  job->sources = sources;
  job->capsules = capsules;
  job->out = out;
  job->n_sources = n_sources;
  job->n_capsules = n_capsules;
  job->ir_len = ir_len;
  job->pitch = pitch;
  job->max_order = max_order;
  job->c = c;
  job->fs = fs;
  job->tail = IsmTail{};
  job->source_patterns = nullptr;
  job->air = 0.0;
  return AL_OK;
}

// the sample at which the image sum of a row with a tail ends: min(ir_len, M + F), for any mix and fade >= 0 (no overflow)
inline int32_t ism_tail_y_end(int64_t mix, int64_t fade, int32_t ir_len) {
  return mix < ir_len && fade < ir_len && mix + fade < ir_len ? (int32_t)(mix + fade) : ir_len;
}

// the tail's arguments (mix >= 0: the entry or the prepare that calls this has seen to it) into a job ism_prepare has filled: the tail,
// the split, the two grids; one knot table for every row and source (the strides 0)
inline int ism_tail_prepare(int64_t mix, int64_t fade, uint64_t seed, int64_t source_id0, int64_t capsule_id0, const double *ln_env,
                            int32_t n_knots, IsmJob *job) {
  if (!ln_env) return fail(AL_E_BADARG, "al_ism_shoebox_tail: null envelope table");
  if (fade < 1) return fail(AL_E_BADARG, "al_ism_shoebox_tail: fade must be >= 1");
  if (source_id0 < 0 || capsule_id0 < 0) return fail(AL_E_BADARG, "al_ism_shoebox_tail: source_id0 and capsule_id0 must be >= 0");
  if (source_id0 + job->n_sources > 0x100000000ll || capsule_id0 + job->n_capsules > 0x100000000ll)
    return fail(AL_E_BADARG, "al_ism_shoebox_tail: source_id0 + n_sources and capsule_id0 + n_capsules must not exceed 2^32");
  if (n_knots != (job->ir_len - 1) / ISM_TILE + 2) return fail(AL_E_BADARG, "al_ism_shoebox_tail: n_knots must be (ir_len - 1) / 256 + 2");
  if (((uintptr_t)job->out & 15) != 0) return fail(AL_E_BADARG, "al_ism_shoebox_tail: out must be 16-byte aligned");
  const int64_t row_tiles = ((int64_t)job->pitch + ISM_TILE - 1) / ISM_TILE;
  const int64_t cap = row_tiles * ISM_TILE;
  IsmTail &tail = job->tail;
  tail.ln_env = ln_env;
  tail.mix = mix < cap ? mix : cap;   // a mix past the row is a mix at its end (and M + F cannot overflow)
  tail.fade = fade;
  tail.split = (int32_t)cap;
  tail.y_end = ism_tail_y_end(tail.mix, fade, job->ir_len);
  if (fade < cap && tail.mix + fade < cap) tail.split = (int32_t)((tail.mix + fade + ISM_TILE - 1) / ISM_TILE * ISM_TILE);
  tail.tail_blocks = tail.split < job->pitch ? (job->pitch - tail.split + ISM_TAIL_SPAN - 1) / ISM_TAIL_SPAN : 0;
  tail.seed_lo = (uint32_t)seed;
  tail.seed_hi = (uint32_t)(seed >> 32);
  tail.source_id0 = (uint32_t)source_id0;
  tail.capsule_id0 = (uint32_t)capsule_id0;
  job->n_tiles = (int32_t)(tail.split < job->pitch ? tail.split / ISM_TILE : row_tiles);   // k_ism_shoebox<true> stops at the split
  if ((int64_t)tail.tail_blocks * job->n_sources * job->n_capsules > 0x7fffffff)
    return fail(AL_E_BADARG, "al_ism_shoebox_tail: more than 2^31 - 1 workgroups (spans of 4096 samples x pairs): split the call");
  return AL_OK;
}

// DIRECTIONAL RECEIVERS (al_ism_shoebox_dir, al_ism_shoebox_dir_tail; DESIGN.md "Shoebox IRs: directional receivers").  A call takes
// P receiver positions with K <= 4 channels each and a pattern table pat[P][K][4] = (w, vx, vy, vz); row c = p K + k of the output
// is the image sum of position p with every amplitude multiplied by w + v . R / |R|.  The K channels of a position share every
// image, its delay and its 81 taps, so
//   k_ism_shoebox_dir<K, TAIL>  one workgroup of one wave per (position, source, tile) serves all K rows: ism_gather runs once,
//     a list entry carries the K gains beside what is common, and a lane forms the tap's shape once per (image, sample) and adds it
//     into K float64 accumulators: a channel costs a multiply-add per tap.  The list window is ISM_DIR_LIST = 96 entries of
//     48 + 8 K bytes (rounded to 16), which keeps the workgroup's LDS at 7448 B (K <= 2) or 8984 B (K >= 3): the register count,
//     not the LDS, sets the occupancy.  The order of a sample's sum does not depend on the window's length.
//   k_ism_tail  as it is, over the P K rows, each row reading its own knot table (IsmTail::env_stride).
constexpr int ISM_MAX_CHANNELS = 4;
constexpr int ISM_DIR_LIST = 96;
#ifdef __HIP__   // hipcc; a host compiler does not know the attribute
#define ISM_WAVES_PER_SIMD(n) __attribute__((amdgpu_waves_per_eu(n)))
#else
#define ISM_WAVES_PER_SIMD(n)
#endif

struct IsmDirJob {
  IsmJob base;              // n_capsules: the P K ROWS (what k_ism_tail and the id ranges count); capsules: the P positions
  const double *patterns;   // (P, K, 4), device
  int32_t n_positions, n_channels;
};

template <int K>
struct alignas(16) IsmDirEntry {
  double f, g, a, c81, s81;   // as IsmEntry, a and g of the omnidirectional image
  int32_t t0, reserved;
  double gain[K];             // w + v . R / d of each channel
};

// the directional variant: K pattern gains beside the omnidirectional image
template <int K>
struct IsmDir : IsmWalls {
  static constexpr int NG = K, LIST = ISM_DIR_LIST;
  using Entry = IsmDirEntry<K>;
  const double *pat;   // the position's K patterns; uniform over the wave: scalar loads, no vector register holds a pattern
  __device__ __forceinline__ void fill(Entry &e, const IsmImage &im) const {
    // the gains go to the list before the common part is formed: neither is live while the other is computed
    {
      const double ux = im.Rx / im.d, uy = im.Ry / im.d, uz = im.Rz / im.d;   // the direction the image arrives from
#pragma unroll
      for (int k = 0; k < K; ++k) e.gain[k] = pat[4 * k] + (pat[4 * k + 1] * ux + pat[4 * k + 2] * uy + pat[4 * k + 3] * uz);
    }
    ism_fill_shape(e, im, amplitude(im));
  }
};

// IsmDir with a source pattern and air: the receiver's K gains as they are, the source's in the common amplitude
template <int K>
struct IsmDirSrc : IsmDir<K> {
  using Entry = IsmDirEntry<K>;
  IsmSource src;
  __device__ __forceinline__ void fill(Entry &e, const IsmImage &im) const {
    {
      const double ux = im.Rx / im.d, uy = im.Ry / im.d, uz = im.Rz / im.d;
#pragma unroll
      for (int k = 0; k < K; ++k)   // IsmDir's expression: its bits
        e.gain[k] = this->pat[4 * k] + (this->pat[4 * k + 1] * ux + this->pat[4 * k + 2] * uy + this->pat[4 * k + 3] * uz);
      e.a = src.gain(im, ux, uy, uz);   // parked in the list and read back below: not live while the wall gain's exp is evaluated
    }
    ism_park();
    ism_fill_shape(e, im, ism_air_amplitude(this->job, im) * e.a);
  }
};

// (waves per SIMD: with SRC and K = 4 hipcc lands a few registers past the 128 of four waves and then stops trying, 166 VGPRs; asked
// for four it finds 128 without scratch.  1 is the default: the other instantiations are compiled as before.)
template <int K, bool TAIL, bool SRC = false, bool COH = false>
__global__ __launch_bounds__(ISM_THREADS) ISM_WAVES_PER_SIMD(SRC && K == 4 && !COH ? 4 : 1) void k_ism_shoebox_dir(IsmDirJob dj) {
  __shared__ IsmDirEntry<K> list[ISM_DIR_LIST];
  __shared__ double win_c[ISM_TAPS], win_s[ISM_TAPS];
  __shared__ int wave_total[2];
  const IsmJob &job = dj.base;
  const int tid = threadIdx.x;
  const int tile = (int)(blockIdx.x % (unsigned)job.n_tiles);
  const int64_t pair = blockIdx.x / (unsigned)job.n_tiles;   // p * N + n
  const int n = (int)(pair % job.n_sources), pos = (int)(pair / job.n_sources);
  const int t_lo = tile * ISM_TILE, t = t_lo + tid;
  const int y_end = TAIL ? job.tail.y_end : job.ir_len;
  const int t_hi = min(t_lo + ISM_TILE, y_end) - 1;
  const int64_t row_stride = (int64_t)job.n_sources * job.pitch;   // from channel k to channel k + 1
  float *row = job.out + ((int64_t)pos * K * job.n_sources + n) * (int64_t)job.pitch;   // channel 0
  if (t_lo >= job.ir_len) {   // a tile of pad samples only
    for (int k = 0; k < K; ++k)
      for (int s = 0; s < ISM_PER_LANE; ++s)
        if (t + s * ISM_THREADS < job.pitch) row[k * row_stride + t + s * ISM_THREADS] = 0.f;
    return;
  }
  double acc[ISM_PER_LANE][K] = {};
  if constexpr (SRC)
    ism_gather(job, IsmDirSrc<K>{{{job}, dj.patterns + (int64_t)pos * (4 * K)}, ism_source(job, n)}, n, pos, t_lo, t_hi, y_end, list, win_c,
               win_s, wave_total, acc);
  else
    ism_gather(job, IsmDir<K>{{job}, dj.patterns + (int64_t)pos * (4 * K)}, n, pos, t_lo, t_hi, y_end, list, win_c, win_s, wave_total, acc);
#pragma unroll
  for (int s = 0; s < ISM_PER_LANE; ++s) {
    const int ts = t + s * ISM_THREADS;
    if (ts >= job.pitch) continue;
    bool mixed = false;
    double w_e = 1.0, w_l = 0.0;
    if constexpr (TAIL) {
      if (ts > job.tail.mix && ts < job.ir_len) {   // at or below M: w_e = 1, w_l = 0, the image sum as it is
        mixed = true;
        ism_fade(job.tail, ts, w_e, w_l);
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      double v = acc[s][k];
      if constexpr (TAIL) {
        if (mixed) {
          const int c = pos * K + k;   // the row: its own noise stream and its own knot table
          const double *ln_env = SRC ? ism_tail_table(job.tail, c, n) : job.tail.ln_env + (int64_t)c * job.tail.env_stride;
          if constexpr (COH)
            v = w_e * v + w_l * ism_envelope(ln_env, ts) * ism_ctail_g(job.tail, c, n, ts);
          else
            v = w_e * v + w_l * ism_envelope(ln_env, ts) * (double)ism_tail_normal(job.tail, ts, n, c);
        }
      }
      row[k * row_stride + ts] = ts < job.ir_len ? (float)v : 0.f;
    }
  }
}

// the source side of a job that ism_prepare has filled
inline int ism_source_prepare(const double *source_patterns, double air, IsmJob *job) {
  if (!isfinite(air) || !(air >= 0.0)) return fail(AL_E_BADARG, "al_ism_shoebox_src: air must be finite and >= 0 (Np/m)");
  job->source_patterns = source_patterns;
  job->air = air;
  return AL_OK;
}

// THE PREPARE OF THE POINT-RECEIVER ENTRIES (al_ism_shoebox, _tail, _dir, _dir_tail, _src): their arguments as the kernels' job, 0 with
// *dj filled or the error of the first bad argument.  patterns == nullptr (with n_channels == 1): omni capsules, dj->patterns null and
// the rows are the positions.  source_patterns == nullptr and air == 0: no source side.  mix < 0: no tail, and the tail's arguments are
// not looked at; else ln_env holds a knot table every env_row_stride knots from row to row and every env_src_stride from source to
// source (0: one table serves them all).  What an entry requires beyond this (a pattern table, a tail) it states itself.
inline int ism_images_prepare(const double *sources, int32_t n_sources, const double *source_patterns, const double *receivers,
                              int32_t n_receivers, const double *patterns, int32_t n_channels, const double *L, const double *beta,
                              double air, double c, double fs, int32_t max_order, int32_t ir_len, int32_t pitch, int64_t mix, int64_t fade,
                              uint64_t seed, int64_t source_id0, int64_t capsule_id0, const double *ln_env, int32_t n_knots,
                              int64_t env_row_stride, int64_t env_src_stride, float *out, IsmDirJob *dj) {
  if (!patterns && n_channels != 1) return fail(AL_E_BADARG, "al_ism_shoebox_src: a null pattern table (omni capsules) takes n_channels == 1");
  if (n_channels < 1 || n_channels > ISM_MAX_CHANNELS) return fail(AL_E_BADARG, "al_ism_shoebox_dir: n_channels must be in 1 .. 4");
  // ism_prepare counts the image workgroups per POSITION; the rows are P K
  if (int rc = ism_prepare(sources, n_sources, receivers, n_receivers, L, beta, c, fs, max_order, ir_len, pitch, out, &dj->base)) return rc;
  if ((int64_t)n_receivers * n_channels > 0x7fffffff) return fail(AL_E_BADARG, "al_ism_shoebox_dir: more than 2^31 - 1 rows (n_receivers x n_channels)");
  dj->patterns = patterns;
  dj->n_positions = n_receivers;
  dj->n_channels = n_channels;
  dj->base.n_capsules = n_receivers * n_channels;
  if (int rc = ism_source_prepare(source_patterns, air, &dj->base)) return rc;
  if (mix >= 0) {
    if (int rc = ism_tail_prepare(mix, fade, seed, source_id0, capsule_id0, ln_env, n_knots, &dj->base)) return rc;
    if (env_row_stride > 0xffffffffll) return fail(AL_E_BADARG, "al_ism_shoebox_src: n_knots x n_sources must be below 2^32");
    dj->base.tail.env_stride = (uint32_t)env_row_stride;
    dj->base.tail.env_src_stride = (uint32_t)env_src_stride;
  }
  return AL_OK;
}

// the coherent tail of a job that ism_images_prepare has filled with a tail: the two tables, and k_ism_ctail's grid in place of
// k_ism_tail's.  The delays' limit (-256 <= D, D + n_taps - 1 <= 256) is the tables' contract: they are not read here
inline int ism_coherent_prepare(const double *taps, const int32_t *delays, int32_t n_waves, int32_t n_taps, int64_t group_id, IsmJob *job) {
  if (!taps || !delays) return fail(AL_E_BADARG, "al_ism_shoebox_coherent: null tap or delay table");
  if (n_waves < 1 || n_waves > ISM_CTAIL_MAX_WAVES) return fail(AL_E_BADARG, "al_ism_shoebox_coherent: n_waves must be in 1 .. 256");
  if (n_taps < 1 || n_taps > ISM_CTAIL_MAX_TAPS) return fail(AL_E_BADARG, "al_ism_shoebox_coherent: n_taps must be in 1 .. 32");
  if (group_id < 0 || group_id > 0xffffffffll) return fail(AL_E_BADARG, "al_ism_shoebox_coherent: group_id must be in [0, 2^32)");
  IsmTail &tail = job->tail;
  tail.taps = taps;
  tail.delays = delays;
  tail.n_waves = n_waves;
  tail.n_taps = n_taps;
  tail.group_id = (uint32_t)group_id;
  tail.tail_blocks = 0;   // k_ism_tail has no sample of these rows
  tail.ctail_blocks = tail.split < job->pitch ? (job->pitch - tail.split + ISM_CTAIL_TILE - 1) / ISM_CTAIL_TILE : 0;
  const int64_t row_blocks = ((int64_t)job->n_capsules + ISM_CTAIL_ROWS - 1) / ISM_CTAIL_ROWS;
  if ((int64_t)tail.ctail_blocks * job->n_sources * row_blocks > 0x7fffffff)
    return fail(AL_E_BADARG, "al_ism_shoebox_coherent: more than 2^31 - 1 workgroups (tiles of 512 samples x sources x blocks of 8 rows): split the call");
  return AL_OK;
}

// the image kernel of a job: k_ism_shoebox for omni capsules, k_ism_shoebox_dir<K> for a pattern table
template <bool TAIL, bool SRC, bool COH = false>
inline void launch_ism_image_kernel(const IsmDirJob &dj, hipStream_t stream) {
  const dim3 grid((unsigned)((int64_t)dj.base.n_tiles * dj.base.n_sources * dj.n_positions)), block(ISM_THREADS);
  switch (dj.patterns ? dj.n_channels : 0) {
    case 0: hipLaunchKernelGGL((k_ism_shoebox<TAIL, SRC, COH>), grid, block, 0, stream, dj.base); break;
    case 1: hipLaunchKernelGGL((k_ism_shoebox_dir<1, TAIL, SRC, COH>), grid, block, 0, stream, dj); break;
    case 2: hipLaunchKernelGGL((k_ism_shoebox_dir<2, TAIL, SRC, COH>), grid, block, 0, stream, dj); break;
    case 3: hipLaunchKernelGGL((k_ism_shoebox_dir<3, TAIL, SRC, COH>), grid, block, 0, stream, dj); break;
    default: hipLaunchKernelGGL((k_ism_shoebox_dir<4, TAIL, SRC, COH>), grid, block, 0, stream, dj); break;
  }
}

// THE LAUNCH OF al_ism_shoebox_coherent: the image kernel with the coherent epilogue below the split, k_ism_ctail past it
inline void launch_ism_coherent(const IsmDirJob &dj, hipStream_t stream) {
  launch_ism_image_kernel<true, true, true>(dj, stream);
  const IsmJob &job = dj.base;
  if (job.tail.ctail_blocks > 0) {
    const int64_t row_blocks = ((int64_t)job.n_capsules + ISM_CTAIL_ROWS - 1) / ISM_CTAIL_ROWS;
    hipLaunchKernelGGL(k_ism_ctail, dim3((unsigned)((int64_t)job.tail.ctail_blocks * job.n_sources * row_blocks)), dim3(ISM_CTAIL_THREADS), 0,
                       stream, job);
  }
}

// THE LAUNCH OF THE POINT-RECEIVER ENTRIES: the image kernel, with a tail over the tiles below the split, then k_ism_tail past it.
// src: the instantiations with the source side (al_ism_shoebox_src takes them whatever its source table and air are)
inline void launch_ism_images(const IsmDirJob &dj, bool with_tail, bool src, hipStream_t stream) {
  if (with_tail)
    src ? launch_ism_image_kernel<true, true>(dj, stream) : launch_ism_image_kernel<true, false>(dj, stream);
  else
    src ? launch_ism_image_kernel<false, true>(dj, stream) : launch_ism_image_kernel<false, false>(dj, stream);
  const IsmJob &job = dj.base;
  if (with_tail && job.tail.tail_blocks > 0)
    hipLaunchKernelGGL(k_ism_tail, dim3((unsigned)((int64_t)job.tail.tail_blocks * job.n_sources * job.n_capsules)), dim3(ISM_TAIL_THREADS),
                       0, stream, job);
}

}  // namespace al
