// LD blocks, r and g from PLINK 1 .bed genotypes (SNP-major 2-bit codes), on
// the device.  Sample n of a marker has code (byte[n / 4] >> 2 (n % 4)) & 3:
//   0 homozygous A1 (x = 2), 1 missing, 2 heterozygous (x = 1), 3 homozygous A2
//   (x = 0); x counts A1.  The bits past sample N of a row's last byte are
//   padding: they read as code 0 and are never counted.
// Per marker, over the observed samples, exact integers n_obs, S1 = sum x,
// S2 = sum x^2; mean = S1 / n_obs, sd = sqrt((n_obs S2 - S1^2) / n_obs^2)
// (k_geno_stats' operations), t[code] = ((x - mean) / sd) / sqrt(N) (k_geno_G's),
// t[missing] = 0 (mean imputation).  G[i][n] = t_i[code_in]; R_b = G_b G_b^T,
// r_b = G_b y, g[n] = sum_i X_std[i][n] beta_i with X_std = sqrt(N) G.
// The rows sit on the device at a stride of whole 32-bit words (16 samples, one
// K-step of the contraction); G itself is never formed.
// Compiled with -ffp-contract=off; the contraction uses explicit fma.
#include "common.h"

namespace sgv {

// valid-sample mask (one bit per 2-bit code, the low bit's position) of word wi
__device__ __forceinline__ uint32_t bed_word_mask(int wi, int nsamp) {
  const int left = nsamp - 16 * wi;
  if (left >= 16) return 0x55555555u;
  if (left <= 0) return 0u;
  return 0x55555555u & ((1u << (2 * left)) - 1u);
}

__device__ __forceinline__ double bed_pick(int code, double t0, double t2, double t3) {
  return code == 0 ? t0 : code == 2 ? t2 : code == 3 ? t3 : 0.0;
}

// One workgroup per marker: the four code counts by popcounts of the two bit
// planes, then mean, sd and the marker's table.  counts[i][code]; lut[i][code]
// = t_i[code] (0 for the missing code); msd[i] = {mean, sd}.  A marker with no
// observed sample, or one value among them (n_obs S2 == S1^2), has no LD: its
// table is zeros and the caller finds it in the counts.
__global__ __launch_bounds__(256) void k_bed_stats(const uint32_t* __restrict__ bits,
                                                   int64_t stride_w, int nsamp,
                                                   long long* __restrict__ counts,
                                                   double* __restrict__ lut,
                                                   double* __restrict__ msd) {
  const int i = blockIdx.x;
  const uint32_t* row = bits + (int64_t)i * stride_w;
  const int nw = (nsamp + 15) / 16;
  int c[4] = {0, 0, 0, 0};
  for (int w = threadIdx.x; w < nw; w += 256) {
    const uint32_t v = row[w];
    const uint32_t m = bed_word_mask(w, nsamp);
    const uint32_t lo = v & 0x55555555u, hi = (v >> 1) & 0x55555555u;
    c[0] += __popc(~lo & ~hi & m);
    c[1] += __popc(lo & ~hi & m);
    c[2] += __popc(~lo & hi & m);
    c[3] += __popc(lo & hi & m);
  }
  __shared__ int sm[4][256];
#pragma unroll
  for (int k = 0; k < 4; ++k) sm[k][threadIdx.x] = c[k];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
#pragma unroll
      for (int k = 0; k < 4; ++k) sm[k][threadIdx.x] += sm[k][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const long long c0 = sm[0][0], c1 = sm[1][0], c2 = sm[2][0], c3 = sm[3][0];
    counts[4 * (int64_t)i + 0] = c0;
    counts[4 * (int64_t)i + 1] = c1;
    counts[4 * (int64_t)i + 2] = c2;
    counts[4 * (int64_t)i + 3] = c3;
    const long long nobs = c0 + c2 + c3, S1 = 2 * c0 + c2, S2 = 4 * c0 + c2;
    const long long num = nobs * S2 - S1 * S1;  // n_obs^2 var, exact
    double t[4] = {0.0, 0.0, 0.0, 0.0}, mean = 0.0, sd = 0.0;
    if (nobs > 0 && num != 0) {
      mean = (double)S1 / (double)nobs;
      sd = sqrt((double)num / ((double)nobs * (double)nobs));
      const double rn = sqrt((double)nsamp);
      t[0] = ((2.0 - mean) / sd) / rn;
      t[2] = ((1.0 - mean) / sd) / rn;
      t[3] = ((0.0 - mean) / sd) / rn;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) lut[4 * (int64_t)i + k] = t[k];
    msd[2 * (int64_t)i] = mean;
    msd[2 * (int64_t)i + 1] = sd;
  }
}

hipError_t launch_bed_stats(const uint32_t* d_bits, int64_t stride_w, int n, int nsamp,
                            long long* d_counts, double* d_lut, double* d_msd, hipStream_t st) {
  hipLaunchKernelGGL(k_bed_stats, dim3(n), dim3(256), 0, st, d_bits, stride_w, nsamp, d_counts,
                     d_lut, d_msd);
  return hipGetLastError();
}

// One 64 x 64 tile of G_a G_b^T straight from the bits, the contraction of every
// LD kernel below: k_syrk_nt's tiles (256 threads x (4 x 4) outputs, K-steps of 16
// samples through LDS); the loader differs.  Rows ra0 .. ra0 + 63 of (bits_a,
// lut_a) against rows rb0 .. rb0 + 63 of (bits_b, lut_b).  Thread t owns tile row
// t / 4 on both sides, whose tables it keeps in registers, and byte t % 4 of the
// K-step's word: four samples decoded into the As / Bs tiles.  Samples >= N and
// rows >= na / nb give 0.  The next K-step's bytes are loaded before the current
// one's products.  acc[a][b] is output (ra0 + ty + 16 a, rb0 + tx + 16 b): one
// sample-sequential fma chain, k ascending, one accumulator per output, so an
// entry is the same double whichever kernel forms it.
__device__ __forceinline__ void bed_tile(const uint8_t* __restrict__ bits_a,
                                         const double* __restrict__ lut_a, int ra0, int na,
                                         const uint8_t* __restrict__ bits_b,
                                         const double* __restrict__ lut_b, int rb0, int nb,
                                         int64_t stride_b, int nsamp, double (&acc)[4][4]) {
  __shared__ double As[16][64 + 2];
  __shared__ double Bs[16][64 + 2];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int lr = threadIdx.x >> 2, lq = threadIdx.x & 3;   // loader: tile row, byte of the word
  const bool va = ra0 + lr < na, vb = rb0 + lr < nb;
  double a0 = 0.0, a2 = 0.0, a3 = 0.0, b0 = 0.0, b2 = 0.0, b3 = 0.0;
  if (va) {
    const double* l = lut_a + 4 * (int64_t)(ra0 + lr);
    a0 = l[0], a2 = l[2], a3 = l[3];
  }
  if (vb) {
    const double* l = lut_b + 4 * (int64_t)(rb0 + lr);
    b0 = l[0], b2 = l[2], b3 = l[3];
  }
  const uint8_t* pa = bits_a + (int64_t)(va ? ra0 + lr : 0) * stride_b + lq;
  const uint8_t* pb = bits_b + (int64_t)(vb ? rb0 + lr : 0) * stride_b + lq;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
  const int kpad = (nsamp + 15) / 16 * 16;   // == 4 stride_b: every byte read is inside the row
  unsigned ba = pa[0], bb = pb[0];
  for (int k0 = 0; k0 < kpad; k0 += 16) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int kk = 4 * lq + e;
      const bool in = k0 + kk < nsamp;
      As[kk][lr] = in ? bed_pick((ba >> (2 * e)) & 3, a0, a2, a3) : 0.0;
      Bs[kk][lr] = in ? bed_pick((bb >> (2 * e)) & 3, b0, b2, b3) : 0.0;
    }
    if (k0 + 16 < kpad) {
      ba = pa[(k0 >> 2) + 4];
      bb = pb[(k0 >> 2) + 4];
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      double av[4], bv[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) av[a] = As[kk][ty + 16 * a];
#pragma unroll
      for (int b = 0; b < 4; ++b) bv[b] = Bs[kk][tx + 16 * b];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_fma(av[a], bv[b], acc[a][b]);
    }
    __syncthreads();
  }
}

// R = G G^T: bed_tile over the upper tiles, then k_syrk_nt's epilogue (dense or
// packed triangle, both mirrors)
template <class T>
__global__ __launch_bounds__(256) void k_bed_syrk(const uint8_t* __restrict__ bits,
                                                  int64_t stride_b, const double* __restrict__ lut,
                                                  int n, int nsamp, T* __restrict__ R, int64_t lda,
                                                  int packed, const int64_t* __restrict__ poff,
                                                  const int64_t* __restrict__ pw) {
  const int tj = blockIdx.x, ti = blockIdx.y;
  if (ti > tj) return;
  const int i0 = ti * 64, j0 = tj * 64;
  double acc[4][4];
  bed_tile(bits, lut, i0, n, bits, lut, j0, n, stride_b, nsamp, acc);
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
      if (i < n && j < n) {
        if (packed) {
          T* p = sym_addr(R, poff, pw, i, j);
          if (p) *p = (T)acc[a][b];
          p = sym_addr(R, poff, pw, j, i);
          if (p) *p = (T)acc[a][b];
        } else {
          R[(int64_t)i * lda + j] = (T)acc[a][b];
          R[(int64_t)j * lda + i] = (T)acc[a][b];
        }
      }
    }
}

hipError_t launch_bed_syrk(const uint32_t* d_bits, int64_t stride_w, const double* d_lut, int n,
                           int nsamp, void* d_R, int64_t lda, int packed, const int64_t* d_poff,
                           const int64_t* d_pw, int bits, hipStream_t st) {
  const int nt = (n + 63) / 64;
  if (bits == 32 && !packed) return hipErrorInvalidValue;   // f32 is a packed layout only
  const uint8_t* by = reinterpret_cast<const uint8_t*>(d_bits);
  if (bits == 32)
    hipLaunchKernelGGL(k_bed_syrk<float>, dim3(nt, nt), dim3(256), 0, st, by, stride_w * 4, d_lut,
                       n, nsamp, (float*)d_R, lda, packed, d_poff, d_pw);
  else
    hipLaunchKernelGGL(k_bed_syrk<double>, dim3(nt, nt), dim3(256), 0, st, by, stride_w * 4, d_lut,
                       n, nsamp, (double*)d_R, lda, packed, d_poff, d_pw);
  return hipGetLastError();
}

// How far row i of a symmetric band reaches: hi(i), its last stored column (i <=
// hi(i) <= n - 1, non-decreasing), a policy k_bed_band takes by value.  A marker
// window is a reach: for i <= j < n, j - i <= W iff j <= min(i + W, n - 1), which
// ReachWindow forms in registers; ReachRows reads the caller's array.
struct ReachWindow {
  int W, n;   // 1 <= W <= n - 1
  __device__ __forceinline__ int hi(int i) const { return i + W < n - 1 ? i + W : n - 1; }
};
struct ReachRows {
  const int32_t* __restrict__ h;
  __device__ __forceinline__ int hi(int i) const { return h[i]; }
};

// Windowed R (include/sgvamp_hip.h, "windowed genotype LD" and "distance-windowed
// genotype LD"): bed_tile over the tiles of the band only.  Grid (column tiles a
// row tile reaches) x (row tiles), tj = ti + blockIdx.x.  Entry (i, j), j >= i, is
// stored iff j <= hi(i); everything else keeps the zero the caller's memset left.
// hi is non-decreasing, so row min(i0 + 63, n - 1) has the tile's farthest reach
// and a tile past it returns before loading.  (j, i) is stored too where it lies
// in the panel's diagonal 256 x 256 block, which the packed layout keeps in full.
// ext: the packed band's stored extent (0: the packed triangle); a panel starting
// at row r0 holds columns r0 .. r0 + min(n - r0, ext) - 1, which sym_addr does not
// know.  TAPER: the finished sum times w = 1 - (pos[j] - pos[i]) / span, formed in
// that order in f64 (one subtraction, one division, one subtraction, one
// multiplication; w >= 0 by the reach predicate), rounded once on store.
template <class T, class Reach, bool TAPER>
__global__ __launch_bounds__(256) void k_bed_band(const uint8_t* __restrict__ bits,
                                                  int64_t stride_b, const double* __restrict__ lut,
                                                  int n, int nsamp, const Reach reach,
                                                  const double* __restrict__ pos, double span,
                                                  int64_t ext, T* __restrict__ R,
                                                  const int64_t* __restrict__ poff,
                                                  const int64_t* __restrict__ pw) {
  const int ti = blockIdx.y;
  const int64_t tj = (int64_t)ti + blockIdx.x;
  const int i0 = ti * 64;
  // no column, or the first column is past the reach of the tile's last row: nothing to load
  if (tj * 64 >= n || tj * 64 > reach.hi(i0 + 63 < n ? i0 + 63 : n - 1)) return;
  const int j0 = (int)tj * 64;
  double acc[4][4];
  bed_tile(bits, lut, i0, n, bits, lut, j0, n, stride_b, nsamp, acc);
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = i0 + ty + 16 * a;
    if (i >= n) continue;
    const int hi_i = reach.hi(i);
    const int r0 = i / SYM_H * SYM_H;
    const int64_t cols = ext > 0 && ext < n - r0 ? ext : n - r0;   // the panel's stored columns
    double pi = 0.0;
    if (TAPER) pi = pos[i];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int j = j0 + tx + 16 * b;
      if (j >= n || j < i || j > hi_i) continue;
      if (j - r0 >= cols) continue;        // cannot happen: j <= hi(i) <= i + bw < r0 + 256 + bw <= r0 + ext
      double v = acc[a][b];
      if (TAPER) {
        const double w = 1.0 - (pos[j] - pi) / span;
        v = v * w;
      }
      *sym_addr(R, poff, pw, i, j) = (T)v;
      if (j != i && j < r0 + SYM_H) *sym_addr(R, poff, pw, j, i) = (T)v;
    }
  }
}

template <class Reach, bool TAPER>
static void launch_band(dim3 grid, hipStream_t st, const uint32_t* d_bits, int64_t stride_w,
                        const double* d_lut, int n, int nsamp, Reach reach, const double* d_pos,
                        double span, int64_t ext, void* d_R, const int64_t* d_poff,
                        const int64_t* d_pw, int bits) {
  const uint8_t* by = reinterpret_cast<const uint8_t*>(d_bits);
  if (bits == 32)
    hipLaunchKernelGGL((k_bed_band<float, Reach, TAPER>), grid, dim3(256), 0, st, by, stride_w * 4,
                       d_lut, n, nsamp, reach, d_pos, span, ext, (float*)d_R, d_poff, d_pw);
  else
    hipLaunchKernelGGL((k_bed_band<double, Reach, TAPER>), grid, dim3(256), 0, st, by,
                       stride_w * 4, d_lut, n, nsamp, reach, d_pos, span, ext, (double*)d_R, d_poff,
                       d_pw);
}

// hi == nullptr: the marker window, whose farthest column of row tile ti is 64 ti +
// 63 + W: tile ti + (63 + W) / 64; no array is made or read.  Else hi is the host's
// copy of d_hi (checked by the caller: i <= hi[i] <= n - 1, non-decreasing), from
// which the grid's width is the most column tiles any row tile reaches -- never
// the square of tiles unless the reach is the triangle.
hipError_t launch_bed_band(const uint32_t* d_bits, int64_t stride_w, const double* d_lut, int n,
                           int nsamp, int64_t window, const int32_t* hi, const int32_t* d_hi,
                           const double* d_pos, double span, int64_t ext, void* d_R,
                           const int64_t* d_poff, const int64_t* d_pw, int bits, hipStream_t st) {
  const int64_t nt = ((int64_t)n + 63) / 64;
  if (n < 1 || nt > 65535 || (hi ? !d_hi : window < 1)) return hipErrorInvalidValue;
  if (!hi) {
    const int64_t nx = std::min<int64_t>(nt, (63 + window) / 64 + 1);
    const ReachWindow rw{(int)std::min<int64_t>(window, n - 1), n};
    launch_band<ReachWindow, false>(dim3((unsigned)nx, (unsigned)nt), st, d_bits, stride_w, d_lut,
                                    n, nsamp, rw, nullptr, 0.0, ext, d_R, d_poff, d_pw, bits);
    return hipGetLastError();
  }
  int64_t nx = 1;
  for (int64_t ti = 0; ti < nt; ++ti)
    nx = std::max<int64_t>(nx, hi[std::min<int64_t>(64 * ti + 63, n - 1)] / 64 - ti + 1);
  const dim3 grid((unsigned)nx, (unsigned)nt);
  if (d_pos)
    launch_band<ReachRows, true>(grid, st, d_bits, stride_w, d_lut, n, nsamp, ReachRows{d_hi},
                                 d_pos, span, ext, d_R, d_poff, d_pw, bits);
  else
    launch_band<ReachRows, false>(grid, st, d_bits, stride_w, d_lut, n, nsamp, ReachRows{d_hi},
                                  d_pos, span, ext, d_R, d_poff, d_pw, bits);
  return hipGetLastError();
}

// How many head columns tail row a of a corner keeps: keep(a) in [0, nc], non-
// decreasing, k_bed_corner's policy.  A marker window is a count: entry (a, c)
// couples markers c + nr - a apart, and c + nr - a <= W iff c < W - nr + a + 1.
struct KeepWindow {
  int W, nr, nc;   // 1 <= W <= nr + nc
  __device__ __forceinline__ int keep(int a) const {
    const int k = W - nr + a + 1;
    return k < 0 ? 0 : k > nc ? nc : k;
  }
};
struct KeepRows {
  const int32_t* __restrict__ k;
  __device__ __forceinline__ int keep(int a) const { return k[a]; }
};

// The band's corner between two pieces: C = G_tail G_head^T (nr x nc, row major)
// from one staged row set, the tail's nr rows first, then the head's nc.  Entry
// (a, c) is stored iff c < keep(a); C was zeroed by the caller.  keep is non-
// decreasing, so row min(a0 + 63, nr - 1) has the tile's largest count.  TAPER:
// times w = 1 - (pos[nr + c] - pos[a]) / span (pos: the nr + nc halo rows'
// positions), as k_bed_band forms it.  f32: the entry is rounded once to f32 (what
// the uncut f32 band stores) and kept as the double of that float.
template <class Keep, bool TAPER>
__global__ __launch_bounds__(256) void k_bed_corner(const uint8_t* __restrict__ bits,
                                                    int64_t stride_b,
                                                    const double* __restrict__ lut, int nr, int nc,
                                                    int nsamp, const Keep keep,
                                                    const double* __restrict__ pos, double span,
                                                    int f32, double* __restrict__ C) {
  const int a0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  if (a0 >= nr || c0 >= nc || c0 >= keep.keep(a0 + 63 < nr ? a0 + 63 : nr - 1)) return;
  double acc[4][4];
  bed_tile(bits, lut, a0, nr, bits + (int64_t)nr * stride_b, lut + 4 * (int64_t)nr, c0, nc,
           stride_b, nsamp, acc);
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int ia = a0 + ty + 16 * a;
    if (ia >= nr) continue;
    const int k = keep.keep(ia);
    double pa = 0.0;
    if (TAPER) pa = pos[ia];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int ic = c0 + tx + 16 * b;
      if (ic >= nc || ic >= k) continue;
      double v = acc[a][b];
      if (TAPER) {
        const double w = 1.0 - (pos[nr + ic] - pa) / span;
        v = v * w;
      }
      C[(int64_t)ia * nc + ic] = f32 ? (double)(float)v : v;
    }
  }
}

// d_keep == nullptr: the marker window, kmax = min(W, nc) (row nr - 1's count).
// Else kmax is the largest keep (the caller's, from its host copy).  The grid
// covers the kept columns only.
hipError_t launch_bed_corner(const uint32_t* d_bits, int64_t stride_w, const double* d_lut, int nr,
                             int nc, int nsamp, int64_t window, const int32_t* d_keep, int kmax,
                             const double* d_pos, double span, int bits, double* d_C,
                             hipStream_t st) {
  if (nr < 1 || nc < 1 || (nr + 63) / 64 > 65535) return hipErrorInvalidValue;
  if (!d_keep) {
    if (window < 1) return hipErrorInvalidValue;
    kmax = (int)std::min<int64_t>(window, nc);
  }
  if (kmax < 1 || kmax > nc) return hipErrorInvalidValue;
  const dim3 grid((kmax + 63) / 64, (nr + 63) / 64);
  const uint8_t* by = reinterpret_cast<const uint8_t*>(d_bits);
  const int f32 = bits == 32 ? 1 : 0;
  if (!d_keep) {
    const KeepWindow kw{(int)std::min<int64_t>(window, (int64_t)nr + nc), nr, nc};
    hipLaunchKernelGGL((k_bed_corner<KeepWindow, false>), grid, dim3(256), 0, st, by, stride_w * 4,
                       d_lut, nr, nc, nsamp, kw, nullptr, 0.0, f32, d_C);
  } else if (d_pos) {
    hipLaunchKernelGGL((k_bed_corner<KeepRows, true>), grid, dim3(256), 0, st, by, stride_w * 4,
                       d_lut, nr, nc, nsamp, KeepRows{d_keep}, d_pos, span, f32, d_C);
  } else {
    hipLaunchKernelGGL((k_bed_corner<KeepRows, false>), grid, dim3(256), 0, st, by, stride_w * 4,
                       d_lut, nr, nc, nsamp, KeepRows{d_keep}, d_pos, span, f32, d_C);
  }
  return hipGetLastError();
}

// out[i] = sum_n t_i[code_in] y[n]; one wave per marker, k_row_dot's lane order
__global__ __launch_bounds__(256) void k_bed_row_dot(const uint8_t* __restrict__ bits,
                                                     int64_t stride_b,
                                                     const double* __restrict__ lut, int n,
                                                     int nsamp, const double* __restrict__ y,
                                                     double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const double* l = lut + 4 * (int64_t)i;
  const double t0 = l[0], t2 = l[2], t3 = l[3];
  const uint8_t* row = bits + (int64_t)i * stride_b;
  double s = 0.0;
  for (int k = lane; k < nsamp; k += 64) {
    const int code = (row[k >> 2] >> (2 * (k & 3))) & 3;
    s = __builtin_fma(bed_pick(code, t0, t2, t3), y[k], s);
  }
  s = wave_sum(s);
  if (lane == 0) out[i] = s;
}

hipError_t launch_bed_row_dot(const uint32_t* d_bits, int64_t stride_w, const double* d_lut, int n,
                              int nsamp, const double* d_y, double* d_out, hipStream_t st) {
  hipLaunchKernelGGL(k_bed_row_dot, dim3((n + 3) / 4), dim3(256), 0, st,
                     reinterpret_cast<const uint8_t*>(d_bits), stride_w * 4, d_lut, n, nsamp, d_y,
                     d_out);
  return hipGetLastError();
}

// g[n] = sum_i X_std[i][n] beta[i], X_std = (x - mean) / sd (0 where missing), in
// marker order as k_g_accum; markers with beta == 0 are skipped
__global__ __launch_bounds__(256) void k_bed_g_accum(const uint8_t* __restrict__ bits,
                                                     int64_t stride_b,
                                                     const double* __restrict__ msd, int nb,
                                                     int nsamp, const double* __restrict__ beta,
                                                     double* __restrict__ g) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= nsamp) return;
  const uint8_t* col = bits + (n >> 2);
  const int sh = 2 * (n & 3);
  double s = 0.0;
  for (int i = 0; i < nb; ++i) {
    const double b = beta[i];
    if (b == 0.0) continue;  // exact: adding +0*x changes nothing unless x is inf/nan
    const int code = (col[(int64_t)i * stride_b] >> sh) & 3;
    if (code == 1) continue;  // missing: X_std = 0
    const double x = code == 0 ? 2.0 : code == 2 ? 1.0 : 0.0;
    const double xs = (x - msd[2 * (int64_t)i]) / msd[2 * (int64_t)i + 1];
    s = s + xs * b;
  }
  g[n] = s;
}

hipError_t launch_bed_g_accum(const uint32_t* d_bits, int64_t stride_w, const double* d_msd, int n,
                              int nsamp, const double* d_beta, double* d_g, hipStream_t st) {
  hipLaunchKernelGGL(k_bed_g_accum, dim3((nsamp + 255) / 256), dim3(256), 0, st,
                     reinterpret_cast<const uint8_t*>(d_bits), stride_w * 4, d_msd, n, nsamp,
                     d_beta, d_g);
  return hipGetLastError();
}

}  // namespace sgv
