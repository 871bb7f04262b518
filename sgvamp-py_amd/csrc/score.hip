// Scoring a target panel with saved effects (include/sgvamp_hip.h, "scoring"):
//   S[n][c] = sum_i X[i][n] B[i][c]
// over the markers i of a stream of chunks, all target samples n and up to 16
// columns c per column group, on the f64 matrix cores.  X[i][n] = tab_i[code_in],
// a 4-entry f64 table per marker, code = bits 2 (n % 16) of word n / 16 of row i
// as geno.hip and geno_factor.hip read it.
//
//   k_score_tab   tab from the chunk's exact counts (TARGET and RAW modes).
//   k_score_pack  pk[i][c], the group's columns interleaved per marker, unused
//                 columns zero.
//   k_score_mfma  part[s][n][c]: the partial of slab s (SC_SLAB = 1,024 markers by
//                 GLOBAL index; a chunk starts on a slab boundary).  One workgroup
//                 of 4 waves per (256 samples, slab); a wave owns 4 groups of 16
//                 samples, so one decode of tab_i and one B operand serve four
//                 independent accumulator chains.  v_mfma_f64_16x16x4_f64:
//                   A (16 samples x 4 markers): lane l holds sample l & 15 of
//                     marker l >> 4 -- one 32-bit word of a row is the group's 16
//                     samples, the lane shifts it by 2 (l & 15);
//                   B (4 markers x 16 columns): lane l holds pk[marker l >> 4][l & 15];
//                   D (16 x 16 of S): lane l, register r: sample (l >> 4) + 4 r,
//                     column l & 15.
//                 The slab's rows go through LDS SC_TM = 128 markers at a time
//                 (16 words of a row per 16 threads: loads coalesced along
//                 samples), with the markers' tables and pk rows beside them.
//                 The decode is an LDS read, tab_i[code]: a bit-field extract, an
//                 address and a ds_read_b64 per MFMA.  Selecting among the four
//                 entries in registers (six v_cndmask per value) measured 1.17x
//                 the kernel's time at N = 50,000: on this device VALU work
//                 beside f64 MFMAs adds to their time instead of hiding in it
//                 (profiles/score/README.md).
//   k_score_sum   S += part[0], += part[1], ...: ascending slab order.
//
// Order contract.  A slab's partial starts from +0 and takes its markers four at
// a time in ascending order (one MFMA per quad and sample group); S is the slab
// partials added left to right in ascending slab order, across chunk boundaries.
// No atomics; nothing depends on the grid, the CU count, the chunk length or
// how many slabs a launch takes.  A column's chain never meets another column's
// values, so a result does not depend on which columns share its group.  D rows
// are independent per sample and rows n >= N are never stored, so the padding
// bits of a row's last word never reach a result; words past the row's stride
// are not read.  Markers past the chunk's end in a quad have a zero pk row and a
// zero table: exact zero products.
// Compiled with -ffp-contract=off.
#include "score.h"

namespace sgv {

constexpr int SC_TM = 128;          // markers per LDS tile
constexpr int SC_WG = 4;            // 16-sample groups (32-bit words of a row) per wave
constexpr int SC_WW = 4 * SC_WG;    // words of a row per workgroup (4 waves): 256 samples

typedef double sc_d4 __attribute__((ext_vector_type(4)));
typedef uint32_t sc_u4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void k_score_tab(int mode, const long long* __restrict__ cnt,
                                                   const double* __restrict__ msd, int n,
                                                   double* __restrict__ tab) {
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= n) return;
  double t[4] = {0.0, 0.0, 0.0, 0.0};
  if (mode == 0) {
    const double mean = msd[2 * (int64_t)i], sd = msd[2 * (int64_t)i + 1];
    if (sd > 0.0) {   // k_bed_stats: sd = 0 marks a marker without variance (or unobserved)
      t[0] = (2.0 - mean) / sd;
      t[2] = (1.0 - mean) / sd;
      t[3] = (0.0 - mean) / sd;
    }
  } else {
    const long long c0 = cnt[4 * (int64_t)i], c2 = cnt[4 * (int64_t)i + 2],
                    c3 = cnt[4 * (int64_t)i + 3];
    const long long nobs = c0 + c2 + c3, S1 = 2 * c0 + c2;
    t[0] = 2.0;
    t[1] = nobs > 0 ? (double)S1 / (double)nobs : 0.0;
    t[2] = 1.0;
    t[3] = 0.0;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) tab[4 * (int64_t)i + k] = t[k];
}

hipError_t launch_score_tab(int mode, const long long* d_cnt, const double* d_msd, int n,
                            double* d_tab, hipStream_t st) {
  if (n < 1 || (mode != 0 && mode != 1)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_score_tab, dim3((n + 255) / 256), dim3(256), 0, st, mode, d_cnt, d_msd, n,
                     d_tab);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void k_score_pack(const double* __restrict__ beta, int n,
                                                    int ncol, int c0, double* __restrict__ pk) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)n * SC_COLS) return;
  const int64_t i = idx / SC_COLS;
  const int c = c0 + (int)(idx % SC_COLS);
  pk[idx] = c < ncol ? beta[(int64_t)c * n + i] : 0.0;
}

hipError_t launch_score_pack(const double* d_beta, int n, int ncol, int c0, double* d_pk,
                             hipStream_t st) {
  if (n < 1 || ncol < 1 || c0 < 0 || c0 >= ncol) return hipErrorInvalidValue;
  const int64_t nb = ((int64_t)n * SC_COLS + 255) / 256;
  hipLaunchKernelGGL(k_score_pack, dim3((unsigned)nb), dim3(256), 0, st, d_beta, n, ncol, c0, d_pk);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void k_score_mfma(const uint32_t* __restrict__ bits,
                                                    int64_t stride_w,
                                                    const double* __restrict__ tab,
                                                    const double* __restrict__ pk, int nm,
                                                    int nsamp, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) uint32_t sbits[SC_TM][SC_WW];
  __shared__ __attribute__((aligned(16))) double stab[SC_TM][4];
  __shared__ __attribute__((aligned(16))) double spk[SC_TM][SC_COLS];
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int lo = lane & 15, hi = lane >> 4;
  const int w0 = blockIdx.x * SC_WW;              // the workgroup's first word of a row
  const int slab = blockIdx.y;
  const int i0 = slab * SC_SLAB;
  const int i1 = min(nm, i0 + SC_SLAB);           // i0 < nm: the launcher's grid
  sc_d4 acc[SC_WG];
#pragma unroll
  for (int g = 0; g < SC_WG; ++g) acc[g] = sc_d4{0.0, 0.0, 0.0, 0.0};
  const int lw = tid & 15, lr = tid >> 4;
  const bool wok = w0 + lw < stride_w;            // words past the row's stride are not read
#pragma unroll 1
  for (int t0 = i0; t0 < i1; t0 += SC_TM) {
    if (t0 != i0) __syncthreads();                // the tile before this one has been read
#pragma unroll
    for (int j = 0; j < SC_TM / 16; ++j) {
      const int r = lr + 16 * j;
      uint32_t v = 0u;
      if (wok && t0 + r < i1) v = ldg(bits + (int64_t)(t0 + r) * stride_w + w0 + lw);
      sbits[r][lw] = v;
    }
#pragma unroll
    for (int j = 0; j < SC_TM * 4 / 256; ++j) {
      const int idx = tid + 256 * j;
      const int r = idx >> 2;
      (&stab[0][0])[idx] = t0 + r < i1 ? ldg(tab + (int64_t)t0 * 4 + idx) : 0.0;
    }
#pragma unroll
    for (int j = 0; j < SC_TM * SC_COLS / 256; ++j) {
      const int idx = tid + 256 * j;
      const int r = idx >> 4;
      (&spk[0][0])[idx] = t0 + r < i1 ? ldg(pk + (int64_t)t0 * SC_COLS + idx) : 0.0;
    }
    __syncthreads();
    const int nq = (min(SC_TM, i1 - t0) + 3) / 4;
    for (int q = 0; q < nq; ++q) {
      const int r = 4 * q + hi;
      const sc_u4 w = *(const sc_u4*)&sbits[r][SC_WG * wid];
      const double* t = &stab[r][0];               // the decode is an LDS read: tab_r[code]
      const double b = spk[r][lo];
      const int sh = 2 * lo;
      const double a0 = t[(w.x >> sh) & 3u];
      const double a1 = t[(w.y >> sh) & 3u];
      const double a2 = t[(w.z >> sh) & 3u];
      const double a3 = t[(w.w >> sh) & 3u];
      acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, acc[1], 0, 0, 0);
      acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, b, acc[2], 0, 0, 0);
      acc[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a3, b, acc[3], 0, 0, 0);
    }
  }
  double* o = part + (int64_t)slab * nsamp * SC_COLS;
#pragma unroll
  for (int g = 0; g < SC_WG; ++g)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t n = (int64_t)16 * (w0 + SC_WG * wid + g) + hi + 4 * r;
      if (n < nsamp) o[n * SC_COLS + lo] = acc[g][r];
    }
}

hipError_t launch_score_mfma(const uint32_t* d_bits, int64_t stride_w, const double* d_tab,
                             const double* d_pk, int nm, int nslab, int nsamp, double* d_part,
                             hipStream_t st) {
  if (nm < 1 || nsamp < 1 || nslab < 1 || nslab > 65535 || stride_w < ((int64_t)nsamp + 15) / 16 ||
      (int64_t)(nslab - 1) * SC_SLAB >= nm || (int64_t)nslab * SC_SLAB < nm)
    return hipErrorInvalidValue;
  const int gx = (int)((((int64_t)nsamp + 15) / 16 + SC_WW - 1) / SC_WW);
  hipLaunchKernelGGL(k_score_mfma, dim3(gx, nslab), dim3(256), 0, st, d_bits, stride_w, d_tab, d_pk,
                     nm, nsamp, d_part);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void k_score_sum(const double* __restrict__ part, int nslab,
                                                   int64_t len, double* __restrict__ S) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= len) return;
  double v = S[idx];
  for (int s = 0; s < nslab; ++s) v += ldg(part + (int64_t)s * len + idx);
  S[idx] = v;
}

hipError_t launch_score_sum(const double* d_part, int nslab, int nsamp, double* d_S,
                            hipStream_t st) {
  if (nslab < 1 || nsamp < 1) return hipErrorInvalidValue;
  const int64_t len = (int64_t)nsamp * SC_COLS;
  hipLaunchKernelGGL(k_score_sum, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, st, d_part,
                     nslab, len, d_S);
  return hipGetLastError();
}

}  // namespace sgv
