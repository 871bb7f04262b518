// Factor LD blocks: the LD pass of a block kept as its 2-bit genotype rows,
// Q = G_b (G_b^T P), R_b = G_b G_b^T never formed (include/sgvamp_hip.h, "factor
// LD blocks").  G[i][n] = lut_i[code_in] as geno.hip reads it: code = bits 2 (n %
// 16) of word n / 16 of row i; the bits past sample nsamp are never read as
// samples.  Four kernels per launch over some of a matrix's blocks, 1-16 columns:
//
//   k_gf_pack  pk[i][c] = P[i][c], the columns interleaved per marker.
//   k_gf_t     tp[s][c][n] = sum_{i in slab s} G[i][n] P[i][c]
//              one thread per sample (a workgroup: GF_SCH = 256 consecutive samples
//              of one slab of GF_SLAB = 1024 markers), markers in ascending order
//              in one fma chain per column.  A lane reads the 32-bit word of its
//              sample (16 lanes share a word, a wave reads 16 consecutive bytes of
//              the row); the marker's table and its pk row are wave-uniform and come
//              through scalar loads (one each), so P is read once per wave, not
//              per lane.
//   k_gf_tsum  t[n][c] = ((tp[0] + tp[1]) + ...) + tp[nslab - 1], slab order.
//   k_gf_q     Q[i][c] = sum_n G[i][n] t[n][c], then the pass's epilogue
//              one workgroup per tile of GF_TILE = 64 markers, one lane per marker;
//              wave w takes sample chunk w of GF_QCH = 4 (whole words: ceil(nw / 4)
//              words each, nw = ceil(nsamp / 16)), samples in ascending order in
//              one fma chain per column.  The wave's 64 rows x 16 words of bits are
//              read coalesced along samples (a wave instruction: 4 rows x 64
//              consecutive bytes) into LDS, from where each lane takes its row; the
//              sample's t row is wave-uniform: one scalar load serves the tile's 64
//              markers (the operand reuse: t crosses the scalar cache once per 64
//              markers, n_b N nc / 8 bytes per block instead of 8 n_b N nc).
//              The four chunk sums are added in chunk order, ((q0 + q1) + q2) + q3;
//              out = c1 Q + c2 in, yout = ys1 Q + ys0 in, and the tile's dot
//              partial (wave butterfly over its 64 markers) goes to its own slot.
//
// Every sum's order is a function of (n_b, nsamp, nc) alone: slabs, tiles and
// chunks are cut from the block's own extents, no atomics, nothing depends on
// the grid, the CU count or what else is in the launch.
// Scratch per launch (owned by the context, grown by ensure_plan): t, nsamp x nc,
// and tp, nslab x nsamp x nc doubles per block; ensure_plan cuts a matrix's
// blocks into launches of at most GF_SCRATCH_MAX doubles at 16 columns (256 MB:
// 11 north-star blocks, 240 MB beside 2.5 GB of rows).  pk is the context's
// interleaved right-hand-side buffer (Mpad x 16 doubles, the MFMA pass's).
// Compiled with -ffp-contract=off; the products use explicit fma.
#include "common.h"

namespace sgv {

// wave-uniform read-only data through the constant address space: a scalar load
// where the address is uniform (nothing in these kernels writes what it reads)
__device__ __forceinline__ double cld(const double* p) {
  return *(const __attribute__((address_space(4))) double*)p;
}

__device__ __forceinline__ double gf_pick(uint32_t code, double t0, double t2, double t3) {
  return code == 0 ? t0 : code == 2 ? t2 : code == 3 ? t3 : 0.0;
}

// pk[voff + i][c] = in[c][voff + i]: a marker's P row in one piece, for k_gf_t's
// scalar loads (NC separate columns would cost NC loads per marker)
template <int NC>
__global__ __launch_bounds__(GF_SCH) void k_gf_pack(const FacBlock* __restrict__ fbs, PassArgs pa,
                                                    double* __restrict__ pk) {
  const FacBlock fb = fbs[blockIdx.z];
  if (pa.run && !ldg(pa.run)) return;   // no-op pass (pipelined CG past its stop test)
  const int i = blockIdx.x * GF_SCH + (int)threadIdx.x;
  if (i >= fb.n) return;
  double* o = pk + (fb.voff + i) * NC;
#pragma unroll
  for (int c = 0; c < NC; ++c) o[c] = pa.in[c][fb.voff + i];
}

template <int NC>
__global__ __launch_bounds__(GF_SCH) void k_gf_t(const FacBlock* __restrict__ fbs,
                                                 const int* __restrict__ run,
                                                 const double* __restrict__ pk,
                                                 double* __restrict__ tp) {
  const FacBlock fb = fbs[blockIdx.z];
  if (run && !ldg(run)) return;
  const int n0 = blockIdx.x * GF_SCH, s = blockIdx.y;
  if (n0 >= fb.nsamp || s >= fb.nslab) return;
  const int n = n0 + (int)threadIdx.x;
  const bool live = n < fb.nsamp;
  const uint32_t* col = fb.bits + (live ? n >> 4 : 0);   // word n / 16 < ceil(nsamp / 16) <= stride_w
  const int sh = 2 * (n & 15);
  const int i0 = s * GF_SLAB, i1 = min(fb.n, i0 + GF_SLAB);
  double acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.0;
  // four markers per round (measured: 16 and 8 at few columns spill scalar
  // registers and are 0.97-1.17x the time, profiles/geno_factor/README.md)
#pragma unroll 4
  for (int i = i0; i < i1; ++i) {
    const uint32_t w = ldg(col + (int64_t)i * fb.stride_w);
    const double* l = fb.lut + 4 * (int64_t)i;
    const double* pr = pk + (fb.voff + i) * NC;
    const double g = gf_pick((w >> sh) & 3u, cld(l), cld(l + 2), cld(l + 3));
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = __builtin_fma(g, cld(pr + c), acc[c]);
  }
  if (!live) return;
  double* o = tp + fb.pbase * NC + (int64_t)s * NC * fb.nsamp + n;
#pragma unroll
  for (int c = 0; c < NC; ++c) o[(int64_t)c * fb.nsamp] = acc[c];
}

template <int NC>
__global__ __launch_bounds__(GF_SCH) void k_gf_tsum(const FacBlock* __restrict__ fbs,
                                                    const int* __restrict__ run,
                                                    const double* __restrict__ tp,
                                                    double* __restrict__ t) {
  const FacBlock fb = fbs[blockIdx.z];
  if (run && !ldg(run)) return;
  const int n = blockIdx.x * GF_SCH + (int)threadIdx.x;
  if (n >= fb.nsamp) return;
  const double* p = tp + fb.pbase * NC + n;
  double* o = t + (fb.tbase + n) * NC;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    double v = ldg(p + (int64_t)c * fb.nsamp);
    for (int s = 1; s < fb.nslab; ++s) v += ldg(p + ((int64_t)s * NC + c) * fb.nsamp);
    o[c] = v;
  }
}

template <int NC>
__global__ __launch_bounds__(WAVE * GF_QCH) void k_gf_q(const FacBlock* __restrict__ fbs,
                                                        PassArgs pa, const double* __restrict__ t,
                                                        double* __restrict__ partials) {
  // a wave's 64 rows x 16 words of bits (padded rows), then, behind a barrier, the
  // four chunk sums: one buffer
  constexpr size_t SB_BYTES = sizeof(uint32_t) * GF_QCH * GF_TILE * 17;
  constexpr size_t RED_BYTES = sizeof(double) * GF_QCH * NC * GF_TILE;
  __shared__ __attribute__((aligned(16))) unsigned char smem[SB_BYTES > RED_BYTES ? SB_BYTES : RED_BYTES];
  uint32_t (*sb)[GF_TILE][17] = reinterpret_cast<uint32_t (*)[GF_TILE][17]>(smem);
  double (*red)[NC][GF_TILE] = reinterpret_cast<double (*)[NC][GF_TILE]>(smem);
  const FacBlock fb = fbs[blockIdx.z];
  if (pa.run && !ldg(pa.run)) return;
  const int i0 = blockIdx.x * GF_TILE;
  if (i0 >= fb.n) return;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int nw = (fb.nsamp + 15) / 16;
  const int wpc = (nw + GF_QCH - 1) / GF_QCH;          // words per sample chunk
  const int w0 = wv * wpc, w1 = min(nw, w0 + wpc);     // this wave's words (none: w0 >= w1)
  const int iters = (wpc + 15) / 16;                   // the same for every wave: barriers inside
  const int i = i0 + lane;
  const bool live = i < fb.n;
  double t0 = 0.0, t2 = 0.0, t3 = 0.0;
  if (live) {
    const double* l = fb.lut + 4 * (int64_t)i;
    t0 = ldg(l), t2 = ldg(l + 2), t3 = ldg(l + 3);
  }
  double acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.0;
  const int lw = lane & 15, lr = lane >> 4;
#pragma unroll 1
  for (int it = 0; it < iters; ++it) {
    const int wb = w0 + 16 * it;
    if (it) __syncthreads();   // the tile before this one has been read
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int r = lr + 4 * k;
      uint32_t v = 0u;
      if (i0 + r < fb.n && wb + lw < w1) v = ldg(fb.bits + (int64_t)(i0 + r) * fb.stride_w + wb + lw);
      sb[wv][r][lw] = v;
    }
    __syncthreads();
    const int nwd = min(16, w1 - wb);
    for (int k = 0; k < nwd; ++k) {
      uint32_t v = sb[wv][lane][k];
      const int s0 = 16 * (wb + k);
      const int ns = min(16, fb.nsamp - s0);   // the last word's padding is never a sample
      const double* tr = t + (fb.tbase + s0) * NC;
      if (ns == 16) {
#pragma unroll 4
        for (int e = 0; e < 16; ++e) {
          const double g = gf_pick(v & 3u, t0, t2, t3);
          v >>= 2;
#pragma unroll
          for (int c = 0; c < NC; ++c) acc[c] = __builtin_fma(g, cld(tr + e * NC + c), acc[c]);
        }
      } else {
        for (int e = 0; e < ns; ++e) {
          const double g = gf_pick(v & 3u, t0, t2, t3);
          v >>= 2;
#pragma unroll
          for (int c = 0; c < NC; ++c) acc[c] = __builtin_fma(g, cld(tr + e * NC + c), acc[c]);
        }
      }
    }
  }
  __syncthreads();   // every wave has read its last tile of bits
#pragma unroll
  for (int c = 0; c < NC; ++c) red[wv][c][lane] = acc[c];
  __syncthreads();
  if (wv != 0) return;
  const int64_t idx = fb.voff + i;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    double y = red[0][c][lane];
#pragma unroll
    for (int q = 1; q < GF_QCH; ++q) y += red[q][c][lane];
    double contrib = 0.0;
    if (live) {
      const double in = pa.in[c][idx];
      const double o = pa.c1[c] * y + pa.c2[c] * in;
      pa.out[c][idx] = o;
      if (pa.yout[c]) pa.yout[c][idx] = pa.ys1 * y + pa.ys0 * in;
      if (pa.dot[c]) contrib = pa.dot[c][idx] * o;
    }
    contrib = wave_sum(contrib);
    if (lane == 0) partials[(int64_t)(fb.part0 + (int)blockIdx.x) * NC + c] = contrib;
  }
}

template <int NC>
static hipError_t launch_nc(const FacBlock* d_fb, int nfb, int gx_t, int gy_t, int gx_q,
                            const PassArgs& pa, double* d_pk, double* d_t, double* d_tp,
                            double* d_part, hipStream_t st) {
  hipLaunchKernelGGL(k_gf_pack<NC>, dim3(gy_t * (GF_SLAB / GF_SCH), 1, nfb), dim3(GF_SCH), 0, st,
                     d_fb, pa, d_pk);
  hipLaunchKernelGGL(k_gf_t<NC>, dim3(gx_t, gy_t, nfb), dim3(GF_SCH), 0, st, d_fb, pa.run, d_pk,
                     d_tp);
  hipLaunchKernelGGL(k_gf_tsum<NC>, dim3(gx_t, 1, nfb), dim3(GF_SCH), 0, st, d_fb, pa.run, d_tp,
                     d_t);
  hipLaunchKernelGGL(k_gf_q<NC>, dim3(gx_q, 1, nfb), dim3(WAVE * GF_QCH), 0, st, d_fb, pa, d_t,
                     d_part);
  return hipGetLastError();
}

hipError_t launch_geno_factor(int nc, const FacBlock* d_fb, int nfb, int gx_t, int gy_t, int gx_q,
                              const PassArgs& pa, double* d_pk, double* d_t, double* d_tp,
                              double* d_part, hipStream_t st) {
  if (nfb < 1 || nfb > 65535 || gx_t < 1 || gy_t < 1 || gy_t > 65535 || gx_q < 1)
    return hipErrorInvalidValue;
  switch (nc) {
#define SGV_GF_CASE(N) \
  case N: return launch_nc<N>(d_fb, nfb, gx_t, gy_t, gx_q, pa, d_pk, d_t, d_tp, d_part, st);
    SGV_GF_CASE(1) SGV_GF_CASE(2) SGV_GF_CASE(3) SGV_GF_CASE(4) SGV_GF_CASE(5) SGV_GF_CASE(6)
    SGV_GF_CASE(7) SGV_GF_CASE(8) SGV_GF_CASE(9) SGV_GF_CASE(10) SGV_GF_CASE(11) SGV_GF_CASE(12)
    SGV_GF_CASE(13) SGV_GF_CASE(14) SGV_GF_CASE(15) SGV_GF_CASE(16)
#undef SGV_GF_CASE
    default: return hipErrorInvalidValue;
  }
}

}  // namespace sgv
