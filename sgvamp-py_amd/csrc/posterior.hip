// Per-marker posterior of the spike-and-slab prior at the denoiser's inputs:
// inclusion probability, log-odds of inclusion, posterior variance, the slab
// responsibilities, and three per-chunk partials (sum pip, sum var, count of
// pip >= thr) for the ordered reductions of vec.hip.  A translation unit of its
// own (vec.hip's flags, -ffp-contract=off) so that vec.hip's code objects do
// not move with it.
//
// The model (the meta denoiser's): t = sum_k r1_k a_k gam1_k observes x with
// precision G = sum_k a_k gam1_k; slab l has q_l = 1 / (G sigma_l + 1), s2_l =
// sigma_l q_l, x | l ~ N(t s2_l, s2_l), and against the spike the log-weight
//   D_l = log(lam omega_l / (1 - lam)) + (t^2 / 2) s2_l + log(q_l) / 2.
// Everything is formed in the log domain around max_l D_l, so the tails (|z| of
// 40 in 65 cohorts) and lam next to 0 or 1 stay finite and do not cancel.
#include "common.h"

namespace sgv {

constexpr int MPT = CHUNK / VTHREADS;   // markers per thread, as vec.hip's kernels
static_assert(CHUNK % VTHREADS == 0, "markers per thread");

// KM: cohort bound of the instantiation (vr holds MPT x KM values), as k_denoise
template <int KM>
__global__ __launch_bounds__(VTHREADS) void k_posterior(const ChunkDesc* __restrict__ chs,
                                                        PosteriorArgs a,
                                                        double* __restrict__ part) {
  const ChunkDesc ch = chs[blockIdx.x];
  // loads of the thread's MPT markers first, then the markers in order
  double vr[MPT][KM];
#pragma unroll
  for (int j = 0; j < MPT; ++j) {
    const int t = threadIdx.x + j * VTHREADS;
    if (t < ch.len) {
      const int64_t i = ch.voff + t;
      if (a.inner) {
        vr[j][0] = a.inner[i];
      } else {
#pragma unroll
        for (int k = 0; k < KM; ++k)
          if (k < a.K) vr[j][k] = a.r1[k][i];
      }
    }
  }
  double acc[POST_SUMS] = {0.0, 0.0, 0.0};   // sum pip, sum var, count(pip >= thr)
#pragma unroll
  for (int j = 0; j < MPT; ++j) {
    const int tt = threadIdx.x + j * VTHREADS;
    if (tt >= ch.len) continue;
    const int64_t i = ch.voff + tt;
    // t = sum_k r1_k ag_k in cohort order, as the denoiser's np.inner
    double t = 0.0;
    if (a.inner) {
      t = vr[j][0];
    } else {
#pragma unroll
      for (int k = 0; k < KM; ++k)
        if (k < a.K) t = (k == 0) ? vr[j][0] * a.ag[0] : t + vr[j][k] * a.ag[k];
    }
    const double h = t * t / 2;
    double D[MAXL];
    double mx = 0.0;
#pragma unroll
    for (int l = 0; l < MAXL; ++l)
      if (l < a.nslab) {
        D[l] = (a.cw[l] + h * a.s2[l]) + a.hq[l];
        mx = (l == 0 || D[l] > mx) ? D[l] : mx;
      }
    // slab responsibilities given inclusion and the slab-conditional moments
    double E[MAXL];
    double se = 0.0;
#pragma unroll
    for (int l = 0; l < MAXL; ++l)
      if (l < a.nslab) {
        E[l] = exp(D[l] - mx);
        se = (l == 0) ? E[l] : se + E[l];
      }
    double m1 = 0.0;   // sum_l resp_l s2_l
#pragma unroll
    for (int l = 0; l < MAXL; ++l)
      if (l < a.nslab) {
        E[l] = E[l] / se;
        m1 = (l == 0) ? E[l] * a.s2[l] : m1 + E[l] * a.s2[l];
      }
    const double ms = t * m1;   // slab mean
    double vs = m1;             // E Var(x | l) + Var E(x | l) over the slabs, terms >= 0
#pragma unroll
    for (int l = 0; l < MAXL; ++l)
      if (l < a.nslab) {
        const double d = t * a.s2[l] - ms;
        vs = vs + E[l] * (d * d);
      }
    // log-odds: max + log-sum-exp; lam == 0 / 1 (a.edge) are exact edges
    double lo = mx + log(se);
    if (a.edge < 0) lo = -__builtin_inf();
    if (a.edge > 0) lo = __builtin_inf();
    // the sigmoid and its complement, each from the branch that does not cancel
    double pip, qip;
    if (lo >= 0) {
      const double e = exp(-lo);
      pip = 1 / (1 + e);
      qip = e / (1 + e);
    } else {
      const double e = exp(lo);
      pip = e / (1 + e);
      qip = 1 / (1 + e);
    }
    const double var = pip * vs + pip * qip * (ms * ms);
    a.pip[i] = pip;
    a.lodds[i] = lo;
    a.var[i] = var;
#pragma unroll
    for (int l = 0; l < MAXL; ++l)
      if (l < a.nslab && a.resp[l]) a.resp[l][i] = E[l];
    acc[0] += pip;
    acc[1] += var;
    acc[2] += (pip >= a.thr) ? 1.0 : 0.0;
  }
  block_reduce_store<POST_SUMS>(acc, part + (int64_t)blockIdx.x * POST_SUMS, POST_SUMS);
}

hipError_t launch_posterior(const ChunkDesc* d_ch, int nch, const PosteriorArgs& a, double* d_part,
                            hipStream_t st) {
#define L_POST(KM) \
  hipLaunchKernelGGL(k_posterior<KM>, dim3(nch), dim3(VTHREADS), 0, st, d_ch, a, d_part)
  if (a.K < 1 || a.K > MAXK || a.nslab < 1 || a.nslab > MAXL) return hipErrorInvalidValue;
  if (!a.pip || !a.lodds || !a.var) return hipErrorInvalidValue;
  if (a.inner || a.K <= 1) L_POST(1);   // K > MAXK: t precomputed (launch_den_inner)
  else if (a.K <= 2) L_POST(2);
  else if (a.K <= 4) L_POST(4);
  else if (a.K <= 8) L_POST(8);
  else if (a.K <= 16) L_POST(16);
  else L_POST(MAXK);
#undef L_POST
  return hipGetLastError();
}

}  // namespace sgv
