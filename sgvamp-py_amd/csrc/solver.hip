// The solver half of libsgvamp_hip.so's host side: the LMMSE step
// (src/sgvamp.py:301-364) over the batched CG of cg.hip, the metrics, and the
// one-call outer iteration with its worker thread (:222-387).  The prior side
// (denoiser, posterior, EM, MLE) is prior.hip.
#include "ctx.h"

// The vectors of one LMMSE cohort group (cohorts g0 .. g0 + K - 1, CG columns
// 2 k and 2 k + 1 of cohort k: xhat2 and Sigma2 u) and its slices of the
// solver state: the one place that indexes the context by group
struct GroupView {
  int K, ncol;
  double *X[MAXC], *X0[MAXC], *Rr[MAXC], *P[MAXC], *Q[MAXC], *RX0[MAXC], *RXp[MAXC], *Y[MAXC];
  double *r[MAXKG], *r1[MAXKG], *r2[MAXKG], *U[MAXKG];
  int ld[MAXC];        // the column's LD matrix (its cohort's)
  int* xnz;            // [ncol] x0.any()
  int* rx0_valid;      // [ncol] RX0 == R_s X
  const double* N;     // [K] cohort sizes
  GroupView(sgv_ctx* c, int g0, int Kg) : K(Kg), ncol(2 * Kg) {
    for (int j = 0; j < ncol; ++j) {
      const int cj = 2 * g0 + j;
      X[j] = c->X[cj], X0[j] = c->X0[cj], Rr[j] = c->Rr[cj], P[j] = c->P[cj], Q[j] = c->Q[cj];
      RX0[j] = c->RX0[cj], RXp[j] = c->RXp[cj], Y[j] = c->Y[cj];
      ld[j] = c->ld_of[g0 + j / 2];
    }
    for (int k = 0; k < K; ++k)
      r[k] = c->r[g0 + k], r1[k] = c->r1[g0 + k], r2[k] = c->r2[g0 + k], U[k] = c->U[g0 + k];
    xnz = c->xnz.data() + 2 * g0;
    rx0_valid = c->rx0_valid.data() + 2 * g0;
    N = c->Ncoh.data() + g0;
  }
};

// z, xRx, Tr(R Sigma2) and the learned gamw of one cohort (:350-363)
static void gamw_outputs(double N, double xRx, double TrRSigma2, double* o) {
  double z = N - 2 * o[SGV_O_XR] + xRx;                            // :352
  if (z < 0) z = 0;                                                // :353-354
  o[SGV_O_Z] = z;
  o[SGV_O_XRX] = xRx;
  o[SGV_O_TRRSIGMA2] = TrRSigma2;
  o[SGV_O_GAMW] = 1 / (z / N + TrRSigma2 / N);                     // :363
}

// LMMSE of the cohorts g0 .. g0 + Kg - 1 (Kg <= MAXKG: 2 Kg <= MAXC CG columns,
// one batched CG loop); per-cohort inputs/outputs are the group's slices
static int lmmse_group(sgv_ctx* c, int g0, int Kg, const double* gamw, const double* gam2,
                       const double* alpha1, const double* alpha2_prev, int cg_maxit, double rtol,
                       int lmmse_damp, double rho, int learn_gamw, double* out, int* cg_out,
                       int* passes_out) {
  const GroupView v(c, g0, Kg);
  const int K = v.K, ncol = v.ncol;
  const double s = c->s;
  int passes = 0;
  // a pass y = R_s x over the columns of LD matrix ld that `take` accepts: RX0 = R_s X
  // (valid from here on), dotted with w(j) (null: no dot)
  auto rs_pass_cols = [&](int ld, auto take, auto w) {
    return gather_cols(
        ncol, [&](int j) { return v.ld[j] == ld && take(j); },
        [&](PassArgs& pa, int n, int j) {
          pa.in[n] = v.X[j];
          pa.out[n] = v.RX0[j];
          pa.dot[n] = w(j);
          pa.c1[n] = 1.0 - s;
          pa.c2[n] = s;
          v.rx0_valid[j] = 1;
        });
  };

  // warm start needs R_s x0: carried from the previous iteration (rs_rec), or the
  // previous gamw pass; a pass only when X was set from outside
  for (int ld = 0; ld < c->nld; ++ld) {
    const PassCols pc = rs_pass_cols(
        ld, [&](int j) { return v.xnz[j] && !v.rx0_valid[j]; },
        [](int) -> const double* { return nullptr; });
    if (pc.nc) {
      CHK(ld_pass(c, ld, pc.nc, pc.pa));
      ++passes;
    }
  }

  // r2, mu2, r0 = b - A x0, p0 = r0 (:305-313, iterative.py:376-392)
  InitArgs ia{};
  ia.xhat1 = c->xhat1;
  ia.K = K;
  ia.save_x0 = lmmse_damp;
  for (int k = 0; k < K; ++k) {
    ia.cp.r[k] = v.r[k];
    ia.cp.r1[k] = v.r1[k];
    ia.cp.r2[k] = v.r2[k];
    ia.cp.u[k] = v.U[k];
    ia.alpha1[k] = alpha1[k];
    ia.gamw[k] = gamw[k];
    ia.gam2[k] = gam2[k];
  }
  for (int j = 0; j < ncol; ++j) {
    ia.col.X[j] = v.X[j];
    ia.col.X0[j] = v.X0[j];
    ia.col.Rr[j] = v.Rr[j];
    ia.col.P[j] = v.P[j];
    ia.col.Q[j] = v.Q[j];
    ia.col.RX0[j] = v.RX0[j];
    ia.col.RXp[j] = c->rs_rec ? v.RXp[j] : nullptr;
    ia.warm[j] = v.xnz[j];
  }
  double tot[2 * MAXC];
  const bool dev_init = c->cg_pipe;   // CG prologue on the device: no host round trip
  // with a communicator and one LD matrix for the group's columns: the prologue's
  // sums share iteration 0's exchange (cg_loop_dev, CgMerge0); without an
  // iteration 0 (cg_maxit == 0) nothing would reduce them or set the CG state
  bool one_ld = true;
  for (int j = 1; j < ncol; ++j) one_ld &= v.ld[j] == v.ld[0];
  const bool merge0 = dev_init && (c->comm || c->host_ag) && one_ld && cg_maxit > 0;
  if (merge0) CHK(grow(c, &c->d_part2, &c->part2_cap, (size_t)c->nch * 2 * MAXC));
  HIPCHK(launch_lmmse_init(c->d_ch, c->nch, ia, merge0 ? c->d_part2 : c->d_part, c->st));
  CgMerge0 mg;
  if (merge0) {
    mg.part = c->d_part2;
    mg.rtol = rtol;
    mg.X = v.X;
    mg.RX = v.RX0;
  } else if (dev_init) {
    CHK(reduce_dev(c, 2 * MAXC, c->d_ch_begin, identity_map(), c->d_tot));
    HIPCHK(launch_cg_init(c->d_cgs, c->d_tot, rtol, ncol, c->d_ch, c->nch, v.X, v.RX0, c->st));
  } else {
    CHK(reduce_host(c, 2 * MAXC, c->d_ch_begin, tot));
  }
  // carried: RX0 follows X through the CG; otherwise the gamw pass refreshes it
  for (int j = 0; j < ncol; ++j) v.rx0_valid[j] = c->rs_rec ? 1 : 0;

  CgCols cc;
  cc.ncol = ncol;
  cc.s = s;
  double rhov[MAXC], atol[MAXC];
  int active[MAXC], iters[MAXC], info[MAXC];
  for (int j = 0; j < ncol; ++j) {
    const int k = j / 2;
    cc.col_ld[j] = v.ld[j];
    cc.c1[j] = gamw[k] * (1.0 - s);           // A = gamw R_s + gam2 I (:312)
    cc.c2[j] = gamw[k] * s + gam2[k];
    cc.X[j] = v.X[j];
    cc.Rr[j] = v.Rr[j];
    cc.P[j] = v.P[j];
    cc.Q[j] = v.Q[j];
    if (c->rs_rec) {
      cc.RX[j] = v.RX0[j];
      cc.Y[j] = v.Y[j];
    }
    active[j] = 1;                            // dev_init: k_cg_init decides
  }
  if (!dev_init) {
    cg_prologue(ncol, tot, tot + MAXC, rtol, atol, rhov, active);
    for (int j = 0; j < ncol; ++j)
      if (!active[j]) {                       // x = b = 0
        HIPCHK(hipMemsetAsync(v.X[j], 0, sizeof(double) * c->Mpad, c->st));
        HIPCHK(hipMemsetAsync(v.RX0[j], 0, sizeof(double) * c->Mpad, c->st));   // R_s 0
      }
  }
  CHK(dev_init ? cg_loop_dev(c, cc, nullptr, nullptr, cg_maxit, active, iters, info, &passes,
                             merge0 ? &mg : nullptr)
               : cg_run(c, cc, rhov, atol, cg_maxit, active, iters, info, &passes));

  // damping, u.Sigma2_u, xhat2.r, x.any() (:322-323, 338, 352)
  PostArgs po{};
  po.K = K;
  po.damp = lmmse_damp;
  po.rs = c->rs_rec;
  po.rho = rho;
  for (int j = 0; j < ncol; ++j) {
    po.X[j] = v.X[j];
    po.X0[j] = v.X0[j];
    po.RX[j] = v.RX0[j];
    po.RXp[j] = v.RXp[j];
  }
  for (int k = 0; k < K; ++k) {
    po.u[k] = v.U[k];
    po.r[k] = v.r[k];
  }
  HIPCHK(launch_lmmse_post(c->d_ch, c->nch, po, c->d_part, c->st));
  double pt[4 * MAXKG + MAXC];
  // r1 = (xhat2 - alpha2 r2) / (1 - alpha2) (:348): alpha2 from the device-reduced
  // Tr(Sigma2) (trs, dev_init) or by value
  R1Args ra{};
  ra.K = K;
  ra.Mtot = (double)c->Mtot;
  ra.rho = rho;
  ra.damp = lmmse_damp;
  for (int k = 0; k < K; ++k) {
    ra.X[k] = v.X[2 * k];
    ra.r2[k] = v.r2[k];
    ra.r1[k] = v.r1[k];
    ra.gam2[k] = gam2[k];
    ra.alpha2_prev[k] = alpha2_prev[k];
  }
  if (dev_init) {
    // the update is queued before the host reads the sums (which it computes
    // alpha2 from as well)
    CHK(reduce_dev(c, 4 * MAXKG + MAXC, c->d_ch_begin, identity_map(), c->d_tot));
    ra.trs = c->d_tot;
    HIPCHK(launch_r1_update(c->d_ch, c->nch, ra, c->st));
    HIPCHK(launch_copy_f64(c->h_tot, c->d_tot, 4 * MAXKG + MAXC, c->st));
    CHK(stream_wait(c));
    resolve_timers(c);
    std::memcpy(pt, c->h_tot, sizeof(pt));
  } else {
    CHK(reduce_host(c, 4 * MAXKG + MAXC, c->d_ch_begin, pt));
  }
  for (int j = 0; j < ncol; ++j) v.xnz[j] = pt[2 * MAXKG + j] > 0.0;

  for (int k = 0; k < K; ++k) {
    const double TrSigma2 = pt[k];
    double a2 = gam2[k] * TrSigma2 / (double)c->Mtot;              // :340
    if (lmmse_damp) a2 = rho * a2 + (1 - rho) * alpha2_prev[k];    // :345-346
    const double g1 = gam2[k] * (1 - a2) / a2;                    // :347
    double* o = out + (size_t)k * SGV_LMMSE_NOUT;
    o[SGV_O_TRSIGMA2] = TrSigma2;
    o[SGV_O_ALPHA2] = a2;
    o[SGV_O_GAM1] = g1;
    o[SGV_O_XR] = pt[MAXKG + k];
    o[SGV_O_Z] = 0.0;
    o[SGV_O_TRRSIGMA2] = 0.0;
    o[SGV_O_XRX] = 0.0;
    o[SGV_O_GAMW] = gamw[k];
    ra.alpha2[k] = a2;
    cg_out[4 * k + 0] = iters[2 * k];
    cg_out[4 * k + 1] = info[2 * k];
    cg_out[4 * k + 2] = iters[2 * k + 1];
    cg_out[4 * k + 3] = info[2 * k + 1];
  }
  if (!dev_init) HIPCHK(launch_r1_update(c->d_ch, c->nch, ra, c->st));

  if (learn_gamw && c->rs_rec) {  // :350-363 from the carried products: no pass
    for (int k = 0; k < K; ++k)
      gamw_outputs(v.N[k], pt[2 * MAXKG + MAXC + k], pt[3 * MAXKG + MAXC + k],
                   out + (size_t)k * SGV_LMMSE_NOUT);
  } else if (learn_gamw) {  // :350-363; R_s [xhat2, Sigma2_u] is also the next warm start's R_s x0
    for (int ld = 0; ld < c->nld; ++ld) {
      const PassCols pc = rs_pass_cols(
          ld, [](int) { return true; },
          [&](int j) -> const double* { return j % 2 == 0 ? v.X[j] : v.U[j / 2]; });
      if (!pc.nc) continue;
      CHK(ld_pass(c, ld, pc.nc, pc.pa));
      ++passes;
      double gt[MAXC];
      CHK(reduce_dev(c, pc.nc, ld_parts(c, ld), pc.map, c->h_tot));
      CHK(stream_wait(c));
      resolve_timers(c);
      std::memcpy(gt, c->h_tot, sizeof(double) * ncol);
      for (int k = 0; k < K; ++k)
        if (v.ld[2 * k] == ld)
          gamw_outputs(v.N[k], gt[2 * k], gt[2 * k + 1], out + (size_t)k * SGV_LMMSE_NOUT);
    }
  } else {
    CHK(stream_wait(c));
  }
  if (passes_out) *passes_out = passes;
  return SGV_OK;
}

extern "C" int sgv_lmmse(sgv_ctx* c, int it, const double* gamw, const double* gam2,
                         const double* alpha1, const double* alpha2_prev, const int8_t* probes,
                         int cg_maxit, double rtol, int lmmse_damp, double rho, int learn_gamw,
                         double* out, int* cg_out, int* passes_out) {
  ENTER(c);
  (void)it;
  if (!gamw || !gam2 || !alpha1 || !alpha2_prev || !probes || !out || !cg_out || cg_maxit < 0)
    return fail(c, SGV_ERR_ARG, "sgv_lmmse: bad arguments");
  const int K = c->K;

  // probes u_k (:326), int8 +-1 -> f64; uploaded at the start of sgv_step, or now
  int ps = c->pref_slot;
  if (ps < 0 || c->pref_src != probes) CHK(probe_upload(c, probes, &ps));
  c->pref_slot = -1;
  c->pref_src = nullptr;
  HIPCHK(hipStreamWaitEvent(c->st, c->ev_probe[ps], 0));
  for (int k = 0; k < K; ++k)
    HIPCHK(launch_unpack_i8(c->d_ch, c->nch, c->d_ch_doff,
                            c->d_probe + ps * c->probe_cap + (size_t)k * c->Mloc, c->U[k], c->st));
  HIPCHK(hipEventRecord(c->ev_unpk[ps], c->st));

  // cohorts in groups of MAXKG (2 MAXKG = MAXC CG columns per LD pass): the
  // LMMSE of a cohort touches only its own vectors and the shared xhat1, so the
  // groups run one after another with the same per-cohort arithmetic
  int passes = 0;
  for (int g0 = 0; g0 < K; g0 += MAXKG) {
    const int Kg = std::min(MAXKG, K - g0);
    int gp = 0;
    CHK(lmmse_group(c, g0, Kg, gamw + g0, gam2 + g0, alpha1 + g0, alpha2_prev + g0, cg_maxit, rtol,
                    lmmse_damp, rho, learn_gamw, out + (size_t)g0 * SGV_LMMSE_NOUT, cg_out + 4 * g0,
                    &gp));
    passes += gp;
  }
  if (passes_out) *passes_out = passes;
  return SGV_OK;
}

extern "C" int sgv_metrics(sgv_ctx* c, double* out4) {
  ENTER(c);
  if (!out4) return fail(c, SGV_ERR_ARG, "out4 is null");
  HIPCHK(launch_metrics(c->d_ch, c->nch, c->xhat1, c->x0, c->d_part, c->st));
  return reduce_host(c, 4, c->d_ch_begin, out4);
}

// The same sums, queued without a host wait (xhat1 and x0 are not written
// again before sgv_metrics_end); the ordered totals land in pinned memory.
// With the host exchange the reduction itself waits, so begin completes it.
extern "C" int sgv_metrics_begin(sgv_ctx* c) {
  ENTER(c);
  if (!c->h_met) {
    HIPCHK(hipHostMalloc(&c->h_met, sizeof(double) * 4, hipHostMallocCoherent));
    HIPCHK(hipEventCreateWithFlags(&c->ev_met, hipEventDisableTiming));
  }
  HIPCHK(launch_metrics(c->d_ch, c->nch, c->xhat1, c->x0, c->d_part, c->st));
  CHK(reduce_dev(c, 4, c->d_ch_begin, identity_map(), c->h_met));
  HIPCHK(hipEventRecord(c->ev_met, c->st));
  c->met_pending = 1;
  return SGV_OK;
}

extern "C" int sgv_metrics_end(sgv_ctx* c, double* out4) {
  ENTER(c);
  if (!out4) return fail(c, SGV_ERR_ARG, "out4 is null");
  if (!c->met_pending) return fail(c, SGV_ERR_ARG, "sgv_metrics_end without sgv_metrics_begin");
  hipError_t e;
  while ((e = hipEventQuery(c->ev_met)) == hipErrorNotReady) __builtin_ia32_pause();
  if (e != hipSuccess) return fail(c, SGV_ERR_HIP, "metrics wait: %s", hipGetErrorString(e));
  std::memcpy(out4, c->h_met, sizeof(double) * 4);
  c->met_pending = 0;
  return SGV_OK;
}

// ---------------------------------------------------------------------------
// one outer iteration in the shim (src/sgvamp.py:222-387 minus the files and
// logs): the host returns to the caller once, not between the phases
// ---------------------------------------------------------------------------
static int step_impl(sgv_ctx* c, int it, int flags, int em_maxit, int nslab,
                     const double* sigmas, const double* a, double* lam_io, double* omegas_io,
                     const double* gam1s, double rho, const double* gamw,
                     const double* alpha1_prev, const double* alpha2_prev,
                     const int8_t* probes, int cg_maxit, double rtol, int out_slot,
                     double* res, int* ires, double* out, int* cg_out, int staged) {
  if (!sigmas || !a || !lam_io || !omegas_io || !gam1s || !gamw || !alpha1_prev ||
      !alpha2_prev || !probes || !res || !ires || !out || !cg_out || out_slot >= NOUT_SLOTS)
    return fail(c, SGV_ERR_ARG, "sgv_step: bad arguments");
  const bool post = (flags & SGV_STEP_POSTERIOR) != 0;
  if (post && !c->post_on)
    return fail(c, SGV_ERR_STATE, "SGV_STEP_POSTERIOR without sgv_set_posterior_outputs");
  const int K = c->K;
  c->chain.valid = 0;   // a step chained behind this one fails unless this one completes
  res[0] = 0.0;
  ires[0] = 0;
  // this step's probes go up now, behind nothing: the copy overlaps EM/denoiser
  // (a step begun behind another had its host copy made by sgv_step_begin)
  if (staged >= 0) CHK(probe_issue(c, staged, &c->pref_slot));
  else CHK(probe_upload(c, probes, &c->pref_slot));
  c->pref_src = probes;
  if (flags & SGV_STEP_EM) {   // :250-257
    CHK(sgv_em(c, gam1s, a, nslab, sigmas, em_maxit, lam_io, omegas_io, &ires[0], &res[0]));
  } else if (flags & SGV_STEP_MLE) {   // :244-247
    CHK(sgv_mle_update(c, gam1s, a, nslab, sigmas, lam_io, omegas_io, &c->mle_gam, &ires[0]));
    res[0] = c->mle_gam;
  }
  if (nslab < 1 || nslab > MAXL) return fail(c, SGV_ERR_ARG, "sgv_step: nslab=%d", nslab);
  // denoiser (:270-291); the output copies and metrics (:281-283, 379-387) are
  // queued behind it before the host waits for the derivative sums
  bool met_fused = false;
  CHK(denoise_enqueue(c, gam1s, a, *lam_io, nslab, omegas_io, sigmas, rho,
                      (flags & SGV_STEP_DENOISE_DAMP) ? 1 : 0, (flags & SGV_STEP_METRICS) != 0,
                      &met_fused));
  HIPCHK(hipEventRecord(c->ev_den, c->st));
  // the posterior at the denoiser's inputs: the same gam1s and r1, the prior
  // after this step's EM / MLE update; its rows ride in the output slot
  if (post) {
    CHK(posterior_enqueue(c, gam1s, a, *lam_io, nslab, omegas_io, sigmas, c->post_thr, false));
  }
  if (out_slot >= 0) CHK(outputs_begin(c, out_slot, post));
  if ((flags & SGV_STEP_METRICS) && !met_fused) CHK(sgv_metrics_begin(c));
  CHK(event_spin(c, c->ev_den));
  std::vector<double> der(c->h_tot, c->h_tot + K), alpha1(K), gam2(K);
  if (met_fused)   // the metrics' ordered sums (sgv_metrics order), long done
    for (int j = 0; j < 4; ++j) res[1 + 2 * K + j] = c->h_tot[K + j];
  for (int k = 0; k < K; ++k) {
    double a1 = der[k] / (double)c->Mtot;                           // np.mean (:285)
    if (flags & SGV_STEP_ALPHA1_DAMP) a1 = rho * a1 + (1 - rho) * alpha1_prev[k];   // :290-291
    alpha1[k] = a1;
    gam2[k] = gam1s[k] * (1 - a1) / a1;                             // :305
    res[1 + k] = a1;
    res[1 + K + k] = gam2[k];
  }
  int passes = 0;
  CHK(sgv_lmmse(c, it, gamw, gam2.data(), alpha1.data(), alpha2_prev, probes, cg_maxit, rtol,
                (flags & SGV_STEP_LMMSE_DAMP) ? 1 : 0, rho, (flags & SGV_STEP_LEARN_GAMW) ? 1 : 0,
                out, cg_out, &passes));
  ires[1] = passes;
  if ((flags & SGV_STEP_METRICS) && !met_fused) CHK(sgv_metrics_end(c, res + 1 + 2 * K));
  if (post) {   // the ordered sums, queued ahead of the LMMSE: long done
    CHK(stream_wait(c));
    for (int j = 0; j < POST_SUMS; ++j) res[1 + 2 * K + 4 + j] = c->h_post[j];
  }
  // inputs of a chained next step: src/sgvamp.py:347, 363-374 (gamw clamped to
  // >= 1 after it is logged, as Python's max(gamw, 1.0))
  sgv_ctx::Chain& ch = c->chain;
  for (int k = 0; k < K; ++k) {
    const double* o = out + (size_t)k * SGV_LMMSE_NOUT;
    ch.gam1[k] = o[SGV_O_GAM1];
    const double gw = (flags & SGV_STEP_LEARN_GAMW) ? o[SGV_O_GAMW] : gamw[k];
    ch.gamw[k] = (1.0 > gw) ? 1.0 : gw;
    ch.alpha1[k] = alpha1[k];
    ch.alpha2[k] = o[SGV_O_ALPHA2];
  }
  ch.lam = *lam_io;
  for (int l = 0; l < nslab; ++l) ch.om[l] = omegas_io[l];
  ch.valid = 1;
  return SGV_OK;
}

extern "C" int sgv_step(sgv_ctx* c, int it, int flags, int em_maxit, int nslab,
                        const double* sigmas, const double* a, double* lam_io, double* omegas_io,
                        const double* gam1s, double rho, const double* gamw,
                        const double* alpha1_prev, const double* alpha2_prev,
                        const int8_t* probes, int cg_maxit, double rtol, int out_slot,
                        double* res, int* ires, double* out, int* cg_out) {
  ENTER(c);
  return step_impl(c, it, flags, em_maxit, nslab, sigmas, a, lam_io, omegas_io, gam1s, rho, gamw,
                   alpha1_prev, alpha2_prev, probes, cg_maxit, rtol, out_slot, res, ires, out,
                   cg_out, -1);
}

// Hand-offs spin (a futex wake costs tens of microseconds, the GPU idles for
// it): the worker spins up to ~2 ms for the next step before it blocks, and
// sgv_step_end spins for the step it waits on.  Steps run in begin order.
static void worker_main(sgv_ctx* c) {
  (void)hipSetDevice(c->dev);
  for (;;) {
    sgv_ctx::Job& j = c->jobs[c->job_run % 2];
    const auto t0 = std::chrono::steady_clock::now();
    while (j.state.load(std::memory_order_acquire) != 1 && !c->worker_quit.load()) {
      __builtin_ia32_pause();
      if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) {
        std::unique_lock<std::mutex> lk(c->wmu);
        c->wcv.wait(lk, [&] { return j.state.load() == 1 || c->worker_quit.load(); });
      }
    }
    if (j.state.load(std::memory_order_acquire) != 1) return;   // quit
    j.state.store(2);
    j.rc = j.fn();
    ++c->job_run;
    j.state.store(3, std::memory_order_release);
  }
}

extern "C" int sgv_step_begin(sgv_ctx* c, int it, int flags, int em_maxit, int nslab,
                              const double* sigmas, const double* a, double* lam_io,
                              double* omegas_io, const double* gam1s, double rho,
                              const double* gamw, const double* alpha1_prev,
                              const double* alpha2_prev, const int8_t* probes, int cg_maxit,
                              double rtol, int out_slot, double* res, int* ires, double* out,
                              int* cg_out) {
  if (!c) return fail(nullptr, SGV_ERR_ARG, "null context");
  if (nslab < 1 || nslab > MAXL || !sigmas || !a || !gam1s || !gamw || !alpha1_prev ||
      !alpha2_prev || !lam_io || !omegas_io)
    return fail(c, SGV_ERR_ARG, "sgv_step_begin: bad arguments");
  sgv_ctx::Job& j = c->jobs[c->job_begun % 2];
  if (j.state.load() != 0) return fail(c, SGV_ERR_ARG, "sgv_step_begin: two steps already queued");
  // the K- and L-length inputs are copied (a chained step takes gam1, gamw,
  // alpha1, alpha2, lam and omegas from the step before it when it starts);
  // lam_io/omegas_io, probes and the outputs stay the caller's until sgv_step_end
  const int K = c->K;
  std::vector<double> v_sig(sigmas, sigmas + nslab), v_a(a, a + K), v_g1(gam1s, gam1s + K),
      v_gw(gamw, gamw + K), v_a1(alpha1_prev, alpha1_prev + K), v_a2(alpha2_prev, alpha2_prev + K);
  // the probes' host copy is made here, while the step ahead runs on the GPU,
  // so the worker starts this step with the device copy alone (the buffers
  // come from the first step's upload; until then the worker stages them)
  int staged = -1;
  if (probes && c->probe_cap.load(std::memory_order_acquire) >= std::max<size_t>((size_t)K * c->Mloc, 8)) {
    staged = probe_stage(c, probes);
    if (staged < 0) return SGV_ERR_HIP;
  }
  j.fn = [=]() mutable {
    if (flags & SGV_STEP_CHAIN) {
      const sgv_ctx::Chain& ch = c->chain;
      if (!ch.valid) return fail(c, SGV_ERR_ARG, "chained step without a completed step");
      for (int k = 0; k < K; ++k) {
        v_g1[k] = ch.gam1[k];
        v_gw[k] = ch.gamw[k];
        v_a1[k] = ch.alpha1[k];
        v_a2[k] = ch.alpha2[k];
      }
      *lam_io = ch.lam;
      for (int l = 0; l < nslab; ++l) omegas_io[l] = ch.om[l];
    }
    ENTER(c);
    return step_impl(c, it, flags & ~SGV_STEP_CHAIN, em_maxit, nslab, v_sig.data(), v_a.data(),
                     lam_io, omegas_io, v_g1.data(), rho, v_gw.data(), v_a1.data(), v_a2.data(),
                     probes, cg_maxit, rtol, out_slot, res, ires, out, cg_out, staged);
  };
  {
    std::lock_guard<std::mutex> lk(c->wmu);   // a worker about to block sees the job
    j.state.store(1, std::memory_order_release);
  }
  ++c->job_begun;
  if (!c->worker.joinable()) c->worker = std::thread(worker_main, c);
  c->wcv.notify_all();
  return SGV_OK;
}

extern "C" int sgv_step_end(sgv_ctx* c) {
  if (!c) return fail(nullptr, SGV_ERR_ARG, "null context");
  if (c->job_ended == c->job_begun) return fail(c, SGV_ERR_ARG, "sgv_step_end without sgv_step_begin");
  sgv_ctx::Job& j = c->jobs[c->job_ended % 2];
  while (j.state.load(std::memory_order_acquire) != 3) __builtin_ia32_pause();
  const int rc = j.rc;
  j.fn = nullptr;
  j.state.store(0);
  ++c->job_ended;
  return rc;
}
