// The prior side of libsgvamp_hip.so's host code: the meta denoiser
// (src/sgvamp.py:93-114, 270-291), the per-marker posterior at its inputs, the
// EM prior loop (:116-136, 250-257) and the MLE prior update (:139-194, fsolve
// restated in hybrd.cpp).  More than MAXK cohorts run in groups of MAXK
// (for_cohort_groups, ctx.h).
#include "ctx.h"

// ---------------------------------------------------------------------------
// denoiser (src/sgvamp.py:93-114, 270-291)
// ---------------------------------------------------------------------------
// more than MAXK cohorts: t = np.inner(r1, a gam1) over all of them into d_inner,
// one sequential sum continued from group to group (launch_den_inner)
static int den_inner_enqueue(sgv_ctx* c, const double* gam1s, const double* a,
                             const double** inner) {
  CHK(grow(c, &c->d_inner, &c->inner_cap, (size_t)std::max<int64_t>(c->Mpad, 1)));
  *inner = c->d_inner;
  return for_cohort_groups(c->K, [&](int g, int k0, int Kg) -> int {
    DenoiseArgs da{};
    da.K = Kg;
    for (int k = 0; k < Kg; ++k) {
      da.r1[k] = c->r1[k0 + k];
      da.ag[k] = a[k0 + k] * gam1s[k0 + k];
    }
    HIPCHK(launch_den_inner(c->d_ch, c->nch, da, c->d_inner, g == 0 ? 1 : 0, c->st));
    return SGV_OK;
  });
}

// denoiser kernel + the ordered reduction of its derivative sums into h_tot[0..K);
// metrics: the four metrics sums of the new xhat1 (sgv_metrics) in the same
// reduction, h_tot[K .. K + 3] (one exchange instead of two with a communicator;
// not with more than MAXK cohorts) -- returns whether they were fused
int denoise_enqueue(sgv_ctx* c, const double* gam1s, const double* a, double lam, int nslab,
                    const double* omegas, const double* sigmas, double rho, int damp, bool metrics,
                    bool* fused) {
  DenoiseArgs da{};
  da.xhat1 = c->xhat1;
  da.nslab = nslab;
  da.lam = lam;
  da.rho = rho;
  da.damp = damp;
  da.write_x = 1;
  for (int k = 0; k < c->K; ++k) {
    const double ag = a[k] * gam1s[k];                 // self.a * gam1s
    da.sum_ag = (k == 0) ? ag : da.sum_ag + ag;        // builtin sum (:95)
  }
  for (int l = 0; l < nslab; ++l) {
    da.omegas[l] = omegas[l];
    da.sigmas[l] = sigmas[l];
    da.s2[l] = 1.0 / (da.sum_ag + 1.0 / sigmas[l]);     // :95
    da.sq[l] = std::sqrt(da.s2[l] / sigmas[l]);         // np.sqrt(sigma2_meta / sigmas)
  }
  // more than MAXK cohorts: np.inner over all of them first (den_inner_enqueue),
  // then one launch per group for its cohorts' derivative sums; the first also
  // writes xhat1
  const bool one = cohort_groups(c->K) == 1;
  if (!one) CHK(den_inner_enqueue(c, gam1s, a, &da.inner));
  const bool met = metrics && one;
  if (fused) *fused = met;
  return for_cohort_groups(c->K, [&](int g, int k0, int Kg) -> int {
    da.K = Kg;
    for (int k = 0; k < Kg; ++k) {
      da.r1[k] = c->r1[k0 + k];
      da.a[k] = a[k0 + k];
      da.gam1[k] = gam1s[k0 + k];
      da.ag[k] = a[k0 + k] * gam1s[k0 + k];
    }
    da.write_x = g == 0 ? 1 : 0;
    da.x0 = met ? c->x0 : nullptr;
    HIPCHK(launch_denoise(c->d_ch, c->nch, da, c->d_part, c->st));
    return reduce_dev(c, Kg + (met ? 4 : 0), c->d_ch_begin, identity_map(), c->h_tot + k0);
  });
}

extern "C" int sgv_denoise(sgv_ctx* c, const double* gam1s, const double* a, double lam,
                           int nslab, const double* omegas, const double* sigmas, double rho,
                           int damp, double* der_sum) {
  ENTER(c);
  if (nslab < 1 || nslab > MAXL || !gam1s || !a || !omegas || !sigmas || !der_sum)
    return fail(c, SGV_ERR_ARG, "sgv_denoise: bad arguments (nslab=%d)", nslab);
  CHK(denoise_enqueue(c, gam1s, a, lam, nslab, omegas, sigmas, rho, damp));
  CHK(stream_wait(c));
  resolve_timers(c);
  for (int k = 0; k < c->K; ++k) der_sum[k] = c->h_tot[k];
  return SGV_OK;
}

// ---------------------------------------------------------------------------
// per-marker posterior at the denoiser's inputs (posterior.hip)
// ---------------------------------------------------------------------------
// kernel + the ordered reduction of [sum pip, sum var, count(pip >= thr)] into
// h_post; pip, lodds, var (and with resp the nslab responsibilities) are left
// in d_post rows 0, 1, 2 (3 + l), padded layout
int posterior_enqueue(sgv_ctx* c, const double* gam1s, const double* a, double lam, int nslab,
                      const double* omegas, const double* sigmas, double thr, bool resp) {
  if (!(lam >= 0.0 && lam <= 1.0))
    return fail(c, SGV_ERR_ARG, "posterior: lam must lie in [0, 1], got %g", lam);
  if (!(thr >= 0.0 && thr <= 1.0))
    return fail(c, SGV_ERR_ARG, "posterior: thr must lie in [0, 1], got %g", thr);
  CHK(grow(c, &c->d_post, &c->post_cap,
           (size_t)(POST_SUMS + (resp ? nslab : 0)) * (size_t)std::max<int64_t>(c->Mpad, 1)));
  if (!c->h_post) HIPCHK(hipHostMalloc(&c->h_post, sizeof(double) * POST_SUMS, hipHostMallocCoherent));
  PosteriorArgs pa{};
  double G = 0.0;
  for (int k = 0; k < c->K; ++k) {
    const double ag = a[k] * gam1s[k];
    G = (k == 0) ? ag : G + ag;             // the denoiser's sum_ag
  }
  pa.nslab = nslab;
  pa.thr = thr;
  pa.edge = lam == 0.0 ? -1 : lam == 1.0 ? 1 : 0;
  const double l1m = std::log1p(-lam);
  for (int l = 0; l < nslab; ++l) {
    const double q = 1.0 / (G * sigmas[l] + 1.0);
    pa.s2[l] = sigmas[l] * q;
    pa.hq[l] = -std::log1p(G * sigmas[l]) / 2;   // log(q_l) / 2
    // at an edge the odds are 0 or infinite whatever the slab: the weights
    // among the slabs (resp, var) take log(omega_l) alone
    pa.cw[l] = pa.edge ? std::log(omegas[l]) : std::log(lam * omegas[l]) - l1m;
    if (resp) pa.resp[l] = c->d_post + (size_t)(POST_SUMS + l) * c->Mpad;
  }
  pa.pip = c->d_post;
  pa.lodds = c->d_post + c->Mpad;
  pa.var = c->d_post + 2 * c->Mpad;
  if (cohort_groups(c->K) > 1) {   // more than MAXK cohorts: t over all of them first, as the denoiser
    CHK(den_inner_enqueue(c, gam1s, a, &pa.inner));
    pa.K = 1;
  } else {
    pa.K = c->K;
    for (int k = 0; k < c->K; ++k) {
      pa.r1[k] = c->r1[k];
      pa.ag[k] = a[k] * gam1s[k];
    }
  }
  HIPCHK(launch_posterior(c->d_ch, c->nch, pa, c->d_part, c->st));
  CHK(reduce_dev(c, POST_SUMS, c->d_ch_begin, identity_map(), c->h_post));
  return SGV_OK;
}

extern "C" int sgv_posterior(sgv_ctx* c, const double* gam1s, const double* a, double lam,
                             int nslab, const double* omegas, const double* sigmas, double thr,
                             double* pip, double* lodds, double* var, double* resp,
                             double* sums_out) {
  ENTER(c);
  if (nslab < 1 || nslab > MAXL || !gam1s || !a || !omegas || !sigmas || !pip || !lodds || !var ||
      !sums_out)
    return fail(c, SGV_ERR_ARG, "sgv_posterior: bad arguments (nslab=%d)", nslab);
  if (c->job_ended != c->job_begun)
    return fail(c, SGV_ERR_STATE, "sgv_posterior: a step is still queued");
  CHK(posterior_enqueue(c, gam1s, a, lam, nslab, omegas, sigmas, thr, resp != nullptr));
  CHK(download_vec(c, c->d_post, pip));
  CHK(download_vec(c, c->d_post + c->Mpad, lodds));
  CHK(download_vec(c, c->d_post + 2 * c->Mpad, var));
  for (int l = 0; resp && l < nslab; ++l)
    CHK(download_vec(c, c->d_post + (size_t)(POST_SUMS + l) * c->Mpad, resp + (size_t)l * c->Mloc));
  resolve_timers(c);
  for (int j = 0; j < POST_SUMS; ++j) sums_out[j] = c->h_post[j];   // behind download_vec's wait
  return SGV_OK;
}

// ---------------------------------------------------------------------------
// EM prior loop (src/sgvamp.py:116-136, 250-257)
// ---------------------------------------------------------------------------
extern "C" int sgv_em(sgv_ctx* c, const double* gam1s, const double* a, int nslab,
                      const double* sigmas, int maxit, double* lam_io, double* omegas_io,
                      int* steps_out, double* final_err_out) {
  ENTER(c);
  if (nslab < 1 || nslab > MAXL || !gam1s || !a || !sigmas || !lam_io || !omegas_io)
    return fail(c, SGV_ERR_ARG, "sgv_em: bad arguments");
  // more than MAXK cohorts: one k_em launch per group of MAXK, the later ones
  // adding to the first's partials (each marker's cohort sum then runs group
  // by group); np.average's weight sum covers all cohorts
  std::vector<EmArgs> eg(cohort_groups(c->K));
  EmArgs& ea = eg[0];
  double scl = 0.0;
  for (int k = 0; k < c->K; ++k) scl = (k == 0) ? a[0] : scl + a[k];
  CHK(for_cohort_groups(c->K, [&](int g, int k0, int Kg) -> int {
    EmArgs& e = eg[g];
    e = EmArgs{};
    e.K = Kg;
    e.nslab = nslab;
    for (int k = 0; k < Kg; ++k) {
      e.r1[k] = c->r1[k0 + k];
      e.a[k] = a[k0 + k];
      e.gam1[k] = gam1s[k0 + k];
    }
    e.scl = scl;
    e.accum = g > 0 ? 1 : 0;
    for (int l = 0; l < nslab; ++l) e.sigmas[l] = sigmas[l];
    e.tab = c->d_emtab + (size_t)k0 * EM_TAB;
    HIPCHK(launch_em_prep(e, c->d_emtab + (size_t)k0 * EM_TAB, c->st));
    return SGV_OK;
  }));
  auto em_groups = [&](const ChunkDesc* ch, int nch, double* part) -> int {
    for (const EmArgs& e : eg) HIPCHK(launch_em(ch, nch, e, part, c->st));
    return SGV_OK;
  };
  double lam = *lam_io;
  double om[MAXL];
  for (int l = 0; l < nslab; ++l) om[l] = omegas_io[l];
  if (c->cg_pipe && maxit > 0) {
    // Device loop: k_em reads lam/omegas from the device state, k_em_ctl updates
    // it and tests convergence; step it + 1 is enqueued before the host waits
    // for step it's test, so the GPU does not idle for a host round trip per
    // step (one no-op step runs past the last).  Every rank enqueues the same
    // steps (the stop decision is made from the same global sums).
    EmState* hi = c->h_emi;   // the previous loop's init copy has completed
    std::memset(hi, 0, sizeof(EmState));
    hi->lam = lam;
    for (int l = 0; l < nslab; ++l) hi->om[l] = om[l];
    HIPCHK(hipMemcpyAsync(c->d_ems, hi, sizeof(EmState), hipMemcpyHostToDevice, c->st));
    for (EmArgs& e : eg) e.st = c->d_ems;
    // one rank: k_em_reduce_ctl where fused_ctl_pays, else two launches (same bits).
    // With a communicator: the replicated EM (em_rep_setup) runs the same
    // one-rank loop over every rank's gathered r1.
    const bool rep = em_mode_pick(c, maxit);
    const bool fuse = rep || (!c->comm && !c->host_ag && fused_ctl_pays(EM_NV, c->nblk));
    hipEvent_t em0 = nullptr, em1 = nullptr;   // the loop on the device: its r1 gather to its last step
    CHK(event_pair(c, &em0, &em1));
    // an error return below hands the pair back to the pool (until empending holds it)
    struct PairBack {
      sgv_ctx* c;
      hipEvent_t *a, *b;
      ~PairBack() {
        if (*a) {
          c->evpool.push_back(*a);
          c->evpool.push_back(*b);
        }
      }
    } pair_back{c, &em0, &em1};
    HIPCHK(hipEventRecord(em0, c->st));
    const ChunkDesc* ech = rep ? c->d_chg : c->d_ch;
    const int* ebeg = rep ? c->d_chg_begin : c->d_ch_begin;
    const int enb = rep ? c->nblkg : c->nblk, ench = rep ? c->nchg : c->nch;
    double* epart = rep ? c->d_partg : c->d_part;
    if (rep) {
      CHK(gather_r1(c));
      for (int k = 0; k < c->K; ++k) ea.r1[k] = c->d_r1g + (size_t)k * c->mpad_max;
    }
    auto enqueue = [&](int j) -> int {
      if (fuse) {
        CHK(em_groups(ech, ench, epart));
        const EmCtl f{ebeg, enb, nslab, c->h_emm + j % CG_RING, (double)c->Mtot, j, maxit};
        HIPCHK(launch_em_reduce_ctl(epart, c->d_ems, f, c->st));
        HIPCHK(hipEventRecord(c->ev_em[j % CG_RING], c->st));
        return SGV_OK;
      }
      CHK(em_groups(c->d_ch, c->nch, c->d_part));
      CHK(reduce_dev(c, EM_NV, c->d_ch_begin, identity_map(), c->d_emtot));
      HIPCHK(launch_em_ctl(c->d_ems, c->h_emm + j % CG_RING, c->d_emtot, nslab, (double)c->Mtot,
                           j, maxit, c->st));
      HIPCHK(hipEventRecord(c->ev_em[j % CG_RING], c->st));
      return SGV_OK;
    };
    CHK(enqueue(0));
    const volatile EmState* last = nullptr;
    for (int it = 0; it < maxit; ++it) {
      if (it + 1 < maxit) CHK(enqueue(it + 1));
      CHK(event_spin(c, c->ev_em[it % CG_RING]));
      last = c->h_emm + it % CG_RING;
      if (last->done) break;
    }
    // converged: behind the one step queued past the last; maxit reached: behind its last step
    HIPCHK(hipEventRecord(em1, c->st));
    c->empending.push_back({em0, em1});
    em0 = em1 = nullptr;
    *lam_io = last->lam;
    for (int l = 0; l < nslab; ++l) omegas_io[l] = last->om[l];
    if (steps_out) *steps_out = last->steps;
    if (final_err_out) *final_err_out = last->err;
    c->em_prev_steps = last->steps;   // the same on every rank
    return SGV_OK;
  }
  double om_err = 0.0, lam_err = 0.0;
  int steps = 0;
  for (int it = 0; it < maxit; ++it) {
    for (EmArgs& e : eg) {
      e.lam = lam;
      for (int l = 0; l < nslab; ++l) e.omegas[l] = om[l];
    }
    CHK(em_groups(c->d_ch, c->nch, c->d_part));
    double tot[EM_NV];
    CHK(reduce_host(c, EM_NV, c->d_ch_begin, tot));
    const double lam_new = tot[0] / (double)c->Mtot;   // np.mean (:134)
    double om_new[MAXL];
    double dn = 0.0, on = 0.0;
    for (int l = 0; l < nslab; ++l) {
      om_new[l] = tot[1 + l] / tot[1 + nslab];         // :136
      const double d = om_new[l] - om[l];
      dn += d * d;
      on += om[l] * om[l];
    }
    om_err = std::sqrt(dn) / std::sqrt(on);            // :254
    lam_err = std::fabs(lam_new - lam) / lam_new;      // :255
    lam = lam_new;
    for (int l = 0; l < nslab; ++l) om[l] = om_new[l];
    steps = it + 1;
    if (om_err < 1e-6 && lam_err < 1e-6) break;        // :256
  }
  *lam_io = lam;
  for (int l = 0; l < nslab; ++l) omegas_io[l] = om[l];
  if (steps_out) *steps_out = steps;
  if (final_err_out) *final_err_out = std::max(om_err, lam_err);
  return SGV_OK;
}

// ---------------------------------------------------------------------------
// MLE prior update (src/sgvamp.py:139-194): the K x M x L sums of
// Lagrangian_der on the device; fsolve (MINPACK hybrd) stays on the host
// ---------------------------------------------------------------------------
// one cohort group: the Kg cohorts from k0 (for_cohort_groups)
static int mle_args(sgv_ctx* c, const double* gam1s, int L, const double* sigma2, int k0, int Kg,
                    MleArgs* m) {
  if (!gam1s || !sigma2 || L < 1 || L > MAXL + 1) return fail(c, SGV_ERR_ARG, "bad MLE arguments");
  *m = MleArgs{};
  m->K = Kg;
  m->L = L;
  for (int k = 0; k < Kg; ++k) {
    m->r1[k] = c->r1[k0 + k];
    m->ginv[k] = 1.0 / gam1s[k0 + k];                        // :146
  }
  for (int l = 0; l < L; ++l) m->sigma2[l] = sigma2[l];
  return SGV_OK;
}

extern "C" int sgv_mle_exp_max(sgv_ctx* c, const double* gam1s, int L, const double* sigma2,
                               double* exp_max) {
  ENTER(c);
  if (!exp_max) return fail(c, SGV_ERR_ARG, "exp_max is null");
  // :152: max over (k, m, l) of (-r1^2 / 2) / v_kl, attained at min_m r1_km^2
  double best = -std::numeric_limits<double>::infinity();
  CHK(for_cohort_groups(c->K, [&](int, int k0, int Kg) -> int {
    MleArgs m;
    CHK(mle_args(c, gam1s, L, sigma2, k0, Kg, &m));
    HIPCHK(launch_mle_minsq(c->d_ch, c->nch, m, c->d_part, c->st));
    double mn[MAXK];
    CHK(reduce_host(c, MAXK, c->d_ch_begin, mn, /*op=min*/ 1));
    for (int k = 0; k < m.K; ++k)
      for (int l = 0; l < L; ++l) best = std::max(best, -mn[k] / 2.0 / (m.sigma2[l] + m.ginv[k]));
    return SGV_OK;
  }));
  *exp_max = best;
  return SGV_OK;
}

extern "C" int sgv_mle_terms(sgv_ctx* c, const double* a, const double* gam1s, int L,
                             const double* sigma2, const double* omega, double exp_max,
                             double* sums) {
  ENTER(c);
  if (!a || !omega || !sums) return fail(c, SGV_ERR_ARG, "bad MLE arguments");
  // one launch per cohort group; the groups' totals are added in group order
  return for_cohort_groups(c->K, [&](int g, int k0, int Kg) -> int {
    MleArgs m;
    CHK(mle_args(c, gam1s, L, sigma2, k0, Kg, &m));
    for (int k = 0; k < Kg; ++k) m.a[k] = a[k0 + k];
    for (int l = 0; l < L; ++l) m.omega[l] = omega[l];
    m.exp_max = exp_max;
    HIPCHK(launch_mle_terms(c->d_ch, c->nch, m, c->d_part, c->st));
    double tot[MAXL + 1];
    CHK(reduce_host(c, MAXL + 1, c->d_ch_begin, tot));
    for (int l = 0; l < L; ++l) sums[l] = g == 0 ? tot[l] : sums[l] + tot[l];
    return SGV_OK;
  });
}

// The MLE prior update, src/sgvamp.py:162-194, with scipy's fsolve restated in
// hybrd.cpp; each function evaluation is one device pass over the r1 vectors
// (sgv_mle_terms), the rest the reference's host arithmetic in its order.
struct MleFn {
  sgv_ctx* c;
  const double* gam1s;
  const double* a;
  int L;
  const double* sigma2;
  const double* omega0;
  double exp_max;
  int rc;
  // the sums of the last evaluation and the omega they were taken at: the
  // Jacobian's gam column (x[L] perturbed) has the same omega, so its sums are
  // these, bitwise (the device sums are deterministic)
  double S[MAXL + 1], Sx[MAXL + 1];
  bool have_s;
};

// Lagrangian_der (:159-160) from the sums S at omega = x[:L]
static void mle_residual(const MleFn& f, const double* x, const double* S, double* y) {
  const int L = f.L;
  const double gam = x[L];
  for (int l = 0; l < L; ++l) y[l] = (S[l] + (f.omega0[l] - 1.0) / x[l]) + gam;   // :159
  double sw = 0.0;                                                                   // :160
  for (int l = 0; l < L; ++l) sw += x[l];
  y[L] = sw - 1.0;
}

static int mle_lagrangian(void* user, int n, const double* x, double* y) {
  MleFn& f = *(MleFn*)user;
  const int L = f.L;
  f.rc = sgv_mle_terms(f.c, f.a, f.gam1s, L, f.sigma2, x, f.exp_max, f.S);   // omega = x[:L]
  if (f.rc != SGV_OK) return -1;
  std::memcpy(f.Sx, x, sizeof(double) * L);
  f.have_s = true;
  mle_residual(f, x, f.S, y);
  (void)n;
  return 0;
}

// the forward-difference Jacobian's n = L + 1 points (hybrd's fdjac1): the L
// omega columns' device sums enqueued back to back with one host wait instead
// of one per point, the gam column from the base point's sums.  One cohort
// group, one rank (the host exchange waits per reduction anyway); otherwise
// point by point.  Each point's sums are the same launches as mle_lagrangian's,
// so the Jacobian is bitwise the per-point one.
static int mle_jacobian(void* user, int n, const double* x, const double* h, double* F) {
  MleFn& f = *(MleFn*)user;
  sgv_ctx* c = f.c;
  const int L = f.L;
  double xj[MAXL + 2];
  const bool base = f.have_s && std::memcmp(f.Sx, x, sizeof(double) * L) == 0;
  if (c->K > MAXK || c->comm || c->host_ag) {
    for (int j = 0; j < n; ++j) {
      std::memcpy(xj, x, sizeof(double) * n);
      xj[j] = x[j] + h[j];
      if (mle_lagrangian(user, n, xj, F + (size_t)j * n) < 0) return -1;
    }
    return 0;
  }
  f.rc = [&]() -> int {
    ENTER(c);
    MleArgs m;
    CHK(mle_args(c, f.gam1s, L, f.sigma2, 0, c->K, &m));
    for (int k = 0; k < m.K; ++k) m.a[k] = f.a[k];
    m.exp_max = f.exp_max;
    for (int j = 0; j < L; ++j) {
      for (int l = 0; l < L; ++l) m.omega[l] = l == j ? x[l] + h[l] : x[l];
      HIPCHK(launch_mle_terms(c->d_ch, c->nch, m, c->d_part, c->st));
      CHK(reduce_dev(c, MAXL + 1, c->d_ch_begin, identity_map(), c->h_tot + j * (MAXL + 1)));
    }
    CHK(stream_wait(c));
    resolve_timers(c);
    return SGV_OK;
  }();
  if (f.rc != SGV_OK) return -1;
  double base_s[MAXL + 1];
  if (base) std::memcpy(base_s, f.S, sizeof(double) * L);
  for (int j = 0; j < L; ++j) {
    std::memcpy(xj, x, sizeof(double) * n);
    xj[j] = x[j] + h[j];
    std::memcpy(f.S, c->h_tot + j * (MAXL + 1), sizeof(double) * L);
    std::memcpy(f.Sx, xj, sizeof(double) * L);
    mle_residual(f, xj, f.S, F + (size_t)j * n);
  }
  // the gam column: omega = x[:L], the base point's sums
  std::memcpy(xj, x, sizeof(double) * n);
  xj[L] = x[L] + h[L];
  if (base) {
    std::memcpy(f.S, base_s, sizeof(double) * L);
    std::memcpy(f.Sx, x, sizeof(double) * L);
    mle_residual(f, xj, f.S, F + (size_t)L * n);
    return 0;
  }
  return mle_lagrangian(user, n, xj, F + (size_t)L * n);
}

extern "C" int sgv_mle_update(sgv_ctx* c, const double* gam1s, const double* a, int nslab,
                              const double* sigmas, double* lam_io, double* omegas_io,
                              double* gam_io, int* status_out) {
  ENTER(c);
  if (!gam1s || !a || !sigmas || !lam_io || !omegas_io || !gam_io || !status_out ||
      nslab < 1 || nslab > MAXL)
    return fail(c, SGV_ERR_ARG, "sgv_mle_update: bad arguments");
  const int L = nslab + 1;
  double omega0[MAXL + 1], sigma2[MAXL + 1], x[MAXL + 2];
  omega0[0] = 1 - *lam_io;                                        // :166-168
  for (int l = 0; l < nslab; ++l) omega0[1 + l] = *lam_io * omegas_io[l];
  sigma2[0] = 1e-16;                                              // :169-171
  for (int l = 0; l < nslab; ++l) sigma2[1 + l] = sigmas[l];
  for (int l = 0; l < L; ++l) x[l] = omega0[l];                   // :173-178
  x[L] = std::isnan(*gam_io) ? 1.0 : *gam_io;
  MleFn f{c, gam1s, a, L, sigma2, omega0, 0.0, SGV_OK, {}, {}, false};
  CHK(sgv_mle_exp_max(c, gam1s, L, sigma2, &f.exp_max));           // :152, once per update
  // :179 (the forward-difference Jacobian's points batched, mle_jacobian)
  const int ier = sgv_fsolve_jac(L + 1, mle_lagrangian, mle_jacobian, &f, x, nullptr, nullptr);
  if (f.rc != SGV_OK) return f.rc;
  if (ier != 1) {                                                 // :181-184
    *status_out = SGV_MLE_NOT_CONVERGED;
    return SGV_OK;
  }
  for (int l = 0; l < L; ++l)
    if (x[l] <= 0) {                                              // :185-188
      *status_out = SGV_MLE_NEGATIVE;
      return SGV_OK;
    }
  double sw = 0.0;                                                // :190 x[:-1] /= sum(x[:-1])
  for (int l = 0; l < L; ++l) sw += x[l];
  for (int l = 0; l < L; ++l) x[l] = x[l] / sw;
  *lam_io = 1 - x[0];                                             // :191
  double ss = 0.0;                                                // :192 w / sum(x[1:-1])
  for (int l = 1; l < L; ++l) ss += x[l];
  for (int l = 0; l < nslab; ++l) omegas_io[l] = x[1 + l] / ss;
  *gam_io = x[L];                                                 // :193
  *status_out = 0;
  return SGV_OK;
}
