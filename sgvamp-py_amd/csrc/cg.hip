// The batched scipy-1.15.3 CG (iterative.py:375-422) of libsgvamp_hip.so's host
// side: one iteration in three enqueue functions, driven by the host loop
// (cg_loop: stop test, beta and rho on the host) and by the pipelined loop
// (cg_loop_dev: device-side control), and the operator seam of the tests
// (con_grad, src/sgvamp.py:7,316,332): R_s v, one pass with the whole PassArgs,
// a batched CG on (c1 R_s + c2 I).
#include "ctx.h"

// ---------------------------------------------------------------------------
// one CG iteration on columns 0..ncol-1 (CgCols, ctx.h).
// On entry: X = x0, Rr = P = r0 (= b - A x0 or b), rho[c] = r0.r0,
// atol[c] = rtol*|b|.  Columns with active[c] = 0 are skipped (bnrm2 == 0).
// Column c uses LD matrix col_ld[c] and A = c1[c] R + c2[c] I.
// The scalars come by value (host loop: beta / rho, st null) or from the device
// state (pipelined loop: st = d_cgs).
// ---------------------------------------------------------------------------
// p = r + beta p (iterative.py:403-407)
static int cg_enqueue_p(sgv_ctx* c, const CgCols& cc, unsigned mask, const double* beta,
                        const CgState* st) {
  PArgs pa{};
  pa.ncol = cc.ncol;
  pa.mask = mask;
  pa.st = st;
  for (int j = 0; j < cc.ncol; ++j) {
    pa.P[j] = cc.P[j];
    pa.Rr[j] = cc.Rr[j];
    if (beta) pa.beta[j] = beta[j];
  }
  HIPCHK(launch_cg_p(c->d_ch, c->nch, pa, c->st));
  return SGV_OK;
}

// q = A p (iterative.py:411): one pass per LD matrix over its columns of `mask`,
// each followed by reduce(ld, cols), which queues the reduction of its partial
// p.q; *npass counts the passes
template <class Reduce>
static int cg_enqueue_passes(sgv_ctx* c, const CgCols& cc, unsigned mask, const int* run,
                             int* npass, Reduce reduce) {
  for (int ld = 0; ld < c->nld; ++ld) {
    PassCols pc = gather_cols(
        cc.ncol, [&](int j) { return (mask >> j & 1u) && cc.col_ld[j] == ld; },
        [&](PassArgs& pa, int n, int j) {
          pa.in[n] = cc.P[j];
          pa.out[n] = cc.Q[j];
          pa.dot[n] = cc.P[j];
          pa.yout[n] = cc.RX[j] ? cc.Y[j] : nullptr;
          pa.c1[n] = cc.c1[j];
          pa.c2[n] = cc.c2[j];
        });
    if (!pc.nc) continue;
    pc.pa.ys1 = 1.0 - cc.s;   // Y = R_s p = (1-s) R p + s p
    pc.pa.ys0 = cc.s;
    pc.pa.run = run;
    CHK(ld_pass(c, ld, pc.nc, pc.pa));
    CHK(reduce(ld, pc));
    ++*npass;
  }
  return SGV_OK;
}

// alpha = rho / p.q; x += alpha p; r -= alpha q; the partials of r.r (:412-415)
static int cg_enqueue_xr(sgv_ctx* c, const CgCols& cc, unsigned mask, const double* pq,
                         const double* rho, const CgState* st) {
  XrArgs xa{};
  xa.ncol = cc.ncol;
  xa.mask = mask;
  xa.pq = pq;
  xa.st = st;
  for (int j = 0; j < cc.ncol; ++j) {
    xa.X[j] = cc.X[j];
    xa.Rr[j] = cc.Rr[j];
    xa.P[j] = cc.P[j];
    xa.Q[j] = cc.Q[j];
    xa.RX[j] = cc.RX[j];
    xa.Y[j] = cc.Y[j];
    if (rho) xa.rho[j] = rho[j];
  }
  HIPCHK(launch_cg_xr(c->d_ch, c->nch, xa, c->d_part, c->st));
  return SGV_OK;
}

void cg_prologue(int ncol, const double* bb, const double* rr, double rtol, double* atol,
                 double* rho, int* active) {
  for (int j = 0; j < ncol; ++j) {
    const double bn = std::sqrt(bb[j]);       // bnrm2 (iterative.py:376)
    atol[j] = std::max(0.0, rtol * bn);
    rho[j] = rr[j];
    active[j] = bn == 0.0 ? 0 : 1;            // iterative.py:380-381: return b
  }
}

static int cg_loop(sgv_ctx* c, const CgCols& cc, double* rho, const double* atol, int maxiter,
                   const int* active_in, int* iters, int* info, int* passes) {
  const int ncol = cc.ncol;
  int active[MAXC];
  double rho_prev[MAXC];
  for (int j = 0; j < ncol; ++j) {
    active[j] = active_in[j];
    rho_prev[j] = 0.0;
    if (!active[j]) {
      iters[j] = 0;
      info[j] = 0;
    }
  }
  for (int it = 0; it < maxiter; ++it) {
    unsigned mask = 0;
    for (int j = 0; j < ncol; ++j) {
      if (!active[j]) continue;
      if (std::sqrt(rho[j]) < atol[j]) {  // iterative.py:398 (strict <)
        active[j] = 0;
        iters[j] = it;
        info[j] = 0;
        continue;
      }
      mask |= 1u << j;
    }
    if (!mask) return SGV_OK;
    if (it > 0) {
      double beta[MAXC];
      for (int j = 0; j < ncol; ++j) beta[j] = (mask >> j & 1u) ? rho[j] / rho_prev[j] : 0.0;
      CHK(cg_enqueue_p(c, cc, mask, beta, nullptr));
    }
    int npass = 0;
    CHK(cg_enqueue_passes(c, cc, mask, nullptr, &npass, [&](int ld, const PassCols& pc) {
      return reduce_dev(c, pc.nc, ld_parts(c, ld), pc.map, c->d_pq);
    }));
    if (passes) *passes += npass;
    CHK(cg_enqueue_xr(c, cc, mask, c->d_pq, rho, nullptr));
    double rn[MAXC];
    CHK(reduce_host(c, MAXC, c->d_ch_begin, rn));
    for (int j = 0; j < ncol; ++j)
      if (mask >> j & 1u) {
        rho_prev[j] = rho[j];
        rho[j] = rn[j];
      }
  }
  for (int j = 0; j < ncol; ++j)
    if (active[j]) {  // for-loop exhausted (iterative.py:420-422)
      iters[j] = maxiter;
      info[j] = maxiter;
    }
  return SGV_OK;
}

int event_spin(sgv_ctx* c, hipEvent_t ev) {
  hipError_t e;
  while ((e = hipEventQuery(ev)) == hipErrorNotReady) __builtin_ia32_pause();
  if (e != hipSuccess) return fail(c, SGV_ERR_HIP, "event wait: %s", hipGetErrorString(e));
  return SGV_OK;
}

static unsigned active_mask(const volatile CgState* s, int ncol) {
  unsigned mask = 0;
  for (int j = 0; j < ncol; ++j)
    if (s->active[j]) mask |= 1u << j;
  return mask;
}

// Pipelined CG: the iteration of cg_loop with the stop test, beta and alpha on
// the device, so no host round trip sits between two iterations.  Iteration it
// is enqueued as [k_cg_ctl (stop test of `it`, beta), p update, LD pass(es) +
// p.q, x/r update + r.r]; the p/x/r kernels and the passes read the device
// state and become no-ops once no column is active.  The host then waits only
// for k_cg_ctl of `it` (the first kernel of the iteration: the wait overlaps
// the pass) and enqueues it + 1 behind it with the columns still active after
// that test -- so the column set of every pass is a function of the trajectory
// alone (deterministic; a column stopping at it + 1's test rides along in that
// pass unused).  When the test of `it` stops every column, that iteration's
// kernels were no-ops: the pass ledger is rolled back to its mark.
// Exact column sets (default, from it = 1): the p update of `it` (a no-op for
// the columns the device state has stopped) is enqueued first, then the host
// waits for the test of `it` -- it completes while that p update runs -- and
// enqueues the passes with the columns still active after it.  A CG #1 column
// that stops one iteration before its CG #2 partner then leaves the pass
// (north star: NC 8 -> 4, one pass in three once the iteration counts split;
// the same iterates bit for bit there).  Where the smaller set crosses a kernel
// boundary (NC <= 2 runs the VALU pass, 3..16 the MFMA pass) the surviving
// columns' sums are formed in another order: equal to rounding.
// With a communicator the CG prologue's sums (|b|^2, |r0|^2: the LMMSE init
// kernel's partials, `m0`) ride in the exchange of iteration 0's p.q instead of
// one of their own: the first pass runs on p0 = r0 for every column before the
// stop test of iteration 0 is known (as the look-ahead pass does), then
// k_cg_init and the test follow the shared reduction.  Same values, one
// exchange fewer per LMMSE; only where one LD matrix serves every column.
int cg_loop_dev(sgv_ctx* c, const CgCols& cc, const double* rho0, const double* atol, int maxiter,
                const int* active_in, int* iters, int* info, int* passes, const CgMerge0* m0) {
  const int ncol = cc.ncol;
  unsigned mask = 0;
  if (rho0) {
    CgState* hi = c->h_cgi;   // the previous solve's copy has completed (its mirror was read)
    std::memset(hi, 0, sizeof(CgState));
    for (int j = 0; j < ncol; ++j) {
      hi->rho[j] = rho0[j];
      hi->atol[j] = atol[j];
      hi->active[j] = active_in[j] ? 1 : 0;
      if (active_in[j]) mask |= 1u << j;
    }
    hi->any = mask ? 1 : 0;
    HIPCHK(hipMemcpyAsync(c->d_cgs, hi, sizeof(CgState), hipMemcpyHostToDevice, c->st));
  } else {
    // state set by k_cg_init on the stream; a |b| == 0 column is inactive there
    // and rides along unused in the first pass (its result is never read)
    mask = ncol >= 32 ? ~0u : (1u << ncol) - 1u;
  }
  const volatile CgState* last = nullptr;
  int executed = 0;
  // one rank: iteration it's r.r reduction and the control of it + 1 are one
  // launch (k_cg_reduce_ctl), enqueued at the end of it, when that one
  // workgroup's reduction is short: fused_ctl_pays alone decides (no switch)
  const bool fuse = !c->comm && !c->host_ag && fused_ctl_pays(MAXC, c->nblk);
  // exact sets pay only where fewer columns make a pass cheaper: the MFMA pass
  // (>= 3 columns of one LD matrix, cost by groups of 4); the VALU pass costs
  // the same at 1 and 2 columns (C2: 3.19 vs 3.21 ms), so K = 1 and distinct-LD
  // pairs keep the look-ahead and its host read stays off the critical path
  int widest = 0;
  double wide_bytes = 0.0;   // largest pass of >= 3 columns (this rank's blocks)
  for (int j = 0; j < ncol; ++j) {
    int n = 0;
    for (int i = 0; i < ncol; ++i) n += cc.col_ld[i] == cc.col_ld[j];
    widest = std::max(widest, n);
    if (n >= 3 && c->cg_exact < 0 && !c->comm && !c->host_ag) {
      CHK(ensure_plan(c, cc.col_ld[j]));
      wide_bytes = std::max(wide_bytes, c->plan[cc.col_ld[j]].stored_bytes);
    }
  }
  const bool exact = widest >= 3 && (c->cg_exact > 0 || (c->cg_exact < 0 && !c->comm &&
                                                         !c->host_ag &&
                                                         wide_bytes >= CG_EXACT_MIN_BYTES));
  for (int it = 0; it < maxiter; ++it) {
    const PassLedger::Mark mark0 = c->ledger.mark();
    int npass = 0;
    CgState* slot = c->h_cgm + (it % CG_RING);
    const bool merge = m0 && it == 0;   // the prologue's sums ride with this p.q
    if ((it == 0 || !fuse) && !merge) {
      HIPCHK(launch_cg_ctl(c->d_cgs, slot, c->d_rhonew, it, ncol, -1, c->st));
      HIPCHK(hipEventRecord(c->ev_cg[it % CG_RING], c->st));
    }
    if (it > 0) CHK(cg_enqueue_p(c, cc, mask, nullptr, c->d_cgs));
    const bool pre = exact && it > 0;   // the test of `it` read before its passes
    if (pre) {
      // the device's idle gap this read costs: p update done -> passes enqueued
      hipEvent_t g0, g1;
      CHK(event_pair(c, &g0, &g1));
      HIPCHK(hipEventRecord(g0, c->st));
      CHK(event_spin(c, c->ev_cg[it % CG_RING]));
      HIPCHK(hipEventRecord(g1, c->st));
      c->gpending.emplace_back(g0, g1);
      last = slot;
      if (!last->any) break;            // only the (no-op) p update was enqueued
      mask = active_mask(last, ncol);
    }
    const int* run = merge ? nullptr : &c->d_cgs->any;   // merge: the state is set after the pass
    CHK(cg_enqueue_passes(c, cc, mask, run, &npass, [&](int ld, const PassCols& pc) -> int {
      if (!merge) return reduce_dev(c, pc.nc, ld_parts(c, ld), pc.map, c->d_pq);
      // [|b|^2, |r0|^2] -> d_tot[0 .. 2 MAXC), p.q -> d_tot[2 MAXC + j]
      CHK(reduce_dev2(c, m0->part, 2 * MAXC, c->d_ch_begin, pc.nc, ld_parts(c, ld), pc.map,
                      2 * MAXC, c->d_tot));
      HIPCHK(launch_cg_init(c->d_cgs, c->d_tot, m0->rtol, ncol, c->d_ch, c->nch, m0->X, m0->RX,
                            c->st));
      HIPCHK(launch_cg_ctl(c->d_cgs, slot, c->d_rhonew, it, ncol, -1, c->st));
      HIPCHK(hipEventRecord(c->ev_cg[it % CG_RING], c->st));
      return SGV_OK;
    }));
    CHK(cg_enqueue_xr(c, cc, mask, merge ? c->d_tot + 2 * MAXC : c->d_pq, nullptr, c->d_cgs));
    if (fuse && it + 1 < maxiter) {
      HIPCHK(launch_cg_reduce_ctl(c->d_part, c->d_ch_begin, c->nblk, c->d_cgs,
                                  c->h_cgm + ((it + 1) % CG_RING), it + 1, ncol, c->st));
      HIPCHK(hipEventRecord(c->ev_cg[(it + 1) % CG_RING], c->st));
    } else {
      CHK(reduce_dev(c, MAXC, c->d_ch_begin, identity_map(), c->d_rhonew));
    }
    if (pre) {
      ++executed;
      if (passes) *passes += npass;
      continue;
    }
    // the stop test of `it` (its first kernel) decides whether it did any work
    CHK(event_spin(c, c->ev_cg[it % CG_RING]));
    last = slot;
    if (!last->any) {
      c->ledger.rollback(mark0, c->evpool);   // no-op passes: not timed, not counted
      break;
    }
    ++executed;
    if (passes) *passes += npass;
    mask = active_mask(last, ncol);
  }
  if (executed == maxiter) {  // for-loop exhausted (iterative.py:420-422)
    CgState* slot = c->h_cgm + (maxiter % CG_RING);
    HIPCHK(launch_cg_ctl(c->d_cgs, slot, c->d_rhonew, maxiter, ncol, maxiter, c->st));
    HIPCHK(hipEventRecord(c->ev_cg[maxiter % CG_RING], c->st));
    CHK(event_spin(c, c->ev_cg[maxiter % CG_RING]));
    last = slot;
  }
  for (int j = 0; j < ncol; ++j) {
    iters[j] = last->iters[j];
    info[j] = last->info[j];
  }
  return SGV_OK;
}

int cg_run(sgv_ctx* c, const CgCols& cc, double* rho, const double* atol, int maxiter,
           const int* active, int* iters, int* info, int* passes) {
  if (c->cg_pipe) return cg_loop_dev(c, cc, rho, atol, maxiter, active, iters, info, passes);
  return cg_loop(c, cc, rho, atol, maxiter, active, iters, info, passes);
}

// ---------------------------------------------------------------------------
// operator seam (tests): R_s v and a batched CG on (c1 R_s + c2 I)
// ---------------------------------------------------------------------------
extern "C" int sgv_ld_matvec(sgv_ctx* c, int ld, int ncol, const double* v, double* y) {
  ENTER(c);
  if (ld < 0 || ld >= c->nld || ncol < 1 || ncol > MAXC || !v || !y)
    return fail(c, SGV_ERR_ARG, "sgv_ld_matvec: bad arguments");
  PassArgs pa{};
  for (int j = 0; j < ncol; ++j) {
    CHK(upload_vec(c, v + (size_t)j * c->Mloc, c->S[j]));
    pa.in[j] = c->S[j];
    pa.out[j] = c->S[MAXC + j];
    pa.dot[j] = nullptr;
    pa.c1[j] = 1.0 - c->s;
    pa.c2[j] = c->s;
  }
  CHK(ld_pass(c, ld, ncol, pa));
  for (int j = 0; j < ncol; ++j) CHK(download_vec(c, c->S[MAXC + j], y + (size_t)j * c->Mloc));
  resolve_timers(c);
  return SGV_OK;
}

// One pass with the whole PassArgs, as the CG and gamw learning fill it: the
// columns in S[0..), out S[MAXC..), yout S[2 MAXC..), dot weights S[3 MAXC..);
// the partial dots go through ld_parts + reduce_dev into d_pq like the CG's.
extern "C" int sgv_ld_pass_ex(sgv_ctx* c, int ld, int ncol, const double* in, const double* c1,
                              const double* c2, const double* w, uint32_t dot_mask,
                              uint32_t yout_mask, double ys1, double ys0, int run, double* out,
                              double* yout, double* dots) {
  ENTER(c);
  if (ld < 0 || ld >= c->nld || ncol < 1 || ncol > MAXC || !in || !c1 || !c2 || !out ||
      run < -1 || run > 1 || (yout_mask && !yout) || (dot_mask && !dots))
    return fail(c, SGV_ERR_ARG, "sgv_ld_pass_ex: bad arguments");
  const size_t M = (size_t)c->Mloc;
  PassArgs pa{};
  for (int j = 0; j < ncol; ++j) {
    const bool dj = dot_mask >> j & 1u, yj = yout_mask >> j & 1u;
    CHK(upload_vec(c, in + j * M, c->S[j]));
    CHK(upload_vec(c, out + j * M, c->S[MAXC + j]));
    if (yj) CHK(upload_vec(c, yout + j * M, c->S[2 * MAXC + j]));
    if (dj && w) CHK(upload_vec(c, w + j * M, c->S[3 * MAXC + j]));
    pa.in[j] = c->S[j];
    pa.out[j] = c->S[MAXC + j];
    pa.yout[j] = yj ? c->S[2 * MAXC + j] : nullptr;
    pa.dot[j] = !dj ? nullptr : w ? c->S[3 * MAXC + j] : c->S[j];
    pa.c1[j] = c1[j];
    pa.c2[j] = c2[j];
  }
  pa.ys1 = ys1;
  pa.ys0 = ys0;
  if (run >= 0) {
    if (!c->d_runw) HIPCHK(hipMalloc(&c->d_runw, sizeof(int)));
    HIPCHK(hipMemcpy(c->d_runw, &run, sizeof(int), hipMemcpyHostToDevice));
    pa.run = c->d_runw;
  }
  CHK(ld_pass(c, ld, ncol, pa));
  if (dot_mask) {
    CHK(reduce_dev(c, ncol, ld_parts(c, ld), identity_map(), c->d_pq));
    HIPCHK(launch_copy_f64(c->h_tot, c->d_pq, ncol, c->st));
  }
  for (int j = 0; j < ncol; ++j) {
    CHK(download_vec(c, c->S[MAXC + j], out + j * M));
    if (yout_mask >> j & 1u) CHK(download_vec(c, c->S[2 * MAXC + j], yout + j * M));
  }
  if (dot_mask) std::memcpy(dots, c->h_tot, sizeof(double) * ncol);
  resolve_timers(c);
  return SGV_OK;
}

extern "C" int sgv_cg_solve(sgv_ctx* c, int ld, int ncol, const double* c1, const double* c2,
                            const double* b, double* x, int maxiter, double rtol, int* iters_out,
                            int* info_out) {
  ENTER(c);
  if (ld < 0 || ld >= c->nld || ncol < 1 || ncol > MAXC || !c1 || !c2 || !b || !x ||
      !iters_out || !info_out || maxiter < 0)
    return fail(c, SGV_ERR_ARG, "sgv_cg_solve: bad arguments");
  double* SB[MAXC];
  CgCols cc;
  cc.ncol = ncol;
  int warm[MAXC];
  for (int j = 0; j < ncol; ++j) {
    SB[j] = c->S[j];
    cc.X[j] = c->S[MAXC + j];
    cc.Rr[j] = c->S[2 * MAXC + j];
    cc.P[j] = c->S[3 * MAXC + j];
    cc.Q[j] = c->S[4 * MAXC + j];
    cc.col_ld[j] = ld;
    cc.c1[j] = c1[j] * (1.0 - c->s);
    cc.c2[j] = c1[j] * c->s + c2[j];
    CHK(upload_vec(c, b + (size_t)j * c->Mloc, SB[j]));
    CHK(upload_vec(c, x + (size_t)j * c->Mloc, cc.X[j]));
    warm[j] = host_any(x + (size_t)j * c->Mloc, c->Mloc);
  }
  // r = b - A x0 if x0.any() else b (iterative.py:392)
  AxpbyArgs ax{};
  for (int j = 0; j < ncol; ++j) {
    HIPCHK(hipMemcpyAsync(cc.Rr[j], SB[j], sizeof(double) * c->Mpad, hipMemcpyDeviceToDevice, c->st));
    ax.y[j] = cc.Rr[j];
    ax.x[j] = cc.Q[j];
    ax.a[j] = 1.0;
    ax.b[j] = warm[j] ? -1.0 : 0.0;
  }
  ax.ncol = ncol;
  // the pass writes Q of the warm columns, in order; the others' Q is unused (b = 0 weight)
  const PassCols w0 = gather_cols(
      ncol, [&](int j) { return warm[j] != 0; },
      [&](PassArgs& pa, int n, int j) {
        pa.in[n] = cc.X[j];
        pa.out[n] = cc.Q[j];
        pa.dot[n] = nullptr;
        pa.c1[n] = cc.c1[j];
        pa.c2[n] = cc.c2[j];
      });
  if (w0.nc) CHK(ld_pass(c, ld, w0.nc, w0.pa));
  HIPCHK(launch_axpby(c->d_ch, c->nch, ax, c->st));
  DotsArgs da{};
  da.ncol = 2 * ncol;
  for (int j = 0; j < ncol; ++j) {
    da.x[j] = SB[j];
    da.y[j] = SB[j];
    da.x[ncol + j] = cc.Rr[j];
    da.y[ncol + j] = cc.Rr[j];
    HIPCHK(hipMemcpyAsync(cc.P[j], cc.Rr[j], sizeof(double) * c->Mpad, hipMemcpyDeviceToDevice,
                          c->st));
  }
  if (2 * ncol > MAXC) return fail(c, SGV_ERR_ARG, "sgv_cg_solve: ncol <= %d", MAXC / 2);
  HIPCHK(launch_dots(c->d_ch, c->nch, da, c->d_part, c->st));
  double tot[MAXC];
  CHK(reduce_host(c, MAXC, c->d_ch_begin, tot));
  double rho[MAXC], atol[MAXC];
  int active[MAXC];
  cg_prologue(ncol, tot, tot + ncol, rtol, atol, rho, active);
  for (int j = 0; j < ncol; ++j)
    if (!active[j])   // x = b (= 0)
      HIPCHK(hipMemcpyAsync(cc.X[j], SB[j], sizeof(double) * c->Mpad, hipMemcpyDeviceToDevice, c->st));
  CHK(cg_run(c, cc, rho, atol, maxiter, active, iters_out, info_out, nullptr));
  for (int j = 0; j < ncol; ++j) CHK(download_vec(c, cc.X[j], x + (size_t)j * c->Mloc));
  return SGV_OK;
}
