// C ABI of libsgvamp_hip.so (declared in include/sgvamp_hip.h), part 1 of the
// host side: error handling, the A/B switch gate, context lifetime, host <->
// device staging (pinned copies, probe uploads), solver settings, vectors, the
// device data generator's entry points, output copies, timers.  The other
// parts: exchange.hip, ldplan.hip, cg.hip, prior.hip, solver.hip (ctx.h lists
// them).
#include "ctx.h"
#include "score.h"

static thread_local std::string g_last_err;

// A/B tuning switches: an environment override is honoured only with
// SGV_AB=1 (and then announced once on stderr); without it a set override is
// ignored with a warning, so no stray variable changes a production run.
const char* sgv::ab_env(const char* name) {
  const char* v = std::getenv(name);
  if (!v) return nullptr;
  const char* ab = std::getenv("SGV_AB");
  const bool on = ab && ab[0] == '1';
  static std::mutex mu;
  static std::vector<std::string> told;
  {
    std::lock_guard<std::mutex> lk(mu);
    if (std::find(told.begin(), told.end(), name) == told.end()) {
      told.emplace_back(name);
      std::fprintf(stderr, on ? "[sgvamp] A/B override %s=%s active (SGV_AB=1)\n"
                              : "[sgvamp] %s=%s ignored: A/B overrides need SGV_AB=1\n",
                   name, v);
    }
  }
  return on ? v : nullptr;
}

// ---------------------------------------------------------------------------
// error handling
// ---------------------------------------------------------------------------
int fail(sgv_ctx* c, int code, const char* fmt, ...){
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  g_last_err = buf;
  return code;
}

// Host wait for the ctx stream: record an event and spin on it.  The default
// hipStreamSynchronize may park the thread and wake it late (measured on
// MI355X: ~10 ms extra per wait), and the CG loop waits once per iteration.
int stream_wait(sgv_ctx* c){
  HIPCHK(hipEventRecord(c->ev_sync, c->st));
  hipError_t e;
  while ((e = hipEventQuery(c->ev_sync)) == hipErrorNotReady) {
    __builtin_ia32_pause();
  }
  if (e != hipSuccess)
    return fail(c, SGV_ERR_HIP, "stream wait: %s", hipGetErrorString(e));
  return SGV_OK;
}

// the elapsed times of a list's event pairs to add(ms, i), the events back to the pool
template <class Add>
static void resolve_pairs(sgv_ctx* c, std::vector<std::pair<hipEvent_t, hipEvent_t>>& list, Add add) {
  for (size_t i = 0; i < list.size(); ++i) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, list[i].first, list[i].second) == hipSuccess) add(ms, i);
    c->evpool.push_back(list[i].first);
    c->evpool.push_back(list[i].second);
  }
  list.clear();
}

void resolve_timers(sgv_ctx* c){
  PassLedger& led = c->ledger;
  resolve_pairs(c, led.pending, [&](float ms, size_t i) {
    led.ms += ms;
    if (led.pending_wide[i]) led.ms_wide += ms;
  });
  led.pending_wide.clear();
  resolve_pairs(c, c->xpending, [&](float ms, size_t) { c->xchg_ms += ms; });
  resolve_pairs(c, c->gpending, [&](float ms, size_t) { c->host_wait_ms += ms; });
  resolve_pairs(c, c->empending, [&](float ms, size_t) {
    c->em_ms += ms;
    c->em_loops_timed += 1.0;
  });
}

int event_pair(sgv_ctx* c, hipEvent_t* e0, hipEvent_t* e1){
  if (c->evpool.size() < 2) {
    HIPCHK(hipEventCreate(e0));
    HIPCHK(hipEventCreate(e1));
  } else {
    *e0 = c->evpool.back();
    c->evpool.pop_back();
    *e1 = c->evpool.back();
    c->evpool.pop_back();
  }
  return SGV_OK;
}

int ensure_stage(sgv_ctx* c, size_t bytes){
  if (bytes <= c->stage_bytes) return SGV_OK;
  if (c->d_stage) HIPCHK(hipFree(c->d_stage));
  c->d_stage = nullptr;
  HIPCHK(hipMalloc(&c->d_stage, bytes));
  c->stage_bytes = bytes;
  return SGV_OK;
}

int ensure_hstage(sgv_ctx* c, size_t bytes){
  if (bytes <= c->h_stage_bytes) return SGV_OK;
  if (c->h_stage) HIPCHK(hipHostFree(c->h_stage));
  c->h_stage = nullptr;
  HIPCHK(hipHostMalloc(&c->h_stage, bytes));
  c->h_stage_bytes = bytes;
  return SGV_OK;
}

// host (pageable) -> pinned -> device staging buffer; returns when the copy
// has landed (the pinned buffer may be reused right away)
static int h2d(sgv_ctx* c, const void* host, size_t bytes) {
  CHK(ensure_stage(c, std::max<size_t>(bytes, 8)));
  CHK(ensure_hstage(c, std::max<size_t>(bytes, 8)));
  std::memcpy(c->h_stage, host, bytes);
  HIPCHK(hipMemcpyAsync(c->d_stage, c->h_stage, bytes, hipMemcpyHostToDevice, c->st));
  return stream_wait(c);
}

// host half of a probe upload: the next pinned slot, once its previous copy
// has finished (long done), takes the K x Mloc probes; returns the slot or -1.
// Needs the buffers (probe_cap) in place; touches nothing a running step uses.
int probe_stage(sgv_ctx* c, const int8_t* probes){
  const int slot = c->probe_slot.fetch_xor(1);
  if (hipEventSynchronize(c->ev_probe[slot]) != hipSuccess) {
    fail(c, SGV_ERR_HIP, "probe slot wait failed");
    return -1;
  }
  std::memcpy(c->h_probe[slot], probes, (size_t)c->K * c->Mloc);
  return slot;
}
// K x Mloc int8 probes -> d_probe slot, copied on the copy stream (no host wait);
// returns the slot.  A slot's device half is consumed by the unpack kernels of
// its step (ev_unpk) and reused two uploads later.
int probe_upload(sgv_ctx* c, const int8_t* probes, int* slot_out){
  const size_t bytes = std::max<size_t>((size_t)c->K * c->Mloc, 8);
  if (bytes > c->probe_cap) {
    CHK(stream_wait(c));
    HIPCHK(hipStreamSynchronize(c->st_copy));
    for (int i = 0; i < 2; ++i) {
      if (c->h_probe[i]) HIPCHK(hipHostFree(c->h_probe[i]));
      c->h_probe[i] = nullptr;
      HIPCHK(hipHostMalloc(&c->h_probe[i], bytes));
      if (!c->ev_probe[i]) HIPCHK(hipEventCreateWithFlags(&c->ev_probe[i], hipEventDisableTiming));
      if (!c->ev_unpk[i]) HIPCHK(hipEventCreateWithFlags(&c->ev_unpk[i], hipEventDisableTiming));
    }
    if (c->d_probe) HIPCHK(hipFree(c->d_probe));
    c->d_probe = nullptr;
    HIPCHK(hipMalloc(&c->d_probe, 2 * bytes));
    c->probe_cap.store(bytes, std::memory_order_release);
  }
  const int slot = probe_stage(c, probes);
  if (slot < 0) return SGV_ERR_HIP;
  return probe_issue(c, slot, slot_out);
}

// device half of an upload staged by probe_stage: behind the slot's previous
// unpack (ev_unpk), on the copy stream
int probe_issue(sgv_ctx* c, int slot, int* slot_out){
  HIPCHK(hipStreamWaitEvent(c->st_copy, c->ev_unpk[slot], 0));
  HIPCHK(hipMemcpyAsync(c->d_probe + slot * c->probe_cap, c->h_probe[slot],
                        (size_t)c->K * c->Mloc, hipMemcpyHostToDevice, c->st_copy));
  HIPCHK(hipEventRecord(c->ev_probe[slot], c->st_copy));
  *slot_out = slot;
  return SGV_OK;
}

int upload_vec(sgv_ctx* c, const double* host, double* dpad){
  CHK(h2d(c, host, sizeof(double) * c->Mloc));
  HIPCHK(launch_unpack(c->d_ch, c->nch, c->d_ch_doff, (const double*)c->d_stage, dpad, c->st));
  return SGV_OK;
}

int download_vec(sgv_ctx* c, const double* dpad, double* host){
  const size_t bytes = sizeof(double) * std::max<int64_t>(c->Mloc, 1);
  CHK(ensure_stage(c, bytes));
  CHK(ensure_hstage(c, bytes));
  HIPCHK(launch_pack(c->d_ch, c->nch, c->d_ch_doff, dpad, (double*)c->d_stage, c->st));
  HIPCHK(hipMemcpyAsync(c->h_stage, c->d_stage, sizeof(double) * c->Mloc, hipMemcpyDeviceToHost,
                        c->st));
  CHK(stream_wait(c));
  std::memcpy(host, c->h_stage, sizeof(double) * c->Mloc);
  return SGV_OK;
}

bool host_any(const double* v, int64_t n){
  for (int64_t i = 0; i < n; ++i)
    if (v[i] != 0.0) return true;
  return false;
}

// ---------------------------------------------------------------------------
// lifetime
// ---------------------------------------------------------------------------
extern "C" int sgv_create(int device, int K, int nld, const int* ld_of, int nblk,
                          const int64_t* blk_sizes, int blk0, int nblk_global, int64_t M_total,
                          sgv_ctx** out) {
  sgv_ctx* c = nullptr;
  if (!out) return fail(nullptr, SGV_ERR_ARG, "out is null");
  *out = nullptr;
  if (K < 1 || K > MAXCOH) return fail(nullptr, SGV_ERR_ARG, "K=%d outside [1,%d]", K, MAXCOH);
  if (nld < 1 || nld > K) return fail(nullptr, SGV_ERR_ARG, "nld=%d outside [1,K]", nld);
  if (nblk < 1 || !blk_sizes) return fail(nullptr, SGV_ERR_ARG, "need >= 1 LD block");
  for (int k = 0; k < K; ++k)
    if (!ld_of || ld_of[k] < 0 || ld_of[k] >= nld)
      return fail(nullptr, SGV_ERR_ARG, "ld_of[%d] invalid", k);
  for (int b = 0; b < nblk; ++b)
    if (blk_sizes[b] < 1 || blk_sizes[b] > (int64_t)1 << 30)
      return fail(nullptr, SGV_ERR_ARG, "block %d size %lld invalid", b,
                  (long long)blk_sizes[b]);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(nullptr, SGV_ERR_HIP, "no HIP device visible");
  if (device < 0 || device >= ndev)
    return fail(nullptr, SGV_ERR_ARG, "device %d outside [0,%d)", device, ndev);

  c = new sgv_ctx();
  c->mfma_min = mfma_min_default();
  c->dev = device;
  c->K = K;
  c->nld = nld;
  c->ld_of.assign(ld_of, ld_of + K);
  c->nblk = nblk;
  c->blk0 = blk0;
  c->nblk_global = nblk_global;
  c->Mtot = M_total;
  c->Ncoh.assign(K, 1.0);
  int rc = SGV_OK;
  auto cleanup = [&](int code) {
    sgv_destroy(c);
    return code;
  };
  if (hipSetDevice(device) != hipSuccess) return cleanup(fail(nullptr, SGV_ERR_HIP, "hipSetDevice"));
  (void)hipSetDeviceFlags(hipDeviceScheduleSpin);   // best effort; waits spin anyway
  if (hipEventCreateWithFlags(&c->ev_sync, hipEventDisableTiming) != hipSuccess)
    return cleanup(fail(nullptr, SGV_ERR_HIP, "hipEventCreate"));
  if (hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking) != hipSuccess)
    return cleanup(fail(nullptr, SGV_ERR_HIP, "hipStreamCreate"));
  if (hipStreamCreateWithFlags(&c->st_copy, hipStreamNonBlocking) != hipSuccess)
    return cleanup(fail(nullptr, SGV_ERR_HIP, "hipStreamCreate"));
  if (hipStreamCreateWithFlags(&c->st_fin, hipStreamNonBlocking) != hipSuccess)
    return cleanup(fail(nullptr, SGV_ERR_HIP, "hipStreamCreate"));
  for (int g = 0; g < MAXGRP; ++g)
    if (hipEventCreateWithFlags(&c->ev_grp[g], hipEventDisableTiming) != hipSuccess)
      return cleanup(fail(nullptr, SGV_ERR_HIP, "hipEventCreate"));
  if (hipEventCreateWithFlags(&c->ev_fin, hipEventDisableTiming) != hipSuccess)
    return cleanup(fail(nullptr, SGV_ERR_HIP, "hipEventCreate"));

  // marker layout
  int64_t off = 0, voff = 0;
  for (int b = 0; b < nblk; ++b) {
    c->bn.push_back(blk_sizes[b]);
    c->boff.push_back(off);
    c->bvoff.push_back(voff);
    c->lda.push_back(round_up(blk_sizes[b], PADV));
    off += blk_sizes[b];
    voff += round_up(blk_sizes[b], PADV);
  }
  c->Mloc = off;
  c->Mpad = std::max<int64_t>(voff, PADV);

  // chunks and row groups (restart at every block start)
  std::vector<ChunkDesc> ch;
  std::vector<int64_t> chdoff;
  std::vector<int> chb(nblk + 1, 0);
  for (int b = 0; b < nblk; ++b) {
    chb[b] = (int)ch.size();
    for (int64_t o = 0; o < c->bn[b]; o += CHUNK) {
      ch.push_back(ChunkDesc{c->bvoff[b] + o, (int32_t)std::min<int64_t>(CHUNK, c->bn[b] - o), b});
      chdoff.push_back(c->boff[b] + o);
    }
  }
  chb[nblk] = (int)ch.size();
  c->nch = (int)ch.size();

#define CREATE_HIP(expr)                                                          \
  do {                                                                            \
    hipError_t e_ = (expr);                                                       \
    if (e_ != hipSuccess)                                                         \
      return cleanup(fail(nullptr, SGV_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_))); \
  } while (0)

  CREATE_HIP(hipMalloc(&c->d_ch, sizeof(ChunkDesc) * ch.size()));
  CREATE_HIP(hipMemcpy(c->d_ch, ch.data(), sizeof(ChunkDesc) * ch.size(), hipMemcpyHostToDevice));
  CREATE_HIP(hipMalloc(&c->d_ch_doff, sizeof(int64_t) * chdoff.size()));
  CREATE_HIP(hipMemcpy(c->d_ch_doff, chdoff.data(), sizeof(int64_t) * chdoff.size(),
                       hipMemcpyHostToDevice));
  CREATE_HIP(hipMalloc(&c->d_ch_begin, sizeof(int) * chb.size()));
  CREATE_HIP(hipMemcpy(c->d_ch_begin, chb.data(), sizeof(int) * chb.size(), hipMemcpyHostToDevice));

  // LD descriptors
  c->ldb.assign(nld, std::vector<LdBlock>(nblk));
  c->plan.assign(nld, LdPlan());
  c->cpl.assign(nld, std::vector<LdCoupling>());
  c->rank_blk0 = {blk0, blk0 + nblk};   // one rank until a communicator says otherwise
  for (int l = 0; l < nld; ++l) {
    BlkDesc* d = nullptr;
    CREATE_HIP(hipMalloc(&d, sizeof(BlkDesc) * nblk));
    std::vector<BlkDesc> h(nblk);
    for (int b = 0; b < nblk; ++b) h[b] = BlkDesc{nullptr, c->lda[b], c->bn[b], c->bvoff[b]};
    CREATE_HIP(hipMemcpy(d, h.data(), sizeof(BlkDesc) * nblk, hipMemcpyHostToDevice));
    c->d_blks.push_back(d);
  }

  // vectors: r, r1, r2, U (K each); xhat1, x0; X, X0, Rr, P, Q, RX0, Y, RXp (2K each);
  // S: 5 * MAXC scratch columns for the operator-seam entry points
  const int nvec = 4 * K + 2 + 16 * K + 5 * MAXC;
  const size_t vbytes = sizeof(double) * (size_t)c->Mpad * nvec;
  CREATE_HIP(hipMalloc(&c->pool, vbytes));
  CREATE_HIP(hipMemset(c->pool, 0, vbytes));
  double* p = c->pool;
  auto take = [&](std::vector<double*>& v, int n) {
    for (int i = 0; i < n; ++i) {
      v.push_back(p);
      p += c->Mpad;
    }
  };
  take(c->r, K);
  take(c->r1, K);
  take(c->r2, K);
  take(c->U, K);
  c->xhat1 = p;
  p += c->Mpad;
  c->x0 = p;
  p += c->Mpad;
  take(c->X, 2 * K);
  take(c->X0, 2 * K);
  take(c->Rr, 2 * K);
  take(c->P, 2 * K);
  take(c->Q, 2 * K);
  take(c->RX0, 2 * K);
  take(c->Y, 2 * K);
  take(c->RXp, 2 * K);
  take(c->S, 5 * MAXC);

  const size_t part_n = (size_t)c->nch * MAXNV;
  CREATE_HIP(hipMalloc(&c->d_part, sizeof(double) * part_n));
  c->part_cap = part_n;
  c->nbmax = nblk;
  CREATE_HIP(hipMalloc(&c->d_bsum, sizeof(double) * (size_t)nblk * MAXNV));
  CREATE_HIP(hipMalloc(&c->d_counts, sizeof(int)));
  CREATE_HIP(hipMemcpy(c->d_counts, &nblk, sizeof(int), hipMemcpyHostToDevice));
  CREATE_HIP(hipMalloc(&c->d_tot, sizeof(double) * 64));
  CREATE_HIP(hipMalloc(&c->d_pq, sizeof(double) * 2 * MAXC));
  // >= (MAXL + 1) * (MAXL + 1): the MLE Jacobian's batched sums (mle_jacobian)
  CREATE_HIP(hipHostMalloc(&c->h_tot, sizeof(double) * std::max(128, K), hipHostMallocCoherent));
  CREATE_HIP(hipMalloc(&c->d_cgs, sizeof(CgState)));
  CREATE_HIP(hipMalloc(&c->d_rhonew, sizeof(double) * MAXC));
  CREATE_HIP(hipHostMalloc(&c->h_cgm, sizeof(CgState) * CG_RING, hipHostMallocCoherent));
  CREATE_HIP(hipHostMalloc(&c->h_cgi, sizeof(CgState)));
  for (int i = 0; i < CG_RING; ++i)
    CREATE_HIP(hipEventCreateWithFlags(&c->ev_cg[i], hipEventDisableTiming));
  CREATE_HIP(hipEventCreateWithFlags(&c->ev_den, hipEventDisableTiming));
  CREATE_HIP(hipMalloc(&c->d_ems, sizeof(EmState)));
  CREATE_HIP(hipMalloc(&c->d_emtot, sizeof(double) * MAXNV));
  CREATE_HIP(hipMalloc(&c->d_emtab, sizeof(double) * std::max(K, MAXK) * EM_TAB));
  c->chain.gam1.assign(K, 0.0);
  c->chain.gamw.assign(K, 0.0);
  c->chain.alpha1.assign(K, 0.0);
  c->chain.alpha2.assign(K, 0.0);
  CREATE_HIP(hipHostMalloc(&c->h_emm, sizeof(EmState) * CG_RING, hipHostMallocCoherent));
  CREATE_HIP(hipHostMalloc(&c->h_emi, sizeof(EmState)));
  for (int i = 0; i < CG_RING; ++i)
    CREATE_HIP(hipEventCreateWithFlags(&c->ev_em[i], hipEventDisableTiming));
  c->cg_pipe = cg_pipe_default();
  c->cg_exact = cg_exact_default();
  c->xnz.assign(2 * K, 0);
  c->rx0_valid.assign(2 * K, 0);
#undef CREATE_HIP
  (void)rc;
  *out = c;
  return SGV_OK;
}

extern "C" void sgv_destroy(sgv_ctx* c) {
  if (!c) return;
  if (c->worker.joinable()) {
    for (auto& j : c->jobs)
      while (j.state.load() == 1 || j.state.load() == 2) __builtin_ia32_pause();
    {
      std::lock_guard<std::mutex> lk(c->wmu);
      c->worker_quit = true;
    }
    c->wcv.notify_all();
    c->worker.join();
  }
  (void)hipSetDevice(c->dev);
  if (c->st) (void)hipStreamSynchronize(c->st);
  if (c->st_fin) (void)hipStreamSynchronize(c->st_fin);
  if (c->comm) (void)ncclCommDestroy(c->comm);
  if (c->h_bsum) (void)hipHostFree(c->h_bsum);
  if (c->h_bsum_all) (void)hipHostFree(c->h_bsum_all);
  for (auto& v : c->ldb)
    for (LdBlock& lb : v) free_block(lb);
  for (LdPlan& pl : c->plan) free_plan(pl);
  for (GenoBlock& gb : c->geno) {
    if (gb.d_bits) (void)hipFree(gb.d_bits);
    if (gb.d_lut) (void)hipFree(gb.d_lut);
    if (gb.d_msd) (void)hipFree(gb.d_msd);
  }
  for (auto& v : c->cpl)
    for (LdCoupling& q : v) {
      if (q.d_up) (void)hipFree(q.d_up);
      if (q.d_lo) (void)hipFree(q.d_lo);
    }
  if (c->d_cpbuf) (void)hipFree(c->d_cpbuf);
  if (c->d_halo) (void)hipFree(c->d_halo);
  if (c->h_halo) (void)hipHostFree(c->h_halo);
  if (c->d_rowpart) (void)hipFree(c->d_rowpart);
  if (c->d_ft) (void)hipFree(c->d_ft);
  if (c->d_ftp) (void)hipFree(c->d_ftp);
  for (double* p : {c->score.d_S, c->score.d_part, c->score.d_rows, c->score.d_tab,
                    c->score.d_beta})
    if (p) (void)hipFree(p);
  for (auto& pr : c->score.pending) {
    (void)hipEventDestroy(pr.first);
    (void)hipEventDestroy(pr.second);
  }
  if (c->d_whead) (void)hipFree(c->d_whead);
  if (c->d_wcarry) (void)hipFree(c->d_wcarry);
  if (c->d_colpart) (void)hipFree(c->d_colpart);
  if (c->d_pk) (void)hipFree(c->d_pk);
  if (c->d_out) (void)hipFree(c->d_out);
  for (int i = 0; i < 2; ++i) {

    if (c->h_probe[i]) (void)hipHostFree(c->h_probe[i]);
    if (c->ev_probe[i]) (void)hipEventDestroy(c->ev_probe[i]);
  }
  if (c->d_probe) (void)hipFree(c->d_probe);
  if (c->h_met) (void)hipHostFree(c->h_met);
  if (c->ev_met) (void)hipEventDestroy(c->ev_met);
  for (BlkDesc* d : c->d_blks) (void)hipFree(d);
  (void)hipFree(c->d_ch);
  (void)hipFree(c->d_ch_doff);
  (void)hipFree(c->d_ch_begin);
  (void)hipFree(c->pool);
  (void)hipFree(c->d_part);
  if (c->d_part2) (void)hipFree(c->d_part2);
  (void)hipFree(c->d_bsum);
  if (c->d_bsum_all) (void)hipFree(c->d_bsum_all);
  (void)hipFree(c->d_counts);
  (void)hipFree(c->d_tot);
  (void)hipFree(c->d_pq);
  if (c->d_runw) (void)hipFree(c->d_runw);
  if (c->h_tot) (void)hipHostFree(c->h_tot);
  if (c->d_cgs) (void)hipFree(c->d_cgs);
  if (c->d_rhonew) (void)hipFree(c->d_rhonew);
  if (c->h_cgm) (void)hipHostFree(c->h_cgm);
  if (c->h_cgi) (void)hipHostFree(c->h_cgi);
  for (hipEvent_t e : c->ev_cg)
    if (e) (void)hipEventDestroy(e);
  if (c->d_ems) (void)hipFree(c->d_ems);
  if (c->d_chg) (void)hipFree(c->d_chg);
  if (c->d_chg_begin) (void)hipFree(c->d_chg_begin);
  if (c->d_partg) (void)hipFree(c->d_partg);
  if (c->d_r1send) (void)hipFree(c->d_r1send);
  if (c->d_r1g) (void)hipFree(c->d_r1g);
  if (c->h_r1send) (void)hipHostFree(c->h_r1send);
  if (c->h_r1g) (void)hipHostFree(c->h_r1g);
  if (c->d_emtot) (void)hipFree(c->d_emtot);
  if (c->d_emtab) (void)hipFree(c->d_emtab);
  if (c->d_inner) (void)hipFree(c->d_inner);
  if (c->d_post) (void)hipFree(c->d_post);
  if (c->h_post) (void)hipHostFree(c->h_post);
  if (c->h_emm) (void)hipHostFree(c->h_emm);
  if (c->h_emi) (void)hipHostFree(c->h_emi);
  for (hipEvent_t e : c->ev_em)
    if (e) (void)hipEventDestroy(e);
  if (c->ev_den) (void)hipEventDestroy(c->ev_den);
  if (c->d_stage) (void)hipFree(c->d_stage);
  if (c->h_stage) (void)hipHostFree(c->h_stage);
  for (auto* v : {&c->ledger.pending, &c->xpending, &c->gpending, &c->empending})
    for (auto& pr : *v) {
      (void)hipEventDestroy(pr.first);
      (void)hipEventDestroy(pr.second);
    }
  for (hipEvent_t e : c->evpool) (void)hipEventDestroy(e);
  if (c->ev_sync) (void)hipEventDestroy(c->ev_sync);
  if (c->st_copy) (void)hipStreamSynchronize(c->st_copy);
  for (int i = 0; i < 2; ++i) {
    if (c->ev_unpk[i]) (void)hipEventDestroy(c->ev_unpk[i]);

  }
  for (int i = 0; i < NOUT_SLOTS; ++i) {
    if (c->h_out[i]) (void)hipHostFree(c->h_out[i]);
    if (c->ev_out[i]) (void)hipEventDestroy(c->ev_out[i]);
    if (c->ev_pack[i]) (void)hipEventDestroy(c->ev_pack[i]);
  }
  if (c->st_fin) (void)hipStreamSynchronize(c->st_fin);
  for (hipEvent_t e : c->ev_grp)
    if (e) (void)hipEventDestroy(e);
  if (c->ev_fin) (void)hipEventDestroy(c->ev_fin);
  if (c->st_fin) (void)hipStreamDestroy(c->st_fin);
  if (c->st_copy) (void)hipStreamDestroy(c->st_copy);
  if (c->st) (void)hipStreamDestroy(c->st);
  delete c;
}

extern "C" const char* sgv_last_error(const sgv_ctx* c) {
  return c ? c->err.c_str() : g_last_err.c_str();
}

// Start a new infer() on the same context (src/sgvamp.py:198-217 resets r1,
// xhat1, xhat2, Sigma2_u_prev and the scalars every call): every solver vector
// except r, r1 and x0 is zeroed, the warm-start flags and the chained-step
// inputs are cleared.  LD blocks, ridge and cohort sizes stay.
extern "C" int sgv_reset_solver(sgv_ctx* c) {
  ENTER(c);
  if (c->job_ended != c->job_begun)
    return fail(c, SGV_ERR_STATE, "sgv_reset_solver: a step is still queued");
  const size_t n = sizeof(double) * (size_t)c->Mpad;
  for (auto* v : {&c->r2, &c->U, &c->X, &c->X0, &c->Rr, &c->P, &c->Q, &c->RX0, &c->Y, &c->RXp})
    for (double* d : *v) HIPCHK(hipMemsetAsync(d, 0, n, c->st));
  HIPCHK(hipMemsetAsync(c->xhat1, 0, n, c->st));
  CHK(stream_wait(c));
  std::fill(c->xnz.begin(), c->xnz.end(), 0);
  std::fill(c->rx0_valid.begin(), c->rx0_valid.end(), 0);
  c->chain.valid = 0;
  c->met_pending = 0;
  return SGV_OK;
}

extern "C" int sgv_set_mle_gam(sgv_ctx* c, double gam) {
  ENTER(c);
  c->mle_gam = gam;
  return SGV_OK;
}

extern "C" int sgv_set_rs_recurrence(sgv_ctx* c, int on) {
  ENTER(c);
  c->rs_rec = on ? 1 : 0;
  std::fill(c->rx0_valid.begin(), c->rx0_valid.end(), 0);   // re-derive R_s x0 once
  return SGV_OK;
}

extern "C" int sgv_set_cg_pipeline(sgv_ctx* c, int on) {
  ENTER(c);
  c->cg_pipe = on ? 1 : 0;
  return SGV_OK;
}

extern "C" int sgv_set_cg_exact(sgv_ctx* c, int mode) {
  ENTER(c);
  if (mode < -1 || mode > 1) return fail(c, SGV_ERR_ARG, "cg exact mode must be -1, 0 or 1");
  const int forced = cg_exact_default();   // an A/B override wins
  c->cg_exact = forced >= 0 ? forced : mode;
  return SGV_OK;
}

extern "C" int sgv_set_mfma_min(sgv_ctx* c, int nc_min) {
  ENTER(c);
  if (nc_min < 0) return fail(c, SGV_ERR_ARG, "nc_min must be >= 0");
  c->mfma_min = nc_min;
  return SGV_OK;
}

extern "C" int sgv_set_cohort_n(sgv_ctx* c, int k, double N) {
  ENTER(c);
  if (k < 0 || k >= c->K) return fail(c, SGV_ERR_ARG, "cohort %d", k);
  c->Ncoh[k] = N;
  return SGV_OK;
}

static double* vec_ptr(sgv_ctx* c, int which, int k) {
  const bool kok = k >= 0 && k < c->K;
  switch (which) {
    case SGV_VEC_R: return kok ? c->r[k] : nullptr;
    case SGV_VEC_R1: return kok ? c->r1[k] : nullptr;
    case SGV_VEC_XHAT1: return c->xhat1;
    case SGV_VEC_XHAT2: return kok ? c->X[2 * k] : nullptr;
    case SGV_VEC_SIG2U: return kok ? c->X[2 * k + 1] : nullptr;
    case SGV_VEC_X0: return c->x0;
    default: return nullptr;
  }
}

extern "C" int sgv_set_vector(sgv_ctx* c, int which, int k, const double* host) {
  ENTER(c);
  double* d = vec_ptr(c, which, k);
  if (!d || !host) return fail(c, SGV_ERR_ARG, "sgv_set_vector: which=%d k=%d", which, k);
  CHK(upload_vec(c, host, d));
  CHK(stream_wait(c));
  if (which == SGV_VEC_XHAT2 || which == SGV_VEC_SIG2U) {
    const int col = 2 * k + (which == SGV_VEC_SIG2U);
    c->xnz[col] = host_any(host, c->Mloc);
    c->rx0_valid[col] = 0;
    // a zeroed column is cold: no warm-start pass re-derives its R_s x, yet the
    // carried recurrence adds to RX0 (k_cg_xr) and the damping saves it
    // (k_lmmse_init), so R_s 0 = 0 is stored with it
    if (!c->xnz[col]) {
      HIPCHK(hipMemsetAsync(c->RX0[col], 0, sizeof(double) * (size_t)c->Mpad, c->st));
      CHK(stream_wait(c));
    }
  }
  return SGV_OK;
}

extern "C" int sgv_get_vector(sgv_ctx* c, int which, int k, double* host) {
  ENTER(c);
  double* d = vec_ptr(c, which, k);
  if (!d || !host) return fail(c, SGV_ERR_ARG, "sgv_get_vector: which=%d k=%d", which, k);
  return download_vec(c, d, host);
}

// ---------------------------------------------------------------------------
// synthetic inputs
// ---------------------------------------------------------------------------
struct SynthBufs {
  double *G = nullptr, *mean = nullptr, *sd = nullptr, *vec = nullptr, *g = nullptr;
  ~SynthBufs() {
    if (G) (void)hipFree(G);
    if (mean) (void)hipFree(mean);
    if (sd) (void)hipFree(sd);
    if (vec) (void)hipFree(vec);
    if (g) (void)hipFree(g);
  }
};

extern "C" int sgv_synth_ld_g(sgv_ctx* c, int ld, uint64_t seed, int64_t marker0, int Nsamp,
                              const double* beta, double* g_out) {
  ENTER(c);
  if (ld >= c->nld || Nsamp < 2 || !beta || !g_out)
    return fail(c, SGV_ERR_ARG, "sgv_synth_ld_g: bad arguments");
  const int64_t nmax = *std::max_element(c->bn.begin(), c->bn.end());
  const int ldg = (int)round_up(Nsamp, 16);
  SynthBufs sb;
  HIPCHK(hipMalloc(&sb.G, sizeof(double) * (size_t)nmax * ldg));
  HIPCHK(hipMalloc(&sb.mean, sizeof(double) * nmax));
  HIPCHK(hipMalloc(&sb.sd, sizeof(double) * nmax));
  HIPCHK(hipMalloc(&sb.vec, sizeof(double) * std::max<int64_t>(c->Mloc, 1)));
  HIPCHK(hipMalloc(&sb.g, sizeof(double) * Nsamp));
  CHK(h2d(c, beta, sizeof(double) * c->Mloc));
  HIPCHK(hipMemcpyAsync(sb.vec, c->d_stage, sizeof(double) * c->Mloc, hipMemcpyDeviceToDevice,
                        c->st));
  for (int b = 0; b < c->nblk; ++b) {
    const int n = (int)c->bn[b];
    const int64_t gm0 = marker0 + c->boff[b];
    HIPCHK(launch_geno_stats(seed, gm0, n, Nsamp, sb.mean, sb.sd, c->st));
    if (ld >= 0) {
      CHK(ld_alloc(c, ld, b, c->packing));    // R = G G^T is exactly symmetric
      const LdBlock& lb = c->ldb[ld][b];
      HIPCHK(launch_geno_G(seed, gm0, n, Nsamp, ldg, sb.mean, sb.sd, sb.G, c->st));
      HIPCHK(launch_syrk_nt(sb.G, n, Nsamp, ldg, lb.ptr, c->lda[b], lb.fmt, lb.d_poff, lb.d_pw,
                            lb.bits, c->st));
    }
    HIPCHK(launch_g_accum(seed, gm0, n, Nsamp, sb.mean, sb.sd, sb.vec + c->boff[b], sb.g, c->st));
    CHK(ensure_hstage(c, sizeof(double) * Nsamp));
    HIPCHK(hipMemcpyAsync(c->h_stage, sb.g, sizeof(double) * Nsamp, hipMemcpyDeviceToHost, c->st));
    CHK(stream_wait(c));
    std::memcpy(g_out + (size_t)b * Nsamp, c->h_stage, sizeof(double) * Nsamp);
  }
  std::fill(c->rx0_valid.begin(), c->rx0_valid.end(), 0);
  return SGV_OK;
}

extern "C" int sgv_synth_r(sgv_ctx* c, int k, uint64_t seed, int64_t marker0, int Nsamp,
                           const double* y) {
  ENTER(c);
  if (k < 0 || k >= c->K || Nsamp < 2 || !y) return fail(c, SGV_ERR_ARG, "sgv_synth_r: bad arguments");
  const int64_t nmax = *std::max_element(c->bn.begin(), c->bn.end());
  const int ldg = (int)round_up(Nsamp, 16);
  SynthBufs sb;
  HIPCHK(hipMalloc(&sb.G, sizeof(double) * (size_t)nmax * ldg));
  HIPCHK(hipMalloc(&sb.mean, sizeof(double) * nmax));
  HIPCHK(hipMalloc(&sb.sd, sizeof(double) * nmax));
  HIPCHK(hipMalloc(&sb.g, sizeof(double) * Nsamp));
  CHK(h2d(c, y, sizeof(double) * Nsamp));
  HIPCHK(hipMemcpyAsync(sb.g, c->d_stage, sizeof(double) * Nsamp, hipMemcpyDeviceToDevice, c->st));
  for (int b = 0; b < c->nblk; ++b) {
    const int n = (int)c->bn[b];
    const int64_t gm0 = marker0 + c->boff[b];
    HIPCHK(launch_geno_stats(seed, gm0, n, Nsamp, sb.mean, sb.sd, c->st));
    HIPCHK(launch_geno_G(seed, gm0, n, Nsamp, ldg, sb.mean, sb.sd, sb.G, c->st));
    HIPCHK(launch_row_dot(sb.G, n, Nsamp, ldg, sb.g, c->r[k] + c->bvoff[b], c->st));
  }
  CHK(stream_wait(c));
  return SGV_OK;
}

// ---------------------------------------------------------------------------
// genotype LD source: PLINK .bed rows -> LD blocks, r and g (geno.hip)
// ---------------------------------------------------------------------------
static void geno_free(GenoBlock& gb) {
  if (gb.d_bits) (void)hipFree(gb.d_bits);
  if (gb.d_lut) (void)hipFree(gb.d_lut);
  if (gb.d_msd) (void)hipFree(gb.d_msd);
  gb = GenoBlock();
}

extern "C" int sgv_geno_clear(sgv_ctx* c) {
  ENTER(c);
  CHK(stream_wait(c));
  for (GenoBlock& gb : c->geno) geno_free(gb);
  c->geno.clear();
  return SGV_OK;
}

// n rows of .bed codes -> gb (empty on entry): rows, tables and nbad on the device,
// the code counts in counts_out.  hs_later: the largest use of the pinned staging
// buffer that follows in the same entry, so one sizing covers it.
static int geno_stage(sgv_ctx* c, GenoBlock& gb, const uint8_t* rows, int64_t row_bytes, int nsamp,
                      int64_t n, size_t hs_later, int64_t* counts_out) {
  const int64_t used = ((int64_t)nsamp + 3) / 4;
  const int64_t stride_w = ((int64_t)nsamp + 15) / 16;
  const size_t bits_bytes = (size_t)n * stride_w * 4;
  const size_t cnt_bytes = sizeof(long long) * 4 * (size_t)n;
  HIPCHK(hipMalloc(&gb.d_bits, bits_bytes));
  HIPCHK(hipMalloc(&gb.d_lut, sizeof(double) * 4 * n));
  HIPCHK(hipMalloc(&gb.d_msd, sizeof(double) * 2 * n));
  gb.stride_w = stride_w;
  gb.nsamp = nsamp;
  // rows need not be word aligned in the file: repacked to whole words (zero
  // filled: padding the kernels mask) in the pinned staging buffer
  CHK(ensure_hstage(c, std::max(std::max(bits_bytes, cnt_bytes), hs_later)));
  CHK(ensure_stage(c, cnt_bytes));
  uint8_t* hs = static_cast<uint8_t*>(c->h_stage);
  std::memset(hs, 0, bits_bytes);
  for (int64_t i = 0; i < n; ++i)
    std::memcpy(hs + (size_t)i * stride_w * 4, rows + (size_t)i * row_bytes, (size_t)used);
  HIPCHK(hipMemcpyAsync(gb.d_bits, hs, bits_bytes, hipMemcpyHostToDevice, c->st));
  long long* d_cnt = static_cast<long long*>(c->d_stage);
  HIPCHK(launch_bed_stats(gb.d_bits, stride_w, (int)n, nsamp, d_cnt, gb.d_lut, gb.d_msd, c->st));
  CHK(stream_wait(c));   // the bits have left the staging buffer
  HIPCHK(hipMemcpyAsync(c->h_stage, d_cnt, cnt_bytes, hipMemcpyDeviceToHost, c->st));
  CHK(stream_wait(c));
  const long long* hc = static_cast<const long long*>(c->h_stage);
  gb.nbad = 0;
  for (int64_t i = 0; i < n; ++i) {
    const long long c0 = hc[4 * i], c2 = hc[4 * i + 2], c3 = hc[4 * i + 3];
    const long long nobs = c0 + c2 + c3, S1 = 2 * c0 + c2, S2 = 4 * c0 + c2;
    if (nobs == 0 || nobs * S2 - S1 * S1 == 0) ++gb.nbad;
    for (int k = 0; k < 4; ++k) counts_out[4 * i + k] = (int64_t)hc[4 * i + k];
  }
  return SGV_OK;
}

extern "C" int sgv_geno_set_block(sgv_ctx* c, int b, const uint8_t* rows, int64_t row_bytes,
                                  int nsamp, int64_t* counts_out) {
  ENTER(c);
  if (b < 0 || b >= c->nblk || !rows || !counts_out || nsamp < 1 ||
      row_bytes < ((int64_t)nsamp + 3) / 4)
    return fail(c, SGV_ERR_ARG, "sgv_geno_set_block: bad arguments (block %d, %d samples, rows of "
                "%lld bytes)", b, nsamp, (long long)row_bytes);
  if (c->geno.empty()) c->geno.resize(c->nblk);
  geno_free(c->geno[b]);
  return geno_stage(c, c->geno[b], rows, row_bytes, nsamp, c->bn[b], 0, counts_out);
}

// every owned block holds usable genotypes of nsamp samples (nsamp < 0: any, returned)
static int geno_ready(sgv_ctx* c, const char* who, int* nsamp_io) {
  if ((int)c->geno.size() != c->nblk)
    return fail(c, SGV_ERR_STATE, "%s: no genotypes set (sgv_geno_set_block)", who);
  for (int b = 0; b < c->nblk; ++b) {
    const GenoBlock& gb = c->geno[b];
    if (!gb.d_bits) return fail(c, SGV_ERR_STATE, "%s: block %d has no genotypes", who, b);
    if (gb.nbad)
      return fail(c, SGV_ERR_STATE, "%s: block %d has %lld marker(s) without LD (monomorphic or "
                  "unobserved)", who, b, (long long)gb.nbad);
    if (*nsamp_io < 0) *nsamp_io = gb.nsamp;
    if (gb.nsamp != *nsamp_io)
      return fail(c, SGV_ERR_STATE, "%s: block %d holds %d samples, not %d", who, b, gb.nsamp,
                  *nsamp_io);
  }
  return SGV_OK;
}

// block b can feed an LD build: it holds genotypes (how: where they come from) and
// every marker has LD; band: packing is on and the block is formed in one piece.
// Every refusal comes before any storage changes: the block stays as it was.
static int geno_usable(sgv_ctx* c, const char* who, int b, bool band,
                       const char* how = "sgv_geno_set_block") {
  if (band && !c->packing)
    return fail(c, SGV_ERR_STATE, "%s: a band is a packed layout and packing is off "
                "(sgv_set_ld_packing)", who);
  if ((int)c->geno.size() != c->nblk || !c->geno[b].d_bits)
    return fail(c, SGV_ERR_STATE, "%s: block %d has no genotypes (%s)", who, b, how);
  if (c->geno[b].nbad)
    return fail(c, SGV_ERR_STATE, "%s: block %d has %lld marker(s) without LD (monomorphic or "
                "unobserved)", who, b, (long long)c->geno[b].nbad);
  if (band && c->bn[b] > (int64_t)65535 * 64)
    return fail(c, SGV_ERR_ARG, "%s: block %d has %lld markers, at most %lld are formed in one "
                "piece", who, b, (long long)c->bn[b], (long long)65535 * 64);
  return SGV_OK;
}

extern "C" int sgv_geno_ld(sgv_ctx* c, int ld, int b) {
  ENTER(c);
  if (ld < 0 || ld >= c->nld || b < 0 || b >= c->nblk)
    return fail(c, SGV_ERR_ARG, "sgv_geno_ld: bad arguments (ld %d, block %d)", ld, b);
  CHK(geno_usable(c, "sgv_geno_ld", b, false));
  const GenoBlock& gb = c->geno[b];
  CHK(ld_alloc(c, ld, b, c->packing));    // R = G G^T is exactly symmetric
  const LdBlock& lb = c->ldb[ld][b];
  HIPCHK(launch_bed_syrk(gb.d_bits, gb.stride_w, gb.d_lut, (int)c->bn[b], gb.nsamp, lb.ptr,
                         c->lda[b], lb.fmt, lb.d_poff, lb.d_pw, lb.bits, c->st));
  CHK(stream_wait(c));
  std::fill(c->rx0_valid.begin(), c->rx0_valid.end(), 0);
  return SGV_OK;
}

// Block b of LD matrix ld becomes a factor block (ldplan.hip: ld_pass applies G_b
// (G_b^T p) from the rows): the staged rows and tables change owner, nothing is
// computed or copied.  Every refusal comes before any storage changes.
extern "C" int sgv_geno_ld_factor(sgv_ctx* c, int ld, int b) {
  ENTER(c);
  if (ld < 0 || ld >= c->nld || b < 0 || b >= c->nblk)
    return fail(c, SGV_ERR_ARG, "sgv_geno_ld_factor: bad arguments (ld %d, block %d)", ld, b);
  CHK(geno_usable(c, "sgv_geno_ld_factor", b, false,
                  "sgv_geno_set_block; an earlier sgv_geno_ld_factor took them over"));
  GenoBlock& gb = c->geno[b];
  for (int o = 0; o < c->nblk; ++o)
    if (c->ldb[ld][o].ptr && c->ldb[ld][o].fmt != 3)
      return fail(c, SGV_ERR_STATE, "sgv_geno_ld_factor: LD matrix %d holds a stored block "
                  "(block %d): one form per LD matrix", ld, o);
  if (!c->cpl[ld].empty())
    return fail(c, SGV_ERR_STATE, "sgv_geno_ld_factor: LD matrix %d has couplings (band pieces); "
                "a factor matrix has none", ld);
  CHK(stream_wait(c));   // no pass still reads the block this one replaces
  LdBlock& lb = c->ldb[ld][b];
  free_block(lb);
  c->plan[ld].valid = false;
  const double n = (double)c->bn[b];
  lb.fmt = 3;
  lb.bits = 64;
  lb.ptr = reinterpret_cast<double*>(gb.d_bits);
  lb.g_lut = gb.d_lut;
  lb.g_msd = gb.d_msd;
  lb.g_stride_w = gb.stride_w;
  lb.g_nsamp = gb.nsamp;
  lb.stored_bytes = n * (double)gb.stride_w * 4.0 + n * 4.0 * 8.0;
  lb.stored_elems = 2.0 * (double)gb.nsamp * n;
  gb = GenoBlock();      // the staged block is empty: its buffers are the LD block's now
  BlkDesc d{nullptr, c->lda[b], c->bn[b], c->bvoff[b]};
  HIPCHK(hipMemcpyAsync(c->d_blks[ld] + b, &d, sizeof d, hipMemcpyHostToDevice, c->st));
  CHK(stream_wait(c));
  std::fill(c->rx0_valid.begin(), c->rx0_valid.end(), 0);
  return SGV_OK;
}

// windowed R_b of band width bw: a packed band (or, where the band is as wide as
// the triangle, the packed triangle) by sgv_set_ld_block_csr's allocation rule,
// zeroed, then the kept entries from the bits by launch(lb, ext)
template <class Launch>
static int geno_band_build(sgv_ctx* c, int ld, int b, int64_t bw, Launch launch) {
  const int64_t n = c->bn[b];
  int64_t ext = round_up(SYM_H + bw, BAND_Q);
  if (ext >= n) ext = 0;   // the band is as wide as the triangle
  CHK(ld_alloc(c, ld, b, 1, ext));
  const LdBlock& lb = c->ldb[ld][b];
  // a block kept from an earlier call of the same shape may hold a wider band
  const int64_t g1 = (int64_t)lb.poff.size() - 1;
  const size_t elems = (size_t)(lb.poff[g1] + (n - g1 * SYM_H) * lb.pw[g1]);
  HIPCHK(hipMemsetAsync(lb.ptr, 0, lb.esz() * elems, c->st));
  HIPCHK(launch(lb, ext));
  CHK(stream_wait(c));
  std::fill(c->rx0_valid.begin(), c->rx0_valid.end(), 0);
  return SGV_OK;
}

extern "C" int sgv_geno_ld_band(sgv_ctx* c, int ld, int b, int64_t window) {
  ENTER(c);
  if (ld < 0 || ld >= c->nld || b < 0 || b >= c->nblk)
    return fail(c, SGV_ERR_ARG, "sgv_geno_ld_band: bad arguments (ld %d, block %d)", ld, b);
  if (window < 1)
    return fail(c, SGV_ERR_ARG, "sgv_geno_ld_band: window %lld (must be >= 1 marker)",
                (long long)window);
  CHK(geno_usable(c, "sgv_geno_ld_band", b, true));
  const GenoBlock& gb = c->geno[b];
  const int64_t n = c->bn[b], bw = std::min<int64_t>(window, n - 1);
  return geno_band_build(c, ld, b, bw, [&](const LdBlock& lb, int64_t ext) {
    return launch_bed_band(gb.d_bits, gb.stride_w, gb.d_lut, (int)n, gb.nsamp, bw, nullptr, nullptr,
                           nullptr, 0.0, ext, lb.ptr, lb.d_poff, lb.d_pw, lb.bits, c->st);
  });
}

// the halo of a coupling on the device (its rows and tables, and C), freed on every
// way out
struct HaloGuard {
  GenoBlock g;
  double* d_C = nullptr;
  ~HaloGuard() {
    geno_free(g);
    if (d_C) (void)hipFree(d_C);
  }
};

static int geno_coupling_ids(sgv_ctx* c, const char* who, int ld, int gb, int nr, int nc) {
  if (ld < 0 || ld >= c->nld || gb < 0 || gb + 1 >= c->nblk_global || nr < 1 || nc < 1)
    return fail(c, SGV_ERR_ARG, "%s: bad arguments (ld %d, gb %d, %d x %d)", who, ld, gb, nr, nc);
  return SGV_OK;
}

// coupling gb from the halo's rows (after geno_coupling_ids): a rank that owns
// neither piece only records its shape; else the rows are staged, counted and
// tabulated as a block's, C (zeroed) is formed on the device by launch(halo),
// downloaded and registered as sgv_set_ld_coupling's.  ptrs_ok: the entry's own
// pointers are given; check(): its other argument checks, after the common ones;
// hs_later: its own use of the pinned staging buffer.
template <class Check, class Launch>
static int geno_coupling_build(sgv_ctx* c, const char* who, int ld, int gb, int nr, int nc,
                               const uint8_t* rows, int64_t row_bytes, int nsamp, bool ptrs_ok,
                               size_t hs_later, int64_t* counts_out, Check check, Launch launch) {
  const int ba = gb - c->blk0, bb = gb + 1 - c->blk0;
  const bool own = (ba >= 0 && ba < c->nblk) || (bb >= 0 && bb < c->nblk);
  if (!own) return ld_set_coupling(c, who, ld, gb, nr, nc, nullptr);
  if (!rows || !counts_out || !ptrs_ok || nsamp < 1 || row_bytes < ((int64_t)nsamp + 3) / 4)
    return fail(c, SGV_ERR_ARG, "%s: bad rows (coupling %d, %d samples, rows of %lld bytes)", who,
                gb, nsamp, (long long)row_bytes);
  if ((ba >= 0 && ba < c->nblk && nr > c->bn[ba]) || (bb >= 0 && bb < c->nblk && nc > c->bn[bb]))
    return fail(c, SGV_ERR_ARG, "%s: %d x %d exceeds the pieces", who, nr, nc);
  CHK(check());
  const size_t c_bytes = sizeof(double) * (size_t)nr * nc;
  HaloGuard halo;
  HIPCHK(hipMalloc(&halo.d_C, c_bytes));
  CHK(geno_stage(c, halo.g, rows, row_bytes, nsamp, (int64_t)nr + nc, std::max(c_bytes, hs_later),
                 counts_out));
  if (halo.g.nbad)   // nothing registered: the coupling stays as it was
    return fail(c, SGV_ERR_STATE, "%s: coupling %d has %lld marker(s) without LD (monomorphic or "
                "unobserved)", who, gb, (long long)halo.g.nbad);
  HIPCHK(hipMemsetAsync(halo.d_C, 0, c_bytes, c->st));
  CHK(launch(halo));
  HIPCHK(hipMemcpyAsync(c->h_stage, halo.d_C, c_bytes, hipMemcpyDeviceToHost, c->st));
  CHK(stream_wait(c));
  return ld_set_coupling(c, who, ld, gb, nr, nc, static_cast<const double*>(c->h_stage));
}

extern "C" int sgv_geno_coupling(sgv_ctx* c, int ld, int gb, int nr, int nc, const uint8_t* rows,
                                 int64_t row_bytes, int nsamp, int64_t window,
                                 int64_t* counts_out) {
  ENTER(c);
  CHK(geno_coupling_ids(c, "sgv_geno_coupling", ld, gb, nr, nc));
  if (window < 1)
    return fail(c, SGV_ERR_ARG, "sgv_geno_coupling: window %lld (must be >= 1 marker)",
                (long long)window);
  return geno_coupling_build(
      c, "sgv_geno_coupling", ld, gb, nr, nc, rows, row_bytes, nsamp, true, 0, counts_out,
      [] { return SGV_OK; },
      [&](const HaloGuard& h) -> int {
        HIPCHK(launch_bed_corner(h.g.d_bits, h.g.stride_w, h.g.d_lut, nr, nc, nsamp, window, nullptr,
                                 0, nullptr, 0.0, c->ld_bits, h.d_C, c->st));
        return SGV_OK;
      });
}

// ---------------------------------------------------------------------------
// distance-windowed genotype LD: a reach per row, an optional triangular taper
// ---------------------------------------------------------------------------
// pos (n doubles, or NULL) and span of a taper: finite non-decreasing positions, a
// finite span > 0; nullptr when they are usable, else what is wrong
static const char* reach_pos_error(const double* pos, int64_t n, double span, int64_t* at) {
  *at = -1;
  if (!pos) return nullptr;
  if (!std::isfinite(span) || span <= 0.0) return "the span is not a finite number > 0";
  for (int64_t i = 0; i < n; ++i) {
    *at = i;
    if (!std::isfinite(pos[i])) return "a position is not finite";
    if (i && pos[i] < pos[i - 1]) return "the positions decrease";
  }
  *at = -1;
  return nullptr;
}

// reach (n int32) and, with a taper, positions (npos doubles) in one device
// allocation, through the pinned staging buffer (sized by the caller)
struct ReachAux {
  void* d = nullptr;
  const int32_t* d_reach = nullptr;
  const double* d_pos = nullptr;
  ~ReachAux() {
    if (d) (void)hipFree(d);
  }
};
static size_t reach_aux_bytes(int64_t n, int64_t npos, bool taper) {
  return (size_t)round_up(4 * n, 8) + (taper ? sizeof(double) * (size_t)npos : 0);
}
static int reach_aux_upload(sgv_ctx* c, ReachAux& x, const int32_t* reach, int64_t n,
                            const double* pos, int64_t npos) {
  const size_t o = (size_t)round_up(4 * n, 8), bytes = reach_aux_bytes(n, npos, pos != nullptr);
  HIPCHK(hipMalloc(&x.d, bytes));
  uint8_t* hs = static_cast<uint8_t*>(c->h_stage);
  std::memset(hs, 0, o);
  std::memcpy(hs, reach, sizeof(int32_t) * (size_t)n);
  if (pos) std::memcpy(hs + o, pos, sizeof(double) * (size_t)npos);
  HIPCHK(hipMemcpyAsync(x.d, hs, bytes, hipMemcpyHostToDevice, c->st));
  CHK(stream_wait(c));   // the staging buffer is free again
  x.d_reach = static_cast<const int32_t*>(x.d);
  if (pos) x.d_pos = reinterpret_cast<const double*>(static_cast<const uint8_t*>(x.d) + o);
  return SGV_OK;
}

// R_b with a reach per row: sgv_geno_ld_band's storage rule at bw = max (hi[i] - i)
extern "C" int sgv_geno_ld_band_reach(sgv_ctx* c, int ld, int b, const int32_t* hi,
                                      const double* pos, double span) {
  ENTER(c);
  if (ld < 0 || ld >= c->nld || b < 0 || b >= c->nblk || !hi)
    return fail(c, SGV_ERR_ARG, "sgv_geno_ld_band_reach: bad arguments (ld %d, block %d)", ld, b);
  const int64_t n = c->bn[b];
  int64_t bw = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (hi[i] < i || hi[i] > n - 1 || (i && hi[i] < hi[i - 1]))
      return fail(c, SGV_ERR_ARG, "sgv_geno_ld_band_reach: reach hi[%lld] = %d of block %d (must "
                  "be in [%lld, %lld] and non-decreasing)", (long long)i, (int)hi[i], b,
                  (long long)i, (long long)n - 1);
    bw = std::max<int64_t>(bw, hi[i] - i);
  }
  int64_t at;
  if (const char* why = reach_pos_error(pos, n, span, &at))
    return fail(c, SGV_ERR_ARG, "sgv_geno_ld_band_reach: block %d: %s (span %g, marker %lld)", b,
                why, span, (long long)at);
  if (pos)
    for (int64_t i = 0; i < n; ++i)
      if (pos[hi[i]] - pos[i] > span)
        return fail(c, SGV_ERR_ARG, "sgv_geno_ld_band_reach: block %d: the reach of marker %lld "
                    "(to %d) is farther than the span %g: the taper's weight would be negative", b,
                    (long long)i, (int)hi[i], span);
  CHK(geno_usable(c, "sgv_geno_ld_band_reach", b, true));
  const GenoBlock& gb = c->geno[b];
  ReachAux aux;
  CHK(ensure_hstage(c, reach_aux_bytes(n, n, pos != nullptr)));
  CHK(reach_aux_upload(c, aux, hi, n, pos, n));
  return geno_band_build(c, ld, b, bw, [&](const LdBlock& lb, int64_t ext) {
    return launch_bed_band(gb.d_bits, gb.stride_w, gb.d_lut, (int)n, gb.nsamp, 0, hi, aux.d_reach,
                           aux.d_pos, span, ext, lb.ptr, lb.d_poff, lb.d_pw, lb.bits, c->st);
  });
}

// sgv_geno_coupling with a count of kept head columns per tail row
extern "C" int sgv_geno_coupling_reach(sgv_ctx* c, int ld, int gb, int nr, int nc,
                                       const uint8_t* rows, int64_t row_bytes, int nsamp,
                                       const int32_t* keep, const double* pos, double span,
                                       int64_t* counts_out) {
  ENTER(c);
  CHK(geno_coupling_ids(c, "sgv_geno_coupling_reach", ld, gb, nr, nc));
  const int64_t n = (int64_t)nr + nc;
  int kmax = 0;
  ReachAux aux;
  return geno_coupling_build(
      c, "sgv_geno_coupling_reach", ld, gb, nr, nc, rows, row_bytes, nsamp, keep != nullptr,
      reach_aux_bytes(nr, n, pos != nullptr), counts_out,
      [&]() -> int {
        for (int a = 0; a < nr; ++a) {
          if (keep[a] < 0 || keep[a] > nc || (a && keep[a] < keep[a - 1]))
            return fail(c, SGV_ERR_ARG, "sgv_geno_coupling_reach: keep[%d] = %d of coupling %d "
                        "(must be in [0, %d] and non-decreasing)", a, (int)keep[a], gb, nc);
          kmax = std::max<int>(kmax, keep[a]);
        }
        int64_t at;
        if (const char* why = reach_pos_error(pos, n, span, &at))
          return fail(c, SGV_ERR_ARG, "sgv_geno_coupling_reach: coupling %d: %s (span %g, halo row "
                      "%lld)", gb, why, span, (long long)at);
        if (pos)
          for (int a = 0; a < nr; ++a)
            if (keep[a] > 0 && pos[nr + keep[a] - 1] - pos[a] > span)
              return fail(c, SGV_ERR_ARG, "sgv_geno_coupling_reach: coupling %d: tail row %d keeps "
                          "%d head column(s), farther than the span %g: the taper's weight would "
                          "be negative", gb, a, (int)keep[a], span);
        return SGV_OK;
      },
      [&](const HaloGuard& h) -> int {
        if (kmax == 0) return SGV_OK;   // an all-zero keep: the zero coupling
        CHK(reach_aux_upload(c, aux, keep, nr, pos, n));
        HIPCHK(launch_bed_corner(h.g.d_bits, h.g.stride_w, h.g.d_lut, nr, nc, nsamp, 0, aux.d_reach,
                                 kmax, aux.d_pos, span, c->ld_bits, h.d_C, c->st));
        return SGV_OK;
      });
}

extern "C" int sgv_geno_r(sgv_ctx* c, int k, const double* y) {
  ENTER(c);
  if (k < 0 || k >= c->K || !y) return fail(c, SGV_ERR_ARG, "sgv_geno_r: bad arguments");
  int nsamp = -1;
  CHK(geno_ready(c, "sgv_geno_r", &nsamp));
  if (c->nblk == 0) return SGV_OK;
  SynthBufs sb;
  HIPCHK(hipMalloc(&sb.g, sizeof(double) * nsamp));
  CHK(h2d(c, y, sizeof(double) * nsamp));
  HIPCHK(hipMemcpyAsync(sb.g, c->d_stage, sizeof(double) * nsamp, hipMemcpyDeviceToDevice, c->st));
  for (int b = 0; b < c->nblk; ++b) {
    const GenoBlock& gb = c->geno[b];
    HIPCHK(launch_bed_row_dot(gb.d_bits, gb.stride_w, gb.d_lut, (int)c->bn[b], nsamp, sb.g,
                              c->r[k] + c->bvoff[b], c->st));
  }
  CHK(stream_wait(c));
  return SGV_OK;
}

extern "C" int sgv_geno_g(sgv_ctx* c, const double* beta, double* g_out) {
  ENTER(c);
  if (!beta || !g_out) return fail(c, SGV_ERR_ARG, "sgv_geno_g: bad arguments");
  int nsamp = -1;
  CHK(geno_ready(c, "sgv_geno_g", &nsamp));
  if (c->nblk == 0) return SGV_OK;
  SynthBufs sb;
  HIPCHK(hipMalloc(&sb.vec, sizeof(double) * std::max<int64_t>(c->Mloc, 1)));
  HIPCHK(hipMalloc(&sb.g, sizeof(double) * nsamp));
  CHK(h2d(c, beta, sizeof(double) * c->Mloc));
  HIPCHK(hipMemcpyAsync(sb.vec, c->d_stage, sizeof(double) * c->Mloc, hipMemcpyDeviceToDevice,
                        c->st));
  CHK(ensure_hstage(c, sizeof(double) * nsamp));
  for (int b = 0; b < c->nblk; ++b) {
    const GenoBlock& gb = c->geno[b];
    HIPCHK(launch_bed_g_accum(gb.d_bits, gb.stride_w, gb.d_msd, (int)c->bn[b], nsamp,
                              sb.vec + c->boff[b], sb.g, c->st));
    HIPCHK(hipMemcpyAsync(c->h_stage, sb.g, sizeof(double) * nsamp, hipMemcpyDeviceToHost, c->st));
    CHK(stream_wait(c));
    std::memcpy(g_out + (size_t)b * nsamp, c->h_stage, sizeof(double) * nsamp);
  }
  return SGV_OK;
}

// ---------------------------------------------------------------------------
// scoring a target panel with saved effects (score.hip)
// ---------------------------------------------------------------------------
static void score_resolve(sgv_ctx* c) {
  resolve_pairs(c, c->score.pending, [&](float ms, size_t) { c->score.ms += ms; });
}

extern "C" int sgv_score_begin(sgv_ctx* c, int nsamp, int ncol) {
  ENTER(c);
  if (nsamp < 1 || ncol < 1 || ncol > SGV_SCORE_MAXCOL)
    return fail(c, SGV_ERR_ARG, "sgv_score_begin: bad arguments (%d samples, %d columns; 1..%d "
                "columns)", nsamp, ncol, SGV_SCORE_MAXCOL);
  ScoreState& s = c->score;
  const size_t need = (size_t)((ncol + SC_COLS - 1) / SC_COLS) * nsamp * SC_COLS;
  CHK(stream_wait(c));
  s.active = false;   // a stream in progress is dropped: its S may be released by grow
  CHK(grow(c, &s.d_S, &s.S_cap, need));
  HIPCHK(hipMemsetAsync(s.d_S, 0, sizeof(double) * need, c->st));
  CHK(stream_wait(c));
  s.active = true;
  s.nsamp = nsamp;
  s.ncol = ncol;
  s.seen = 0;
  return SGV_OK;
}

extern "C" int sgv_score_chunk(sgv_ctx* c, const uint8_t* rows, int64_t row_bytes, int n, int mode,
                               const double* tab, const double* beta, int64_t ldb,
                               int64_t* counts_out) {
  ENTER(c);
  ScoreState& s = c->score;
  if (!s.active)
    return fail(c, SGV_ERR_STATE, "sgv_score_chunk: no scoring stream (sgv_score_begin)");
  const int nsamp = s.nsamp, ncol = s.ncol;
  if (!rows || !beta || !counts_out || n < 1 || row_bytes < ((int64_t)nsamp + 3) / 4 ||
      (ncol > 1 && ldb < n) || mode < SGV_SCORE_TARGET || mode > SGV_SCORE_TABLE ||
      (mode == SGV_SCORE_TABLE && !tab))
    return fail(c, SGV_ERR_ARG, "sgv_score_chunk: bad arguments (%d markers, rows of %lld bytes "
                "for %d samples, mode %d, ldb %lld)", n, (long long)row_bytes, nsamp, mode,
                (long long)ldb);
  if (s.seen % SC_SLAB != 0)
    return fail(c, SGV_ERR_ARG, "sgv_score_chunk: the stream holds %lld markers, not a multiple of "
                "%d: only its last chunk may be ragged", (long long)s.seen, SC_SLAB);
  if (mode == SGV_SCORE_TABLE)
    for (int64_t k = 0; k < 4 * (int64_t)n; ++k)
      if (!std::isfinite(tab[k]))
        return fail(c, SGV_ERR_ARG, "sgv_score_chunk: tab[%lld][%d] is not finite",
                    (long long)(k / 4), (int)(k % 4));
  // everything below can fail only in the runtime
  const auto h0 = std::chrono::steady_clock::now();
  const int64_t used = ((int64_t)nsamp + 3) / 4;
  const int64_t stride_w = ((int64_t)nsamp + 15) / 16;
  const size_t bits_bytes = (size_t)n * stride_w * 4;
  const size_t cnt_bytes = sizeof(long long) * 4 * (size_t)n;
  const size_t tab_bytes = sizeof(double) * 4 * (size_t)n;
  const size_t beta_bytes = sizeof(double) * (size_t)ncol * n;
  CHK(grow(c, &s.d_rows, &s.rows_cap, (bits_bytes + 7) / 8));
  CHK(grow(c, &s.d_tab, &s.tab_cap, (size_t)14 * n));
  CHK(grow(c, &s.d_beta, &s.beta_cap, (size_t)(ncol + SC_COLS) * n));
  uint32_t* d_bits = reinterpret_cast<uint32_t*>(s.d_rows);
  double* d_tab = s.d_tab;
  double* d_lut = s.d_tab + 4 * (size_t)n;
  double* d_msd = s.d_tab + 8 * (size_t)n;
  long long* d_cnt = reinterpret_cast<long long*>(s.d_tab + 10 * (size_t)n);
  double* d_beta = s.d_beta;
  double* d_pk = s.d_beta + (size_t)ncol * n;
  CHK(ensure_hstage(c, std::max(std::max(bits_bytes, cnt_bytes), std::max(tab_bytes, beta_bytes))));
  // rows need not be word aligned at the caller: repacked to whole words
  uint8_t* hs = static_cast<uint8_t*>(c->h_stage);
  std::memset(hs, 0, bits_bytes);
  for (int64_t i = 0; i < n; ++i)
    std::memcpy(hs + (size_t)i * stride_w * 4, rows + (size_t)i * row_bytes, (size_t)used);
  HIPCHK(hipMemcpyAsync(d_bits, hs, bits_bytes, hipMemcpyHostToDevice, c->st));
  HIPCHK(launch_bed_stats(d_bits, stride_w, n, nsamp, d_cnt, d_lut, d_msd, c->st));
  CHK(stream_wait(c));   // the bits have left the staging buffer
  HIPCHK(hipMemcpyAsync(c->h_stage, d_cnt, cnt_bytes, hipMemcpyDeviceToHost, c->st));
  CHK(stream_wait(c));
  {
    const long long* hc = static_cast<const long long*>(c->h_stage);
    for (int64_t k = 0; k < 4 * (int64_t)n; ++k) counts_out[k] = (int64_t)hc[k];
  }
  if (mode == SGV_SCORE_TABLE) {
    std::memcpy(c->h_stage, tab, tab_bytes);
    HIPCHK(hipMemcpyAsync(d_tab, c->h_stage, tab_bytes, hipMemcpyHostToDevice, c->st));
    CHK(stream_wait(c));
  } else {
    HIPCHK(launch_score_tab(mode, d_cnt, d_msd, n, d_tab, c->st));
  }
  {
    double* hb = static_cast<double*>(c->h_stage);
    for (int j = 0; j < ncol; ++j)
      std::memcpy(hb + (size_t)j * n, beta + (size_t)j * ldb, sizeof(double) * n);
    HIPCHK(hipMemcpyAsync(d_beta, hb, beta_bytes, hipMemcpyHostToDevice, c->st));
    CHK(stream_wait(c));
  }
  // slabs of one launch: the partials stay under SC_PART_MAX doubles
  const int64_t nslab = ((int64_t)n + SC_SLAB - 1) / SC_SLAB;
  const int64_t per = std::max<int64_t>(
      1, std::min<int64_t>(std::min<int64_t>(nslab, 65535), SC_PART_MAX / ((int64_t)nsamp * SC_COLS)));
  CHK(grow(c, &s.d_part, &s.part_cap, (size_t)per * nsamp * SC_COLS));
  s.stage_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - h0)
                    .count();
  hipEvent_t e0, e1;
  CHK(event_pair(c, &e0, &e1));
  HIPCHK(hipEventRecord(e0, c->st));
  for (int g = 0; g * SC_COLS < ncol; ++g) {
    HIPCHK(launch_score_pack(d_beta, n, ncol, g * SC_COLS, d_pk, c->st));
    double* d_Sg = s.d_S + (size_t)g * nsamp * SC_COLS;
    for (int64_t s0 = 0; s0 < nslab; s0 += per) {
      const int ns = (int)std::min<int64_t>(per, nslab - s0);
      const int64_t m0 = s0 * SC_SLAB;
      const int nm = (int)std::min<int64_t>((int64_t)n - m0, (int64_t)ns * SC_SLAB);
      HIPCHK(launch_score_mfma(d_bits + m0 * stride_w, stride_w, d_tab + 4 * m0,
                               d_pk + SC_COLS * m0, nm, ns, nsamp, s.d_part, c->st));
      HIPCHK(launch_score_sum(s.d_part, ns, nsamp, d_Sg, c->st));
    }
  }
  HIPCHK(hipEventRecord(e1, c->st));
  s.pending.emplace_back(e0, e1);
  CHK(stream_wait(c));
  score_resolve(c);
  s.seen += n;
  s.chunks += 1.0;
  s.flops += 2.0 * (double)nsamp * (double)n * (double)ncol;
  return SGV_OK;
}

extern "C" int sgv_score_end(sgv_ctx* c, double* scores_out) {
  ENTER(c);
  ScoreState& s = c->score;
  if (!s.active)
    return fail(c, SGV_ERR_STATE, "sgv_score_end: no scoring stream (sgv_score_begin)");
  if (!scores_out) return fail(c, SGV_ERR_ARG, "sgv_score_end: null output");
  const size_t per = (size_t)s.nsamp * SC_COLS;
  CHK(ensure_hstage(c, sizeof(double) * per));
  for (int g = 0; g * SC_COLS < s.ncol; ++g) {
    HIPCHK(hipMemcpyAsync(c->h_stage, s.d_S + g * per, sizeof(double) * per, hipMemcpyDeviceToHost,
                          c->st));
    CHK(stream_wait(c));
    const double* h = static_cast<const double*>(c->h_stage);
    const int nc = std::min(SC_COLS, s.ncol - g * SC_COLS);
    for (int j = 0; j < nc; ++j) {
      double* o = scores_out + (size_t)(g * SC_COLS + j) * s.nsamp;
      for (int64_t k = 0; k < s.nsamp; ++k) o[k] = h[k * SC_COLS + j];
    }
  }
  s.active = false;
  return SGV_OK;
}

extern "C" int sgv_score_timers(sgv_ctx* c, double* t, int cap, int reset) {
  ENTER(c);
  if (!t || cap < 0) return fail(c, SGV_ERR_ARG, "sgv_score_timers: bad arguments");
  ScoreState& s = c->score;
  CHK(stream_wait(c));
  score_resolve(c);
  const double v[SGV_SCORE_TIMERS_N] = {s.ms, s.chunks, s.flops, s.stage_ms};
  for (int i = 0; i < std::min(cap, SGV_SCORE_TIMERS_N); ++i) t[i] = v[i];
  if (reset) s.ms = s.chunks = s.flops = s.stage_ms = 0.0;
  return SGV_OK;
}

// ---------------------------------------------------------------------------
// per-iteration outputs without a host wait (src/sgvamp.py:281,283)
// ---------------------------------------------------------------------------
// post: the slot also takes pip, lodds, var (rows K + 1 .. K + 3) from d_post,
// where the step's posterior kernel left them (SGV_STEP_POSTERIOR)
int outputs_begin(sgv_ctx* c, int slot, bool post) {
  if (slot < 0 || slot >= NOUT_SLOTS) return fail(c, SGV_ERR_ARG, "slot must be 0, 1 or 2");
  if (post && (!c->post_on || !c->d_post))
    return fail(c, SGV_ERR_STATE, "posterior rows without sgv_set_posterior_outputs");
  const size_t n = (size_t)std::max<int64_t>(c->Mloc, 1);
  if (!c->d_out) {   // a device staging half and a pinned buffer per slot
    c->out_rows = c->K + 1 + (c->post_on ? POST_SUMS : 0);
    const size_t bytes = sizeof(double) * n * c->out_rows;
    HIPCHK(hipMalloc(&c->d_out, NOUT_SLOTS * bytes));
    for (int i = 0; i < NOUT_SLOTS; ++i) {
      HIPCHK(hipHostMalloc(&c->h_out[i], bytes));
      if (c->ev_out[i]) continue;   // kept when the buffers were resized
      HIPCHK(hipEventCreateWithFlags(&c->ev_out[i], hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&c->ev_pack[i], hipEventDisableTiming));
    }
  }
  const int rows = c->K + 1 + (post ? POST_SUMS : 0);
  double* dst = c->d_out + (size_t)slot * n * c->out_rows;
  HIPCHK(hipStreamWaitEvent(c->st, c->ev_out[slot], 0));   // the slot's previous copy
  HIPCHK(launch_pack(c->d_ch, c->nch, c->d_ch_doff, c->xhat1, dst, c->st));
  for (int k = 0; k < c->K; ++k)
    HIPCHK(launch_pack(c->d_ch, c->nch, c->d_ch_doff, c->r1[k], dst + n * (k + 1), c->st));
  for (int j = 0; post && j < POST_SUMS; ++j)
    HIPCHK(launch_pack(c->d_ch, c->nch, c->d_ch_doff, c->d_post + (size_t)j * c->Mpad,
                       dst + n * (c->K + 1 + j), c->st));
  // the copy runs on the copy stream: the ctx stream goes on with the step
  HIPCHK(hipEventRecord(c->ev_pack[slot], c->st));
  HIPCHK(hipStreamWaitEvent(c->st_copy, c->ev_pack[slot], 0));
  HIPCHK(hipMemcpyAsync(c->h_out[slot], dst, sizeof(double) * n * rows, hipMemcpyDeviceToHost,
                        c->st_copy));
  HIPCHK(hipEventRecord(c->ev_out[slot], c->st_copy));
  return SGV_OK;
}

extern "C" int sgv_outputs_begin(sgv_ctx* c, int slot) {
  ENTER(c);
  return outputs_begin(c, slot, false);
}

extern "C" int sgv_set_posterior_outputs(sgv_ctx* c, int on, double thr) {
  ENTER(c);
  if (!(thr >= 0.0 && thr <= 1.0))
    return fail(c, SGV_ERR_ARG, "sgv_set_posterior_outputs: thr must lie in [0, 1], got %g", thr);
  if (c->job_ended != c->job_begun)
    return fail(c, SGV_ERR_STATE, "sgv_set_posterior_outputs: a step is still queued");
  c->post_on = on ? 1 : 0;
  c->post_thr = thr;
  if (c->d_out && c->out_rows != c->K + 1 + (c->post_on ? POST_SUMS : 0)) {
    // slots of the other layout: dropped once their copies have landed, made
    // again by the next sgv_outputs_begin
    CHK(stream_wait(c));
    HIPCHK(hipStreamSynchronize(c->st_copy));
    HIPCHK(hipFree(c->d_out));
    c->d_out = nullptr;
    for (int i = 0; i < NOUT_SLOTS; ++i) {
      HIPCHK(hipHostFree(c->h_out[i]));
      c->h_out[i] = nullptr;
    }
  }
  return SGV_OK;
}

// May be called from another host thread than the one driving the context: it
// only waits on the slot's event and returns the pinned buffer (valid until the
// slot's next sgv_outputs_begin).
extern "C" int sgv_outputs_wait(sgv_ctx* c, int slot, double** data) {
  if (!c || slot < 0 || slot >= NOUT_SLOTS || !data || !c->ev_out[slot] || !c->h_out[slot])
    return SGV_ERR_ARG;
  if (hipSetDevice(c->dev) != hipSuccess) return SGV_ERR_HIP;
  hipError_t e;
  while ((e = hipEventQuery(c->ev_out[slot])) == hipErrorNotReady) __builtin_ia32_pause();
  if (e != hipSuccess) return SGV_ERR_HIP;
  *data = c->h_out[slot];
  return SGV_OK;
}

extern "C" int sgv_abi_version(void) { return SGV_ABI_VERSION; }

extern "C" int sgv_timers(sgv_ctx* c, double* dst, int cap, int reset) {
  ENTER(c);
  if (cap < 0 || (cap > 0 && !dst)) return fail(c, SGV_ERR_ARG, "sgv_timers: bad buffer");
  CHK(stream_wait(c));
  resolve_timers(c);
  const PassLedger& led = c->ledger;
  const double t[SGV_TIMERS_N] = {led.ms,          led.n.launches,  led.n.bytes, led.n.rhs_bytes,
                                  led.n.dense_bytes, led.n.aux_bytes, led.n.flops, led.n.flops_wide,
                                  led.ms_wide,     led.n.launches_wide};
  for (int i = 0; i < std::min(cap, SGV_TIMERS_N); ++i) dst[i] = t[i];
  if (reset) c->ledger.clear_counts();
  return SGV_OK;
}

extern "C" int sgv_sync(sgv_ctx* c) {
  ENTER(c);
  CHK(stream_wait(c));
  resolve_timers(c);
  return SGV_OK;
}

extern "C" int sgv_read_bw(sgv_ctx* c, int64_t bytes, int reps, double* gbps) {
  ENTER(c);
  const int64_t unit = (int64_t)256 * 1024;
  bytes = bytes / unit * unit;
  if (!gbps || bytes < unit || reps < 1) return fail(c, SGV_ERR_ARG, "sgv_read_bw: bad arguments");
  CHK(stream_wait(c));
  double* buf = nullptr;
  double* out = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = SGV_OK;
  if (hipMalloc(&buf, (size_t)bytes) != hipSuccess || hipMalloc(&out, 256 * sizeof(double)) != hipSuccess ||
      hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)
    rc = fail(c, SGV_ERR_HIP, "sgv_read_bw: allocation of %.2f GB failed", bytes / 1e9);
  if (rc == SGV_OK && hipMemsetAsync(buf, 0, (size_t)bytes, c->st) != hipSuccess)
    rc = fail(c, SGV_ERR_HIP, "sgv_read_bw: memset failed");
  float best = 0.f;
  for (int r = -1; rc == SGV_OK && r < reps; ++r) {   // r = -1: warm-up
    float ms = 0.f;
    if (hipEventRecord(e0, c->st) != hipSuccess ||
        launch_read_probe(buf, (size_t)bytes, out, c->st) != hipSuccess ||
        hipEventRecord(e1, c->st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
        hipEventElapsedTime(&ms, e0, e1) != hipSuccess)
      rc = fail(c, SGV_ERR_HIP, "sgv_read_bw: probe launch failed");
    else if (r >= 0 && (best == 0.f || ms < best))
      best = ms;
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (buf) (void)hipFree(buf);
  if (out) (void)hipFree(out);
  if (rc != SGV_OK) {
    (void)hipGetLastError();   // clear it: the next launch_* would report this failure
    return rc;
  }
  *gbps = (double)bytes / ((double)best * 1e-3) / 1e9;
  return SGV_OK;
}
