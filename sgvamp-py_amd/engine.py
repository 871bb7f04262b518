"""Shard-aware wrapper over one sgv_ctx: this rank's LD blocks, all cohorts.

An Engine owns the rank-local slice [marker0, marker0 + Mloc) of every
marker-length vector; every M-length reduction inside the library is ordered
by global LD block, so the scalars it returns are identical on every rank and
for any number of ranks.
"""
import ctypes
import os

import numpy as np

import hip_backend as hb
from partition import marker_offsets, partition_blocks

CG_EXACT_MIN_BYTES = 24e9   # capi.hip: exact CG column sets from passes of this size
SYM_H = 256                 # rows per packed panel (common.h)


def cg_exact_mode(block_sizes):
    """The run's CG column-set mode (sgv_set_cg_exact) from the GLOBAL LD: exact
    sets when a pass streams >= 24 GB of packed triangle, else look-ahead.  A
    function of the global block sizes only, so every rank of a run and every
    rank count make the same choice (the modes can round differently).  The
    estimate before any LD is stored; Engine.update_cg_exact refines it from the
    bytes actually stored (band blocks store far less than the triangle)."""
    tri = sum(float(n) * (n + SYM_H) / 2.0 * 8.0 for n in block_sizes)
    return 1 if tri >= CG_EXACT_MIN_BYTES else 0


def cg_exact_from_stored(global_bytes_per_ld, ld_of):
    """The same choice from the global stored bytes of each LD matrix: exact when
    a matrix shared by >= 2 cohorts (>= 4 CG columns: the MFMA pass, where a
    narrower column set is cheaper) streams >= 24 GB per pass."""
    shared = [l for l in set(ld_of) if list(ld_of).count(l) >= 2]
    big = max((global_bytes_per_ld[l] for l in shared), default=0.0)
    return 1 if big >= CG_EXACT_MIN_BYTES else 0


class Engine:
    def __init__(self, block_sizes, K, ld_of=None, comm=None, device=None, exchange=None):
        """block_sizes: global LD block sizes (marker order).  ld_of[k]: index of
        the LD matrix cohort k uses (cohorts sharing an LD share LD passes).
        exchange: "rccl" (default) or "host" (the communicator's allgather_f64
        carries the per-block partials; env SGV_EXCHANGE overrides the default).
        With one rank no communicator is made unless `exchange` is passed
        explicitly (a one-rank RCCL/host exchange: same results, used to rehearse
        the exchange on one GPU)."""
        from comm import SingleComm

        self.comm = comm or SingleComm()
        self.rank = self.comm.Get_rank()
        self.nranks = self.comm.Get_size()
        self.block_sizes = [int(b) for b in block_sizes]
        self.K = int(K)
        self.ld_of = list(ld_of) if ld_of is not None else [0] * self.K
        if len(self.ld_of) != self.K:
            raise ValueError("ld_of must have K entries")
        # canonical LD ids 0..nld-1 in order of first use
        remap = {}
        for l in self.ld_of:
            remap.setdefault(l, len(remap))
        self.ld_of = [remap[l] for l in self.ld_of]
        self.nld = len(remap)
        self.ranges = partition_blocks(self.block_sizes, self.nranks)
        self.b0, self.b1 = self.ranges[self.rank]
        offs = marker_offsets(self.block_sizes)
        self.M = int(offs[-1])
        self.marker0 = int(offs[self.b0])
        self.Mloc = int(offs[self.b1] - offs[self.b0])
        self.local_sizes = self.block_sizes[self.b0:self.b1]
        self.sl = slice(self.marker0, self.marker0 + self.Mloc)
        if device is None:   # one process per GPU: the node-local rank (comm.launch_from_env)
            device = int(getattr(self.comm, "local_rank", 0)) if self.nranks > 1 else 0
        self.ctx = hb.Context(device, self.K, self.ld_of, self.local_sizes, self.b0,
                              len(self.block_sizes), self.M)
        self.posterior_rows = 0     # rows behind xhat1, r1 in the output slots (set_posterior_outputs)
        self.cg_exact = cg_exact_mode(self.block_sizes)
        self.ctx.sgv_set_cg_exact(self.cg_exact)    # an SGV_CG_EXACT A/B override wins
        self.exchange = exchange or os.environ.get("SGV_EXCHANGE", "rccl")
        if self.exchange not in ("rccl", "host"):
            raise ValueError("exchange must be 'rccl' or 'host', got %r" % self.exchange)
        self._ag_cb = None
        if self.nranks > 1 or exchange is not None:
            counts = np.array([r1 - r0 for r0, r1 in self.ranges], dtype=np.int32)
            if self.exchange == "host":
                self._ag_cb = hb.make_allgather(self.comm, self.nranks)
                self.ctx.sgv_comm_init_host(self.nranks, self.rank, hb.iptr(counts),
                                            ctypes.cast(self._ag_cb, ctypes.c_void_p), None)
            else:
                uid = hb.unique_id() if self.rank == 0 else None
                uid = self.comm.bcast(uid, root=0)
                self.ctx.sgv_comm_init(self.nranks, self.rank, uid, hb.iptr(counts))
            # this job's all-gather latency, the EM loop's cost-model parameter.
            # The probe is collective, so the decision must be the same on every
            # rank: the library took rank 0's SGV_XCHG_LAT_US (if any) at
            # communicator set-up, and its latency source -- rank 0's, identical
            # on every rank -- says whether to probe ("default": rank 0 set no
            # value) or keep rank 0's setting.  A rank's own environment decides
            # nothing here.
            if self.exchange_stats()["latency_source"] == "default":
                self.exchange_probe(10)

    # ---- inputs ----------------------------------------------------------
    def set_ld_block(self, ld, b_global, block):
        """Upload LD block b_global of LD matrix `ld` if this rank owns it."""
        if not (self.b0 <= b_global < self.b1):
            return
        B = np.ascontiguousarray(block, dtype=np.float64)
        n = self.block_sizes[b_global]
        if B.shape != (n, n):
            raise ValueError("LD block %d has shape %s, expected (%d, %d)" % (b_global, B.shape, n, n))
        self.ctx.sgv_set_ld_block(ld, b_global - self.b0, hb.dptr(B), n)

    def set_ld_block_csr(self, ld, b_global, upper):
        """Upload LD block b_global from the scipy CSR of its upper triangle
        (block-relative, diagonal included) if this rank owns it; stored as a
        packed band when the entries stay near the diagonal (sgv_set_ld_block_csr)."""
        if not (self.b0 <= b_global < self.b1):
            return
        n = self.block_sizes[b_global]
        if upper.shape != (n, n):
            raise ValueError("LD block %d has shape %s, expected (%d, %d)" % (b_global, upper.shape, n, n))
        indptr = np.ascontiguousarray(upper.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(upper.indices, dtype=np.int64)
        data = np.ascontiguousarray(upper.data, dtype=np.float64)
        self.ctx.sgv_set_ld_block_csr(ld, b_global - self.b0, indptr.ctypes.data_as(hb._c_i64_p),
                                      indices.ctypes.data_as(hb._c_i64_p), hb.dptr(data))

    def set_ld_coupling(self, ld, gb, nr, nc, C):
        """Coupling between band pieces gb and gb + 1 (global indices) of LD matrix
        ld: C = R[last nr rows of gb][first nc columns of gb + 1] (dense or
        scipy sparse).  Called on every rank for every coupling; the matrix is
        densified and sent only where this rank owns one of the two pieces."""
        own = self.b0 <= gb < self.b1 or self.b0 <= gb + 1 < self.b1
        ptr = None
        if own:
            D = C.toarray() if hasattr(C, "toarray") else np.asarray(C)
            D = np.ascontiguousarray(D, dtype=np.float64)
            if D.shape != (nr, nc):
                raise ValueError("coupling %d has shape %s, expected (%d, %d)" % (gb, D.shape, nr, nc))
            ptr = hb.dptr(D)
        self.ctx.sgv_set_ld_coupling(int(ld), int(gb), int(nr), int(nc), ptr)

    def stored_bytes(self, ld):
        """Bytes one pass over LD matrix ld reads on this rank (blocks set so far)."""
        out = np.zeros(1)
        self.ctx.sgv_ld_stored_bytes(int(ld), hb.dptr(out))
        return float(out[0])

    def update_cg_exact(self):
        """Once every rank's LD blocks are stored: the run's CG column-set mode
        from the GLOBAL stored bytes (summed over ranks in rank order, so every
        rank makes the same choice for any rank count).  Collective."""
        local = np.array([self.stored_bytes(l) for l in range(self.nld)], dtype=np.float64)
        if self.nranks > 1:
            parts = self.comm.allgather(local)
            tot = np.zeros(self.nld)
            for p in parts:
                tot = tot + np.asarray(p, dtype=np.float64)
        else:
            tot = local
        self.cg_exact = cg_exact_from_stored(list(tot), self.ld_of)
        self.ctx.sgv_set_cg_exact(self.cg_exact)    # an SGV_CG_EXACT A/B override wins
        return self.cg_exact

    def get_ld_block(self, ld, b_global):
        n = self.block_sizes[b_global]
        out = np.empty((n, n), dtype=np.float64)
        self.ctx.sgv_get_ld_block(ld, b_global - self.b0, hb.dptr(out), n)
        return out

    def set_mfma_min(self, nc_min):
        """Packed LD passes with >= nc_min right-hand sides use the f64 MFMA kernel."""
        self.ctx.sgv_set_mfma_min(int(nc_min))

    def set_cg_pipeline(self, on):
        """Device-side CG control with the next iteration enqueued ahead (default)
        or the host-side stop test per iteration."""
        self.ctx.sgv_set_cg_pipeline(1 if on else 0)

    def set_rs_recurrence(self, on):
        """Carry R_s x through the CG (default) instead of a gamw LD pass."""
        self.ctx.sgv_set_rs_recurrence(1 if on else 0)

    def reset_solver(self):
        """Zero the solver state for a new infer() (src/sgvamp.py:198-217)."""
        self.ctx.sgv_reset_solver()

    def set_ridge(self, s):
        self.ctx.sgv_set_ridge(float(s))

    def set_cohort_n(self, k, N):
        self.ctx.sgv_set_cohort_n(k, float(N))

    def set_vector(self, which, k, full_or_local):
        v = np.asarray(full_or_local, dtype=np.float64).ravel()
        if v.shape[0] == self.M and self.M != self.Mloc:
            v = v[self.sl]
        v = np.ascontiguousarray(v)
        if v.shape[0] != self.Mloc:
            raise ValueError("vector length %d != local M %d" % (v.shape[0], self.Mloc))
        self.ctx.sgv_set_vector(which, k, hb.dptr(v))

    def get_vector(self, which, k=0):
        out = np.empty(self.Mloc, dtype=np.float64)
        self.ctx.sgv_get_vector(which, k, hb.dptr(out))
        return out

    # ---- synthetic inputs (device generator) -------------------------------
    def synth_ld_g(self, ld, geno_seed, nsamp, beta_full):
        beta = np.ascontiguousarray(np.asarray(beta_full, dtype=np.float64)[self.sl])
        g = np.empty((len(self.local_sizes), nsamp), dtype=np.float64)
        self.ctx.sgv_synth_ld_g(int(ld), int(geno_seed), self.marker0, int(nsamp), hb.dptr(beta),
                                hb.dptr(g))
        return g

    def synth_r(self, k, geno_seed, nsamp, y):
        y = np.ascontiguousarray(y, dtype=np.float64)
        self.ctx.sgv_synth_r(int(k), int(geno_seed), self.marker0, int(nsamp), hb.dptr(y))

    # ---- genotype LD source (PLINK .bed rows, device) -------------------------
    def geno_set_block(self, b_global, rows, nsamp):
        """Stage the .bed rows of block b_global (uint8, one row per marker, at
        least ceil(nsamp / 4) bytes each) if this rank owns it; returns the
        (n_b, 4) int64 counts of the codes 0..3 per marker, or None."""
        if not (self.b0 <= b_global < self.b1):
            return None
        rows = np.asarray(rows)
        n = self.block_sizes[b_global]
        if rows.dtype != np.uint8 or rows.ndim != 2 or rows.shape[0] != n \
                or rows.shape[1] < (int(nsamp) + 3) // 4 or int(nsamp) < 1:
            raise ValueError("genotype rows of block %d: %s %s, expected uint8 (%d, >= %d)"
                             % (b_global, rows.dtype, rows.shape, n, (int(nsamp) + 3) // 4))
        rows = np.ascontiguousarray(rows)
        counts = np.empty((n, 4), dtype=np.int64)
        self.ctx.sgv_geno_set_block(b_global - self.b0, rows.ctypes.data_as(hb._c_u8_p),
                                    int(rows.shape[1]), int(nsamp),
                                    counts.ctypes.data_as(hb._c_i64_p))
        return counts

    def geno_ld(self, ld, b_global):
        """R_b = G_b G_b^T of the staged genotypes into LD matrix ld (this rank's
        block; the engine's packing and precision)."""
        if not (self.b0 <= b_global < self.b1):
            return
        self.ctx.sgv_geno_ld(int(ld), b_global - self.b0)

    def geno_ld_factor(self, ld, b_global):
        """Block b_global of LD matrix ld becomes a factor block (sgv_geno_ld_factor):
        the staged rows and tables are handed over and every pass applies G_b (G_b^T
        p).  The staged block is empty afterwards: geno_r / geno_g need a fresh
        geno_set_block, or run before this."""
        if not (self.b0 <= b_global < self.b1):
            return
        self.ctx.sgv_geno_ld_factor(int(ld), b_global - self.b0)

    def geno_ld_band(self, ld, b_global, window):
        """Windowed R_b of the staged genotypes (entries with |i - j| <= window, 0
        elsewhere) into LD matrix ld as a packed band (this rank's block; the
        engine's precision; packing must be on)."""
        if not (self.b0 <= b_global < self.b1):
            return
        self.ctx.sgv_geno_ld_band(int(ld), b_global - self.b0, int(window))

    def geno_coupling(self, ld, gb, nr, nc, rows, nsamp, window, check=None):
        """Coupling between band pieces gb and gb + 1 (global indices) of LD matrix
        ld from genotypes: rows = a callable returning, or an array of, the (nr +
        nc, >= ceil(nsamp / 4)) uint8 .bed rows of gb's last nr markers, then gb +
        1's first nc; read only where this rank owns one of the two pieces.  Called
        on every rank for every coupling.  Returns the rows' (nr + nc, 4) code
        counts, or None.  check(counts), if given, runs before the library's error
        for rows without LD is raised, so the caller can name them."""
        return self._geno_coupling("sgv_geno_coupling", ld, gb, nr, nc, rows, nsamp,
                                   lambda own, n: (int(window),), check)

    def _geno_coupling(self, entry, ld, gb, nr, nc, rows, nsamp, own_args, check):
        """The two genotype couplings: the halo rows are read and validated only
        where this rank owns one of the two pieces; own_args(own, n) gives the
        entry's own arguments (between nsamp and the counts)."""
        own = self.b0 <= gb < self.b1 or self.b0 <= gb + 1 < self.b1
        n = int(nr) + int(nc)
        counts, rp, cp, nb = None, None, None, 0
        if own:
            rows = np.asarray(rows() if callable(rows) else rows)
            if rows.dtype != np.uint8 or rows.ndim != 2 or rows.shape[0] != n \
                    or rows.shape[1] < (int(nsamp) + 3) // 4 or int(nsamp) < 1:
                raise ValueError("genotype rows of coupling %d: %s %s, expected uint8 (%d, >= %d)"
                                 % (gb, rows.dtype, rows.shape, n, (int(nsamp) + 3) // 4))
            rows = np.ascontiguousarray(rows)
            counts = np.zeros((n, 4), dtype=np.int64)
            rp, cp, nb = rows.ctypes.data_as(hb._c_u8_p), counts.ctypes.data_as(hb._c_i64_p), \
                int(rows.shape[1])
        args = own_args(own, n)
        rc = getattr(self.ctx.lib, entry)(self.ctx.h, int(ld), int(gb), int(nr), int(nc), rp, nb,
                                          int(nsamp), *args, cp)
        if rc != hb.SGV_OK and check is not None and counts is not None:
            check(counts)
        self.ctx.check(rc, entry)
        return counts

    def geno_ld_band_reach(self, ld, b_global, hi, pos=None, span=0.0):
        """Distance-windowed R_b of the staged genotypes (include/sgvamp_hip.h,
        "distance-windowed genotype LD"): entries (i, j), i <= j <= hi[i], mirrored,
        0 elsewhere; with pos (the block's positions) and span each times 1 -
        (pos[j] - pos[i]) / span, the triangular taper.  A packed band by the widest
        reach (this rank's block; the engine's precision; packing must be on)."""
        if not (self.b0 <= b_global < self.b1):
            return
        hi = np.ascontiguousarray(hi, dtype=np.int32).ravel()
        n = int(self.block_sizes[b_global])
        if len(hi) != n or (pos is not None and np.size(pos) != n):
            raise ValueError("reach of block %d: %d entries (positions: %s), the block has %d "
                             "markers" % (b_global, len(hi),
                                          "none" if pos is None else np.size(pos), n))
        pp = None
        if pos is not None:
            pos = np.ascontiguousarray(pos, dtype=np.float64).ravel()
            pp = hb.dptr(pos)
        self.ctx.sgv_geno_ld_band_reach(int(ld), b_global - self.b0,
                                        hi.ctypes.data_as(hb._c_i32_p), pp, float(span))

    def geno_coupling_reach(self, ld, gb, nr, nc, rows, nsamp, keep, pos=None, span=0.0,
                            check=None):
        """geno_coupling with keep (nr counts of head columns: entry (a, c) is kept
        iff c < keep[a]) in place of the window and, for the taper, pos (the nr + nc
        halo rows' positions) and span.  Called on every rank for every coupling."""
        def own_args(own, n):
            if not own:
                return None, None, float(span)
            k = np.ascontiguousarray(keep, dtype=np.int32).ravel()
            if len(k) != int(nr) or (pos is not None and np.size(pos) != n):
                raise ValueError("coupling %d: %d kept-column counts for %d tail rows (positions: "
                                 "%s for %d halo rows)" % (gb, len(k), int(nr),
                                                           "none" if pos is None else np.size(pos), n))
            pp = None
            if pos is not None:
                pp = hb.dptr(np.ascontiguousarray(pos, dtype=np.float64).ravel())
            return k.ctypes.data_as(hb._c_i32_p), pp, float(span)
        return self._geno_coupling("sgv_geno_coupling_reach", ld, gb, nr, nc, rows, nsamp,
                                   own_args, check)

    def geno_r(self, k, y):
        """r_k = G y over this rank's blocks (get_vector(VEC_R, k) reads it)."""
        y = np.ascontiguousarray(y, dtype=np.float64).ravel()
        self.ctx.sgv_geno_r(int(k), hb.dptr(y))

    def geno_g(self, beta_full, nsamp):
        """Per owned block g_b = X_std,b^T beta_b: (local blocks, nsamp)."""
        beta = np.ascontiguousarray(np.asarray(beta_full, dtype=np.float64).ravel()[self.sl])
        g = np.empty((len(self.local_sizes), int(nsamp)), dtype=np.float64)
        self.ctx.sgv_geno_g(hb.dptr(beta), hb.dptr(g))
        return g

    def geno_clear(self):
        """Free the staged genotypes and their tables."""
        self.ctx.sgv_geno_clear()

    # ---- scoring a target panel (sgv_score_*) ---------------------------------
    def score_begin(self, nsamp, ncol):
        """Start a scoring stream over a target panel of nsamp samples for ncol
        (1..hb.SCORE_MAXCOL) effect columns.  Needs no LD and leaves the LD, the
        staged genotypes and the vectors of this engine alone."""
        self.ctx.sgv_score_begin(int(nsamp), int(ncol))
        self._score_shape = (int(nsamp), int(ncol))

    def score_chunk(self, rows, beta, mode=hb.SCORE_TARGET, tab=None):
        """Add the stream's next markers: rows (n, >= ceil(nsamp / 4)) uint8 .bed
        rows, beta (ncol, n) effects, tab (n, 4) for mode hb.SCORE_TABLE.  Every
        chunk but the last holds a multiple of 1,024 markers.  Returns the (n, 4)
        int64 counts of the codes 0..3 per marker."""
        rows = np.asarray(rows)
        if rows.dtype != np.uint8 or rows.ndim != 2:
            raise ValueError("score rows: %s %s, expected a 2-d uint8 array"
                             % (rows.dtype, rows.shape))
        rows = np.ascontiguousarray(rows)
        n = rows.shape[0]
        beta = hb.f64(beta)
        if beta.ndim == 1:
            beta = beta.reshape(1, -1)
        if beta.ndim != 2 or beta.shape[1] != n:
            raise ValueError("score effects: %s, expected (ncol, %d)" % (beta.shape, n))
        ncol = getattr(self, "_score_shape", (0, beta.shape[0]))[1]
        if beta.shape[0] != ncol:
            raise ValueError("score effects: %d columns, the stream has %d" % (beta.shape[0], ncol))
        tp = None
        if tab is not None:
            tab = hb.f64(tab)
            if tab.shape != (n, 4):
                raise ValueError("score tab: %s, expected (%d, 4)" % (tab.shape, n))
            tp = hb.dptr(tab)
        counts = np.empty((n, 4), dtype=np.int64)
        self.ctx.sgv_score_chunk(rows.ctypes.data_as(hb._c_u8_p), int(rows.shape[1]), int(n),
                                 int(mode), tp, hb.dptr(beta), int(n),
                                 counts.ctypes.data_as(hb._c_i64_p))
        return counts

    def score_end(self):
        """End the stream: (ncol, nsamp) scores."""
        if not hasattr(self, "_score_shape"):
            self.ctx.sgv_score_end(None)     # the library's refusal (no stream)
        nsamp, ncol = self._score_shape
        out = np.empty((ncol, nsamp), dtype=np.float64)
        self.ctx.sgv_score_end(hb.dptr(out))
        return out

    def score_timers(self, reset=False):
        t = np.zeros(hb.SCORE_TIMERS_N)
        self.ctx.sgv_score_timers(hb.dptr(t), len(t), int(bool(reset)))
        return dict(kernel_ms=t[0], chunks=int(t[1]), flops=t[2], stage_ms=t[3])

    # ---- hot path ------------------------------------------------------------
    def denoise(self, gam1s, a, lam, omegas, sigmas, rho, damp):
        out = np.zeros(self.K)
        om = hb.f64(omegas)
        sg = hb.f64(sigmas)
        self.ctx.sgv_denoise(hb.dptr(hb.f64(gam1s)), hb.dptr(hb.f64(a)), float(lam), len(sg),
                             hb.dptr(om), hb.dptr(sg), float(rho), int(bool(damp)), hb.dptr(out))
        return out

    def em(self, gam1s, a, sigmas, maxit, lam, omegas):
        lam_io = np.array([lam], dtype=np.float64)
        om = hb.f64(np.array(omegas, dtype=np.float64).copy())
        sg = hb.f64(sigmas)
        steps = np.zeros(1, dtype=np.int32)
        err = np.zeros(1)
        self.ctx.sgv_em(hb.dptr(hb.f64(gam1s)), hb.dptr(hb.f64(a)), len(sg), hb.dptr(sg),
                        int(maxit), hb.dptr(lam_io), hb.dptr(om), hb.iptr(steps), hb.dptr(err))
        return float(lam_io[0]), om, int(steps[0]), float(err[0])

    def posterior(self, gam1s, a, lam, omegas, sigmas, thr=0.95, resp=False):
        """The per-marker posterior at the context's current r1 (sgv_posterior):
        dict(pip, lodds, var [Mloc], sums = [sum pip, sum var, count(pip >= thr)]
        over all ranks, and with resp=True resp [nslab][Mloc], the slab
        responsibilities given inclusion)."""
        om = hb.f64(omegas)
        sg = hb.f64(sigmas)
        n = max(self.Mloc, 1)
        pip, lodds, var = np.empty(n), np.empty(n), np.empty(n)
        rsp = np.empty((len(sg), n)) if resp else None
        if rsp is not None and n != self.Mloc:
            raise ValueError("resp needs at least one local marker")
        sums = np.zeros(hb.POSTERIOR_ROWS)
        self.ctx.sgv_posterior(hb.dptr(hb.f64(gam1s)), hb.dptr(hb.f64(a)), float(lam), len(sg),
                               hb.dptr(om), hb.dptr(sg), float(thr), hb.dptr(pip), hb.dptr(lodds),
                               hb.dptr(var), None if rsp is None else hb.dptr(rsp), hb.dptr(sums))
        out = dict(pip=pip[:self.Mloc], lodds=lodds[:self.Mloc], var=var[:self.Mloc], sums=sums)
        if rsp is not None:
            out["resp"] = rsp
        return out

    def set_posterior_outputs(self, on, thr=0.95):
        """Posterior rows in the output slots (sgv_set_posterior_outputs): with on,
        outputs_wait returns (K + 4, Mloc) -- rows K + 1 .. K + 3 = pip, lodds, var of
        steps flagged hb.STEP_POSTERIOR.  Call before the first step."""
        self.ctx.sgv_set_posterior_outputs(int(bool(on)), float(thr))
        self.posterior_rows = hb.POSTERIOR_ROWS if on else 0

    def outputs_begin(self, slot):
        """Queue xhat1 and r1[k] (this rank's slice) into pinned slot 0/1 (no wait)."""
        self.ctx.sgv_outputs_begin(int(slot))

    def outputs_wait(self, slot):
        """Wait for slot's copy (any thread); returns a (K + 1, Mloc) view of the
        pinned buffer -- (K + 4, Mloc) after set_posterior_outputs(True) -- valid
        until the slot is begun again."""
        p = hb._c_dbl_p()
        rc = self.ctx.lib.sgv_outputs_wait(self.ctx.h, int(slot), ctypes.byref(p))
        if rc != hb.SGV_OK:
            raise hb.HipError("sgv_outputs_wait failed (%d)" % rc)
        rows = self.K + 1 + self.posterior_rows
        return np.ctypeslib.as_array(p, shape=(rows, max(self.Mloc, 1)))[:, :self.Mloc]

    def mle_exp_max(self, gam1s, sigma2):
        """max over (k, m, l) of (-r1_km^2 / 2) / (sigma2_l + 1/gam1_k) (src/sgvamp.py:152)."""
        out = np.zeros(1)
        sg = hb.f64(sigma2)
        self.ctx.sgv_mle_exp_max(hb.dptr(hb.f64(gam1s)), len(sg), hb.dptr(sg), hb.dptr(out))
        return float(out[0])

    def mle_terms(self, a, gam1s, sigma2, omega, exp_max):
        """The L marker sums of Lagrangian_der (src/sgvamp.py:153-157)."""
        sg = hb.f64(sigma2)
        out = np.zeros(len(sg))
        self.ctx.sgv_mle_terms(hb.dptr(hb.f64(a)), hb.dptr(hb.f64(gam1s)), len(sg), hb.dptr(sg),
                               hb.dptr(hb.f64(omega)), float(exp_max), hb.dptr(out))
        return out

    def set_mle_gam(self, gam):
        """The Lagrange multiplier SGV_STEP_MLE steps start from (None = the reference's)."""
        self.ctx.sgv_set_mle_gam(float("nan") if gam is None else float(gam))

    def mle_update(self, gam1s, a, sigmas, lam, omegas, gam):
        """The whole MLE prior update in the library (sgv_mle_update,
        src/sgvamp.py:162-194): returns (status, lam, omegas, gam); status 0 =
        updated, hb.MLE_NOT_CONVERGED / hb.MLE_NEGATIVE = the reference's "No prior
        update!" cases (inputs returned unchanged).  gam None = the reference's."""
        sg = hb.f64(sigmas)
        lam_io = np.array([lam], dtype=np.float64)
        om = np.array(omegas, dtype=np.float64).copy()
        g = np.array([np.nan if gam is None else gam], dtype=np.float64)
        st = np.zeros(1, dtype=np.int32)
        self.ctx.sgv_mle_update(hb.dptr(hb.f64(gam1s)), hb.dptr(hb.f64(a)), len(sg), hb.dptr(sg),
                                hb.dptr(lam_io), hb.dptr(om), hb.dptr(g), hb.iptr(st))
        return int(st[0]), float(lam_io[0]), om, (None if np.isnan(g[0]) else float(g[0]))

    def lmmse(self, it, gamw, gam2, alpha1, alpha2_prev, probes_local, cg_maxit, lmmse_damp, rho,
              learn_gamw, rtol=1e-5):
        K = self.K
        out = np.zeros((K, hb.LMMSE_NOUT))
        cg = np.zeros((K, 4), dtype=np.int32)
        passes = np.zeros(1, dtype=np.int32)
        pr = np.ascontiguousarray(probes_local, dtype=np.int8)
        if pr.shape != (K, self.Mloc):
            raise ValueError("probes must be (K, Mloc) int8")
        self.ctx.sgv_lmmse(int(it), hb.dptr(hb.f64(gamw)), hb.dptr(hb.f64(gam2)),
                           hb.dptr(hb.f64(alpha1)), hb.dptr(hb.f64(alpha2_prev)),
                           pr.ctypes.data_as(hb._c_i8_p), int(cg_maxit), float(rtol),
                           int(bool(lmmse_damp)), float(rho), int(bool(learn_gamw)), hb.dptr(out),
                           hb.iptr(cg), hb.iptr(passes))
        return out, cg, int(passes[0])

    def step_begin(self, it, flags, em_maxit, sigmas, a, lam, omegas, gam1s, rho, gamw,
                   alpha1_prev, alpha2_prev, probes_local, cg_maxit, out_slot, rtol=1e-5):
        """One outer iteration (sgv_step) on the library's worker thread; returns a
        handle for step_end.  Until then only host work that does not touch the
        context may run (outputs_wait excepted).  With hb.STEP_CHAIN in flags the
        scalar inputs come from the step queued before this one."""
        K = self.K
        sg = hb.f64(sigmas)
        pr = np.ascontiguousarray(probes_local, dtype=np.int8)
        if pr.shape != (K, self.Mloc):
            raise ValueError("probes must be (K, Mloc) int8")
        h = dict(lam=np.array([lam], dtype=np.float64),
                 om=np.array(omegas, dtype=np.float64).copy(),
                 pr=pr, ires=np.zeros(2, dtype=np.int32),
                 res=np.zeros(1 + 2 * K + 4
                              + (hb.POSTERIOR_ROWS if int(flags) & hb.STEP_POSTERIOR else 0)),
                 out=np.zeros((K, hb.LMMSE_NOUT)), cg=np.zeros((K, 4), dtype=np.int32))
        self.ctx.sgv_step_begin(int(it), int(flags), int(em_maxit), len(sg), hb.dptr(sg),
                                hb.dptr(hb.f64(a)), hb.dptr(h["lam"]), hb.dptr(h["om"]),
                                hb.dptr(hb.f64(gam1s)), float(rho), hb.dptr(hb.f64(gamw)),
                                hb.dptr(hb.f64(alpha1_prev)), hb.dptr(hb.f64(alpha2_prev)),
                                pr.ctypes.data_as(hb._c_i8_p), int(cg_maxit), float(rtol),
                                int(out_slot), hb.dptr(h["res"]), hb.iptr(h["ires"]),
                                hb.dptr(h["out"]), hb.iptr(h["cg"]))
        return h

    def step_end(self, h):
        """Wait for the oldest queued step; returns dict(lam, omegas, em_steps,
        em_err, alpha1, gam2, metrics, out, cg, passes, posterior_sums) (see
        sgv_step; posterior_sums is empty without hb.STEP_POSTERIOR)."""
        self.ctx.sgv_step_end()
        K = self.K
        return dict(lam=float(h["lam"][0]), omegas=h["om"], em_steps=int(h["ires"][0]),
                    em_err=float(h["res"][0]), mle_status=int(h["ires"][0]),
                    mle_gam=(None if np.isnan(h["res"][0]) else float(h["res"][0])),
                    alpha1=h["res"][1:1 + K].tolist(),
                    gam2=h["res"][1 + K:1 + 2 * K].tolist(),
                    metrics=h["res"][1 + 2 * K:1 + 2 * K + 4],
                    posterior_sums=h["res"][1 + 2 * K + 4:],
                    out=h["out"], cg=h["cg"], passes=int(h["ires"][1]))

    def metrics(self):
        out = np.zeros(4)
        self.ctx.sgv_metrics(hb.dptr(out))
        return out

    def metrics_begin(self):
        """Queue the metric sums behind the denoiser (no host wait)."""
        self.ctx.sgv_metrics_begin()

    def metrics_end(self):
        out = np.zeros(4)
        self.ctx.sgv_metrics_end(hb.dptr(out))
        return out

    # ---- operator seam (tests) ------------------------------------------------
    def ld_matvec(self, ld, V_local):
        V = np.ascontiguousarray(np.atleast_2d(V_local), dtype=np.float64)
        Y = np.empty_like(V)
        self.ctx.sgv_ld_matvec(int(ld), V.shape[0], hb.dptr(V), hb.dptr(Y))
        return Y

    def ld_pass_ex(self, ld, V_local, c1, c2, w=None, dot_mask=0, yout_mask=0, ys1=0.0, ys0=0.0,
                   run=-1, out=None, yout=None):
        """One pass over the raw R of LD matrix ld with the whole fused epilogue
        (sgv_ld_pass_ex): returns (out, yout, dots).  out / yout: the buffers'
        contents before the pass (default zeros; a no-op pass returns them).
        w None with a dot_mask: the dots alias the input columns."""
        V = np.ascontiguousarray(np.atleast_2d(V_local), dtype=np.float64)
        n = V.shape[0]
        O = np.zeros_like(V) if out is None else hb.f64(out).copy()
        Y = np.zeros_like(V) if yout is None else hb.f64(yout).copy()
        W = None if w is None else hb.f64(w)
        if O.shape != V.shape or Y.shape != V.shape or (W is not None and W.shape != V.shape):
            raise ValueError("out, yout and w must have the shape of V")
        c1, c2 = hb.f64(c1), hb.f64(c2)
        if c1.shape != (n,) or c2.shape != (n,):
            raise ValueError("c1 and c2 must have one entry per column")
        dots = np.zeros(n)
        self.ctx.sgv_ld_pass_ex(int(ld), n, hb.dptr(V), hb.dptr(c1), hb.dptr(c2),
                                None if W is None else hb.dptr(W), int(dot_mask), int(yout_mask),
                                float(ys1), float(ys0), int(run), hb.dptr(O), hb.dptr(Y),
                                hb.dptr(dots))
        return O, Y, dots

    def cg_solve(self, ld, c1, c2, B_local, X0_local, maxiter, rtol=1e-5):
        B = np.ascontiguousarray(np.atleast_2d(B_local), dtype=np.float64)
        X = np.ascontiguousarray(np.atleast_2d(X0_local), dtype=np.float64).copy()
        n = B.shape[0]
        it = np.zeros(n, dtype=np.int32)
        info = np.zeros(n, dtype=np.int32)
        self.ctx.sgv_cg_solve(int(ld), n, hb.dptr(hb.f64(c1)), hb.dptr(hb.f64(c2)), hb.dptr(B),
                              hb.dptr(X), int(maxiter), float(rtol), hb.iptr(it), hb.iptr(info))
        return X, it, info

    def timers(self, reset=False):
        t = np.zeros(hb.TIMERS_N)
        self.ctx.sgv_timers(hb.dptr(t), len(t), int(bool(reset)))
        return dict(ld_ms=t[0], ld_launches=int(t[1]), ld_bytes=t[2], rhs_bytes=t[3],
                    dense_bytes=t[4], aux_bytes=t[5], ld_flops=t[6], wide_flops=t[7],
                    wide_ms=t[8], wide_launches=int(t[9]))

    def exchange_stats(self, reset=False):
        """Cross-rank exchange counters (sgv_exchange_stats): all-gathers issued,
        ms in them, bytes contributed, the EM loops' modes and the cost model's
        last decision, the exact-CG host waits."""
        t = np.zeros(hb.EXCHANGE_STATS_N)
        self.ctx.sgv_exchange_stats(hb.dptr(t), len(t), int(bool(reset)))
        return dict(allgathers=int(t[0]), ms=float(t[1]), bytes=float(t[2]),
                    em_mode={1: "replicated", 0: "per-step", -1: None}[int(t[3])],
                    latency_us=float(t[4]),
                    latency_source={0: "default", 1: "env SGV_XCHG_LAT_US",
                                    2: "measured (sgv_exchange_probe)"}[int(t[12])],
                    transport={1: "rccl", 2: "host", 0: None}[int(t[5])],
                    em_loops_replicated=int(t[6]), em_loops_per_step=int(t[7]),
                    em_pred_replicated_us=float(t[8]), em_pred_per_step_us=float(t[9]),
                    em_pred_steps=float(t[10]), host_wait_ms=float(t[11]),
                    em_replicated_possible=bool(t[13]), em_ms=float(t[14]),
                    em_loops_timed=int(t[15]))

    def comm_info(self):
        """Who the exchange talks to (sgv_comm_info): transport, ranks in the
        communicator and this rank in it (RCCL's own ncclCommCount /
        ncclCommUserRank), the HIP device and its PCI bus id."""
        t = np.zeros(hb.COMM_INFO_N, dtype=np.int32)
        pci = ctypes.create_string_buffer(64)
        self.ctx.sgv_comm_info(hb.iptr(t), len(t), pci, len(pci))
        return dict(transport={1: "rccl", 2: "host", 0: None}[int(t[0])], comm_ranks=int(t[1]),
                    comm_rank=int(t[2]), device=int(t[3]), nranks=int(t[4]),
                    pci_bus_id=pci.value.decode(errors="replace"))

    def exchange_probe(self, reps=20):
        """Measure the exchange's per-all-gather latency (collective) and make the
        maximum over ranks the EM cost model's parameter; returns it in us."""
        us = np.zeros(1)
        self.ctx.sgv_exchange_probe(int(reps), hb.dptr(us))
        return float(us[0])

    def set_ld_packing(self, packed):
        """True: symmetric blocks set/generated from now on are stored packed."""
        self.ctx.sgv_set_ld_packing(int(bool(packed)))

    def set_ld_precision(self, bits):
        """64 (default) or 32: the element type of packed blocks (triangle, band)
        set or generated from now on.  32 rounds R once, on store, to the nearest
        f32 and halves the stored bytes; every product and sum stays f64.  A block
        stored as the full square stays f64."""
        self.ctx.sgv_set_ld_precision(int(bits))

    def ld_block_precision(self, ld, b_global):
        """64 or 32: the element type LD matrix ld's block b_global is stored in."""
        f = np.zeros(1, dtype=np.int32)
        self.ctx.sgv_ld_block_precision(int(ld), b_global - self.b0, hb.iptr(f))
        return int(f[0])

    def ld_pass_form(self, ld, ncol):
        """The kernel form the next pass of ncol columns over LD matrix ld takes
        (hb.PassForm: the packed kind by name, load and finalize forms, Pk layout,
        ...), under the switches as that pass would read them.  Host only, beyond
        the plan tables a first pass builds anyway."""
        f = np.zeros(len(hb.PASS_FORM_FIELDS), dtype=np.int32)
        self.ctx.sgv_ld_pass_form(int(ld), int(ncol), hb.iptr(f), len(f))
        return hb.pass_form_of(f)

    def ld_block_format(self, ld, b_global):
        f = np.zeros(1, dtype=np.int32)
        self.ctx.sgv_ld_block_format(int(ld), b_global - self.b0, hb.iptr(f))
        return int(f[0])

    def sync(self):
        self.ctx.sgv_sync()

    def read_bw(self, nbytes=8 << 30, reps=5):
        """The device's streaming-read rate in GB/s (sgv_read_bw), best of reps."""
        out = np.zeros(1)
        self.ctx.sgv_read_bw(int(nbytes), int(reps), hb.dptr(out))
        return float(out[0])

    def close(self):
        self.ctx.close()
