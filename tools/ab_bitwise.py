#!/usr/bin/env python3
"""Bitwise A/B of two builds: run fixed LD passes (packed VALU/MFMA, dense, the
wide-item block sizes, band; the last two also f32-stored), full VAMP runs of
golden cases, every LD form built from .bed genotypes and the solver's host
paths (LMMSE steps in every mode, the CG loops, the EM loops, the pass ledger)
through the library at --lib, print one SHA-256 per result.  Two builds whose lines are equal produce the
same bits (under the same SGV_AB switches: run it once per arm).

  python tools/ab_bitwise.py --lib sgvamp-py_amd/libsgvamp_hip.so > a.txt
  python tools/ab_bitwise.py --lib ab_lib/base.so > b.txt; diff a.txt b.txt"""
import argparse
import hashlib
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sgvamp-py_amd"))
sys.path.insert(0, ROOT)


def h(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def geno(Engine):
    """Every LD form built from .bed genotypes (geno.hip), f64 and f32 stored: the
    dense build, marker windows across the tile and panel edges, a ragged reach
    without and with the taper, the corner by window and by kept columns (tests/
    test_gpu_geno_band.py's shapes), r and g."""
    import hip_backend as hb
    from tests import bed_ref
    sizes, N = [130, 257, 700], 130
    offs = np.concatenate([[0], np.cumsum(sizes)])
    codes = bed_ref.draw_codes(sum(sizes), N, miss=0.03, seed=7)
    rs = np.random.RandomState(11)
    hi = [np.maximum.accumulate(np.minimum(np.arange(n) + 1 + np.arange(n) * 7 % 90, n - 1))
          for n in sizes]
    pos = [np.cumsum(rs.uniform(0.5, 3.0, n)) for n in sizes]
    span = [1.25 * float(np.max(p[r] - p)) for p, r in zip(pos, hi)]
    pieces, nr, nc = [200, 150], 130, 70
    halo = bed_ref.pack(codes[pieces[0] - nr:pieces[0] + nc])
    E = np.zeros((nc, sum(pieces)))              # the head's unit vectors read C's columns
    E[np.arange(nc), pieces[0] + np.arange(nc)] = 1.0

    def corner(eng):
        return h(np.concatenate([eng.ld_matvec(0, E[c:c + 16])[:, pieces[0] - nr:pieces[0]]
                                 for c in range(0, nc, 16)]))
    for bits, tag in ((64, "f64"), (32, "f32")):
        eng = Engine(sizes, K=1)
        eng.set_ld_precision(bits)
        for b in range(len(sizes)):
            eng.geno_set_block(b, bed_ref.pack(codes[offs[b]:offs[b + 1]]), N)

        def blocks(what):
            print("geno %s %s %s" % (tag, what,
                                     " ".join(h(eng.get_ld_block(0, b)) for b in range(len(sizes)))))
        for b in range(len(sizes)):
            eng.geno_ld(0, b)
        blocks("ld")
        for W in (1, 64, 300):
            for b in range(len(sizes)):
                eng.geno_ld_band(0, b, W)
            blocks("band W=%d" % W)
        for taper in (False, True):
            for b in range(len(sizes)):
                eng.geno_ld_band_reach(0, b, hi[b], pos[b] if taper else None,
                                       span[b] if taper else 0.0)
            blocks("reach taper=%d" % taper)
        eng.geno_r(0, rs.normal(size=N))
        print("geno %s r %s" % (tag, h(eng.get_vector(hb.VEC_R, 0))))
        print("geno %s g %s" % (tag, h(eng.geno_g(rs.normal(size=sum(sizes)), N))))
        eng.close()
        eng = Engine(pieces, K=1)
        eng.set_ld_precision(bits)
        for b, (lo, up) in enumerate(((0, pieces[0]), (pieces[0], sum(pieces)))):
            eng.geno_set_block(b, bed_ref.pack(codes[lo:up]), N)
            eng.geno_ld(0, b)
        for W in (1, 64, 150):
            eng.geno_coupling(0, 0, nr, nc, halo, N, W)
            cw = corner(eng)
            eng.geno_coupling_reach(0, 0, nr, nc, halo, N,
                                    np.clip(W - nr + np.arange(nr) + 1, 0, nc))
            ck = corner(eng)
            print("geno %s corner W=%d window %s keep %s" % (tag, W, cw, ck))
        eng.close()


def hh(*parts):
    """One hash over several results (arrays, scalars, lists), in order."""
    return h(np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts]))


def ledger(eng):
    """The pass ledger's counts and bytes (timers() without its millisecond
    slots), read and cleared."""
    t = eng.timers(reset=True)
    return [t[k] for k in ("ld_launches", "ld_bytes", "rhs_bytes", "dense_bytes", "aux_bytes",
                           "ld_flops", "wide_flops", "wide_launches")]


def solver(Engine, VAMP, BlockLD, Case):
    """The host code that drives the CG, the LMMSE step and the EM loop (cg.hip,
    solver.hip, prior.hip): every line hashes the outputs with cg_out, the pass
    count and the ledger."""
    import hip_backend as hb
    from tests import lmmse_ref as lr
    from tests import marker_ref as mr
    from tests import test_gpu_marker_kernels as tm

    def lmmse_calls(eng, shape, K, rs, pipe, damp, learn):
        """Three consecutive calls: cold; warm (and damped); new gamw / gam2."""
        d = lr.t2_inputs(shape)
        eng.reset_solver()
        eng.set_rs_recurrence(rs)
        eng.set_cg_pipeline(pipe)
        eng.timers(reset=True)
        parts = []
        for n in range(3):
            gamw = [g * (1.7 if n == 2 else 1.0) for g in d["gamw"][:K]]
            gam2 = [g * (0.6 if n == 2 else 1.0) for g in d["gam2"][:K]]
            eng.set_vector(hb.VEC_XHAT1, 0, d["xhat1"])
            for k in range(K):
                eng.set_cohort_n(k, d["N"][k])
                eng.set_vector(hb.VEC_R, k, d["r"][k])
                eng.set_vector(hb.VEC_R1, k, d["r1"][n][k])
            out, cg, passes = eng.lmmse(n, gamw, gam2, d["alpha1"][n][:K], d["a2prev"][:K],
                                        d["u"][n][:K], lr.T2_MAXIT, damp and n > 0, lr.T2_RHO,
                                        learn, rtol=lr.T2_RTOL)
            parts += [out, cg, [passes], ledger(eng)]
            for which in (hb.VEC_XHAT2, hb.VEC_SIG2U, hb.VEC_R1):
                parts += [eng.get_vector(which, k) for k in range(K)]
        return hh(*parts)

    def lmmse_engine(shape, ld_of, exchange=None):
        S = lr.system(shape)
        eng = Engine(S.sizes, K=len(ld_of), ld_of=ld_of, exchange=exchange)
        S.upload(eng, sorted(set(ld_of)))
        eng.set_ridge(S.s)
        return eng

    modes = [(rs, pipe, damp, learn) for rs in (1, 0) for pipe in (1, 0) for damp in (0, 1)
             for learn in (0, 1)]
    for shape in lr.T2_SHAPES:        # cohorts 0 and 2 share an LD matrix, cohort 1 has its own
        eng = lmmse_engine(shape, lr.T2_LD_OF)
        for m in modes:
            print("solver lmmse %s K3 distinct rs=%d pipe=%d damp=%d learn=%d %s"
                  % ((shape,) + m + (lmmse_calls(eng, shape, 3, *m),)))
        eng.close()
    eng = lmmse_engine("mixed9", [0, 0, 0])      # one pass of 6 columns: the exact column sets
    for exact in (0, 1):
        eng.ctx.sgv_set_cg_exact(exact)
        for m in ((1, 1, 1, 1), (1, 0, 1, 1), (0, 1, 0, 1)):
            print("solver lmmse mixed9 K3 shared exact=%d rs=%d pipe=%d damp=%d learn=%d %s"
                  % ((exact,) + m + (lmmse_calls(eng, "mixed9", 3, *m),)))
    eng.close()
    for K in (1, 2):                  # the one-rank host exchange: CgMerge0 at one LD matrix
        eng = lmmse_engine(lr.T3_SHAPE, lr.T2_LD_OF[:K], exchange="host")
        for m in ((1, 1, 1, 1), (0, 1, 0, 1), (1, 0, 1, 0)):
            print("solver lmmse %s K%d rehearsal rs=%d pipe=%d damp=%d learn=%d %s"
                  % ((lr.T3_SHAPE, K) + m + (lmmse_calls(eng, lr.T3_SHAPE, K, *m),)))
        eng.close()
    for name in ("k10_shared", "k11_distinct"):   # more than MAXKG cohorts: two LMMSE groups
        c = Case(name)
        f = c.flags
        lds = [BlockLD(bl, s=f["s"]) for bl in c.ld_blocks]
        R = lds[0] if len(lds) == 1 else [lds[c.ld_of[k]] for k in range(c.K)]
        Nt = sum(c.N)
        with tempfile.TemporaryDirectory() as d:
            v = VAMP(N=c.N, Nt=Nt, M=c.M, K=c.K, rho=f["rho"], gamw=f["gamw"], gam1=f["gam1"],
                     a=np.array(c.N) / Nt, prior_vars=f["prior_vars"],
                     prior_probs=f["prior_probs"], out_dir=d, out_name=name, seed=f["seed"])
            xh = v.infer(R, c.r, f["iterations"], x0=c.x0, cg_maxit=f["cg_maxit"],
                         em_prior_maxit=f["em_prior_maxit"], learn_gamw=f["learn_gamw"],
                         lmmse_damp=f["lmmse_damp"], prior_update=f["prior_update"],
                         update_prior_from=f["update_prior_from"])
            print("solver vamp %s %s" % (name, hh(np.array(xh), [r["cg_iters"] for r in v.history],
                                                  ledger(v.engine))))
            v.engine.close()
    for part in ("edges", "mixed13"):            # the fused and the two-launch EM control
        for K, nslab in ((3, 3), (33, 2)):       # one and two cohort groups
            c = mr.case(("benign", 0, K, nslab), sum(mr.PARTS[part]))
            eng = Engine(mr.PARTS[part], K=K)
            for k, r in enumerate(c["r1s"]):
                eng.set_vector(hb.VEC_R1, k, r)
            for pipe in (1, 0):
                eng.set_cg_pipeline(pipe)
                got = [eng.em(c["gam1s"], c["a"], c["sigmas"], maxit, c["lam"], c["omegas"])
                       for maxit in (25, 1, 3)]
                print("solver em %s K=%d pipe=%d %s" % (part, K, pipe,
                                                      hh(*[x for g in got for x in g])))
            eng.close()
    for part in ("mixed8", "mixed9"):            # the fused and the two-launch CG control
        eng, _, bounds = tm._cg_system(part)
        M = int(bounds[-1])
        for pipe in (1, 0):
            for maxiter in (3, 4, 5):            # the mirror ring's boundary
                eng.timers(reset=True)
                X, it, info = tm._solve(eng, pipe, 0, *tm._columns(M, 2), maxiter)
                print("solver cg %s pipe=%d maxiter=%d %s" % (part, pipe, maxiter,
                                                             hh(X, it, info, ledger(eng))))
            for exact in (0, 1):
                eng.timers(reset=True)
                X, it, info = tm._solve(eng, pipe, exact, *tm._columns(M, 6), 500)
                print("solver cg %s pipe=%d exact=%d 6 columns %s" % (part, pipe, exact,
                                                                     hh(X, it, info, ledger(eng))))
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    a = ap.parse_args()
    import hip_backend
    hip_backend.load(a.lib, strict=False)   # an older build lacks the newest entry points
    from engine import Engine
    from simulate import windowed_ld
    from sgvamp import VAMP, BlockLD
    from tests.golden import Case

    rs = np.random.RandomState(1)
    sizes = [1500, 2600, 700]
    blocks = []
    for n in sizes:
        X = rs.normal(size=(n // 2, n)) / np.sqrt(n)
        B = X.T @ X
        blocks.append((B + B.T) / 2)
    V = rs.normal(size=(16, sum(sizes)))
    for fmt in ("packed", "packed_valu", "dense"):
        eng = Engine(sizes, K=1)
        eng.set_ld_packing(fmt != "dense")
        if fmt == "packed_valu":
            eng.set_mfma_min(0)
        eng.set_ridge(0.05)
        for b, B in enumerate(blocks):
            eng.set_ld_block(0, b, B)
        for nc in (1, 2, 3, 5, 8, 12, 16):
            print("matvec %s nc=%d %s" % (fmt, nc, h(eng.ld_matvec(0, V[:nc]))))
        eng.close()
    # the wide-item sizes (tests/test_gpu_wide_items.py): 9-panel column classes
    # (8 + 1-panel strip pairs), ragged chunk ends on, just past and far before
    # wave boundaries, a one-marker block; f64 and f32-stored
    wsizes = [8500, 1281, 513, 257, 1]
    wblocks = []
    for n in wsizes:
        U = np.triu(np.random.RandomState(1000 + n).standard_normal((n, n)) / np.sqrt(n))
        wblocks.append(U + np.triu(U, 1).T)
    VW = rs.normal(size=(16, sum(wsizes)))
    for bits, tag in ((64, "wide"), (32, "wide f32")):
        eng = Engine(wsizes, K=1)
        eng.set_ld_precision(bits)
        eng.set_ridge(0.1)
        for b, B in enumerate(wblocks):
            eng.set_ld_block(0, b, B)
        for nc in (3, 4, 5, 8, 13, 16):
            print("matvec %s nc=%d %s" % (tag, nc, h(eng.ld_matvec(0, VW[:nc]))))
        eng.close()
    A = windowed_ld(6000, 700, seed=3, taps=40)
    L = BlockLD.from_csr(A)
    W = rs.normal(size=(16, 6000))
    for bits, tag, ncs in ((64, "band", (1, 2, 8, 16)), (32, "band f32", (1, 2, 4, 8, 16))):
        eng = Engine(L.block_sizes, K=1)
        eng.set_ld_precision(bits)
        L.upload(eng, 0, 0)
        for nc in ncs:
            print("matvec %s nc=%d %s" % (tag, nc, h(eng.ld_matvec(0, W[:nc]))))
        eng.close()
    # many blocks (> 8): the two-launch reduction + control path at one rank
    import hip_backend as hb
    sizes = [300] * 20
    M = sum(sizes)
    beta = np.zeros(M)
    beta[rs.choice(M, M // 10, replace=False)] = rs.normal(0, 0.01, M // 10)
    for K in (1, 2):
        eng = Engine(sizes, K=K)
        g = eng.synth_ld_g(0, 5, 250, beta).sum(axis=0)
        for k in range(K):
            eng.synth_r(k, 5, 250, g + np.random.RandomState(k).normal(0, 0.4, 250))
        with tempfile.TemporaryDirectory() as d:
            v = VAMP(N=[250.0] * K, Nt=250.0 * K, M=M, K=K, rho=0.5, gamw=5.0, gam1=1e-6,
                     a=[1.0 / K] * K, prior_vars=[0.0, 0.8 / (M // 10) / K],
                     prior_probs=[0.9, 0.1], out_dir=d, out_name="many", seed=3,
                     write_files=False)
            v.attach_engine(eng, x0=beta * np.sqrt(250.0))
            xh = v.infer(None, None, 5, x0=beta * np.sqrt(250.0), lmmse_damp=True,
                         prior_update="em")
            print("vamp many-blocks K=%d %s cg=%s" % (K, h(np.array(xh)),
                                                     [r["cg_iters"] for r in v.history]))
        eng.close()
    del hb
    for name in ("k1_blocks_csr_s_damp", "k4_shared_s_damp", "k10_shared", "k2_mle_L3"):
        c = Case(name)
        f = c.flags
        lds = [BlockLD(bl, s=f["s"]) for bl in c.ld_blocks]
        R = lds[0] if len(lds) == 1 else [lds[c.ld_of[k]] for k in range(c.K)]
        Nt = sum(c.N)
        with tempfile.TemporaryDirectory() as d:
            v = VAMP(N=c.N, Nt=Nt, M=c.M, K=c.K, rho=f["rho"], gamw=f["gamw"], gam1=f["gam1"],
                     a=np.array(c.N) / Nt, prior_vars=f["prior_vars"],
                     prior_probs=f["prior_probs"], out_dir=d, out_name=name, seed=f["seed"])
            xh = v.infer(R, c.r, f["iterations"], x0=c.x0, cg_maxit=f["cg_maxit"],
                         em_prior_maxit=f["em_prior_maxit"], learn_gamw=f["learn_gamw"],
                         lmmse_damp=f["lmmse_damp"], prior_update=f["prior_update"],
                         update_prior_from=f["update_prior_from"])
            print("vamp %s %s" % (name, h(np.array(xh))))
            v.engine.close()
    geno(Engine)
    solver(Engine, VAMP, BlockLD, Case)


if __name__ == "__main__":
    main()
