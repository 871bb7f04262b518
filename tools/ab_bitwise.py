#!/usr/bin/env python3
"""Bitwise A/B of two builds: run fixed LD passes (packed VALU/MFMA, dense, the
wide-item block sizes, band; the last two also f32-stored), full VAMP runs of
golden cases and every LD form built from .bed genotypes through the library at
--lib, print one SHA-256 per result.  Two builds whose lines are equal produce the
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


if __name__ == "__main__":
    main()
