"""The factor LD form (csrc/geno_factor.hip, sgv_geno_ld_factor): every LD pass
applies R_b p as G_b (G_b^T p) from the block's 2-bit genotype rows.

Extents the kernels cut a block by, and the shapes that cross them:
  markers  GF_TILE = 64 (a workgroup / partial slot of the second product; its
           loader takes rows four at a time), GF_SLAB = 1024 (a slab partial of the
           first product): EXACT_SIZES holds 50 < 64 = 64 < 130 and 700 < 1024 =
           1024 < 1025, beside test_gpu_geno_ld's 50, 130, 257, 700;
  samples  16 (a word), 256 (GF_SCH, a workgroup of the first product, and the 16-
           word tile of the second), ceil(words / 4) words per wave chunk: N = 64
           (4 words, one per wave), 256 (= GF_SCH, 4 words per wave), 1024 (> GF_SCH,
           one whole 16-word tile per wave) in the exact test; 5 (less than a
           word, three idle waves), 130, 500 and 1027 (ragged last word, ragged
           chunks) in the general one.

1. exact arithmetic (tests/factor_panels.py): out, yout and the dots equal ONE
   integer reference bit for bit at every column count, and the stored form on
   the same panel bit for bit -- no tolerance, independent of any sum's order.
2. general panels: |q - q_ref| <= 2^-52 (N + n_b + 16) (|G| |G|^T |V|) per element,
   the standard bound of the two dot-product stages plus the reference's own
   rounding, and maxrel < 1e-12 (test_gpu_geno_ld.TOL: the same kind of sums at
   the same shapes).  Measured on the MI355X: profiles/geno_factor/tolerances.txt.
3. state and ownership; 4. one rank against two, bitwise; 5. a solve against the
   stored form's (1e-5 of the max-norm, the project's parity gate).
"""
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import hip_backend as hb
from engine import Engine
from ldio import write_bed

from tests import bed_ref
from tests import exact_ld as xl
from tests import factor_panels as fp
from tests import test_gpu_geno_ld as tg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT_SIZES = [50, 64, 130, 257, 700, 1024, 1025]
YS = (xl.YS1, xl.YS0)
OUT_FILL, YOUT_FILL = -12345.5, 54321.25
DOT_ALT, YOUT_ALT = 0x5555, 0x6666


def factor_engine(blocks, K=1, sizes=None, pack=bed_ref.pack):
    """An engine whose LD matrix 0 holds `blocks` (codes) as factor blocks."""
    eng = Engine(sizes or [c.shape[0] for c in blocks], K=K)
    for b, c in enumerate(blocks):
        cnt = eng.geno_set_block(b, pack(c), c.shape[1])
        np.testing.assert_array_equal(cnt, bed_ref.counts(c))
        eng.geno_ld_factor(0, b)
    return eng


def stored_engine(blocks):
    eng = Engine([c.shape[0] for c in blocks], K=1)
    for b, c in enumerate(blocks):
        eng.geno_set_block(b, bed_ref.pack(c), c.shape[1])
        eng.geno_ld(0, b)
    return eng


# ---- 1. exact arithmetic ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_data(N):
    blocks = [fp.exact_codes(n, N, 40 + b) for b, n in enumerate(EXACT_SIZES)]
    M = sum(EXACT_SIZES)
    V = xl.exact_rhs(16, M, fp.RHS_BITS, 300 + N)
    W = xl.exact_weights(16, M, 3, 301 + N)
    RV, RA = fp.exact_reference(blocks, V)
    for a in blocks + [V, W, RV, RA]:
        a.setflags(write=False)
    return blocks, V, W, RV, RA


def call(eng, V, c1, c2, w=None, dot_mask=0, yout_mask=0, run=-1):
    return eng.ld_pass_ex(0, V, c1, c2, w=w, dot_mask=dot_mask, yout_mask=yout_mask, ys1=YS[0],
                          ys0=YS[1], run=run, out=np.full_like(V, OUT_FILL),
                          yout=np.full_like(V, YOUT_FILL))


def expect(N, V, RV, RA, c1, c2, w, dot_mask, yout_mask, tag, got):
    ncol, M = V.shape
    bits = N.bit_length() - 1      # the products' grid: multiples of 1 / N
    xl.check_exact(None, V, c1, c2, bits, w=w, ys=YS if yout_mask else None, RA=RA)
    out, yout, dots = xl.reference(RV, V, c1, c2, w=w, ys=YS)
    np.testing.assert_array_equal(got[0], out, err_msg="out %s" % (tag,))
    for j in range(ncol):
        want = yout[j] if yout_mask >> j & 1 else np.full(M, YOUT_FILL)
        np.testing.assert_array_equal(got[1][j], want, err_msg="yout %s column %d" % (tag, j))
        if dot_mask >> j & 1:
            assert got[2][j] == dots[j], ("dot", tag, j, got[2][j], dots[j])


@pytest.mark.parametrize("N", fp.EXACT_NS)
def test_exact_bitwise_every_column_count(N):
    blocks, V16, W16, RV16, RA16 = exact_data(N)
    offs = np.concatenate([[0], np.cumsum(EXACT_SIZES)])
    fac, sto = factor_engine(blocks), stored_engine(blocks)
    try:
        for b in range(len(blocks)):
            assert fac.ld_block_format(0, b) == 3 and sto.ld_block_format(0, b) == 1
        for ncol in range(1, 17):
            f = fac.ld_pass_form(0, ncol)
            assert f.kind == "factor" and f.rest_kind == "none" and not f.dense, f
            V, W, RV, RA = V16[:ncol], W16[:ncol], RV16[:ncol], RA16[:ncol]
            full = (1 << ncol) - 1
            c1, c2 = xl.narrow_coeffs(ncol)
            dm, ym = DOT_ALT & full, YOUT_ALT & full
            first = call(fac, V, c1, c2, W, dm, ym)
            expect(N, V, RV, RA, c1, c2, W, dm, ym, (N, ncol, "alt"), first)
            ref = call(sto, V, c1, c2, W, dm, ym)
            for a, c in zip(first[:2], ref[:2]):       # the stored form, same panel
                np.testing.assert_array_equal(a, c, err_msg="stored %s" % ((N, ncol),))
            # everything on, the dots aliasing the input (the CG's pass)
            got = call(fac, V, c1, c2, None, full, full)
            expect(N, V, RV, RA, c1, c2, V, full, full, (N, ncol, "all"), got)
            # the other coefficient set, out only; sgv_ld_matvec
            k1, k2 = xl.wide_coeffs(ncol)
            got = call(fac, V, k1, k2)
            expect(N, V, RV, RA, k1, k2, None, 0, 0, (N, ncol, "wide"), got)
            np.testing.assert_array_equal(fac.ld_matvec(0, V), RV)
            # run = 0: a no-op; run = 1 is run = -1
            out, yout, _ = call(fac, V, c1, c2, W, dm, full, run=0)
            np.testing.assert_array_equal(out, np.full_like(out, OUT_FILL))
            np.testing.assert_array_equal(yout, np.full_like(out, YOUT_FILL))
            got = call(fac, V, c1, c2, W, dm, ym, run=1)
            expect(N, V, RV, RA, c1, c2, W, dm, ym, (N, ncol, "run=1"), got)
            if ncol in (1, 16):    # per-block partials: weights that vanish outside block b
                for b in range(len(blocks)):
                    Wb = np.zeros_like(W)
                    Wb[:, offs[b]:offs[b + 1]] = W[:, offs[b]:offs[b + 1]]
                    got = call(fac, V, c1, c2, Wb, full, 0)
                    expect(N, V, RV, RA, c1, c2, Wb, full, 0, (N, ncol, "block", b), got)
    finally:
        fac.close()
        sto.close()


# ---- 2. general panels -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def abs_G(N, miss):
    return [np.abs(bed_ref.G(c)) for c in tg.panel(N, miss)[0]]


@pytest.mark.parametrize("miss", tg.MISS)
@pytest.mark.parametrize("N", tg.NS)
def test_general_panels_within_derived_bound(N, miss):
    blocks, Rref = tg.panel(N, miss)
    aG = abs_G(N, miss)
    M = sum(tg.SIZES)
    rs = np.random.RandomState(7 * N + int(100 * miss))
    eng = factor_engine(blocks)
    # the same panel in rows three bytes longer, every padding position holding code 3
    dirty = factor_engine(blocks, pack=lambda c: bed_ref.pack(c, row_bytes=(N + 3) // 4 + 3,
                                                               pad_bits=3))
    try:
        assert eng.stored_bytes(0) == sum(n * ((N + 15) // 16) * 4 + n * 32 for n in tg.SIZES)
        for ncol in (1, 3, 8, 16):
            V = rs.normal(size=(ncol, M))
            Y = eng.ld_matvec(0, V)
            np.testing.assert_array_equal(dirty.ld_matvec(0, V), Y)
            worst = 0.0
            for b, n in enumerate(tg.SIZES):
                sl = slice(tg.OFFS[b], tg.OFFS[b + 1])
                ref = V[:, sl] @ Rref[b].T
                bound = 2.0 ** -52 * (N + n + 16) * ((np.abs(V[:, sl]) @ aG[b]) @ aG[b].T)
                err = np.abs(Y[:, sl] - ref)
                assert (err <= bound).all(), (N, miss, ncol, b, float((err / bound).max()))
                worst = max(worst, tg.maxrel(Y[:, sl], ref))
                assert tg.maxrel(Y[:, sl], ref) < tg.TOL
            print("factor N=%d miss=%g ncol=%d: maxrel %.3e" % (N, miss, ncol, worst))
    finally:
        eng.close()
        dirty.close()


# ---- 3. state and ownership ------------------------------------------------------
def test_state_and_ownership():
    N = 130
    blocks, Rref = tg.panel(N, 0.03)
    A, B = blocks[:2], [blocks[3][:50], blocks[2][:130]]     # two panels on blocks [50, 130]
    sizes = [50, 130]
    rs = np.random.RandomState(3)
    V = rs.normal(size=(2, 180))

    def product(codes):
        return np.concatenate([V[:, :50] @ bed_ref.R(codes[0]).T,
                               V[:, 50:] @ bed_ref.R(codes[1]).T], axis=1)

    # a factor matrix refuses stored blocks, and keeps multiplying as before
    eng = factor_engine(A, sizes=sizes)
    try:
        assert [eng.ld_block_format(0, b) for b in range(2)] == [3, 3]
        assert [eng.ld_block_precision(0, b) for b in range(2)] == [64, 64]
        assert eng.stored_bytes(0) == sum(n * ((N + 15) // 16) * 4 + n * 32 for n in sizes)
        before = eng.ld_matvec(0, V)
        assert tg.maxrel(before, product(A)) < tg.TOL
        with pytest.raises(hb.HipError, match=r"\(-4\).*factor block"):
            eng.get_ld_block(0, 0)
        with pytest.raises(hb.HipError, match=r"\(-4\).*no genotypes"):
            eng.geno_ld_factor(0, 0)                  # nothing staged: the hand-over emptied it
        with pytest.raises(hb.HipError, match=r"\(-4\)"):
            eng.geno_r(0, np.zeros(N))                # needs a fresh staging
        eng.geno_set_block(0, bed_ref.pack(A[0]), N)
        with pytest.raises(hb.HipError, match=r"\(-4\).*factor blocks"):
            eng.geno_ld(0, 0)
        with pytest.raises(hb.HipError, match=r"\(-4\).*factor blocks"):
            eng.geno_ld_band(0, 0, 10)
        with pytest.raises(hb.HipError, match=r"\(-4\).*factor blocks"):
            eng.set_ld_block(0, 0, np.eye(50))
        bad = np.array(A[0])
        bad[7] = 3                                    # monomorphic
        eng.geno_set_block(0, bed_ref.pack(bad), N)
        with pytest.raises(hb.HipError, match=r"\(-4\).*1 marker\(s\) without LD"):
            eng.geno_ld_factor(0, 0)
        assert eng.ld_block_format(0, 0) == 3
        np.testing.assert_array_equal(eng.ld_matvec(0, V), before)
        eng.geno_clear()                              # does not touch what was handed over
        np.testing.assert_array_equal(eng.ld_matvec(0, V), before)
    finally:
        eng.close()

    # a stored matrix refuses a factor block, and keeps multiplying as before
    eng = Engine(sizes, K=1)
    try:
        for b in range(2):
            eng.geno_set_block(b, bed_ref.pack(A[b]), N)
            eng.geno_ld(0, b)
        before = eng.ld_matvec(0, V)
        with pytest.raises(hb.HipError, match=r"\(-4\).*one form per LD matrix"):
            eng.geno_ld_factor(0, 1)
        assert [eng.ld_block_format(0, b) for b in range(2)] == [1, 1]
        np.testing.assert_array_equal(eng.ld_matvec(0, V), before)
        np.testing.assert_array_equal(eng.get_ld_block(0, 1), eng.get_ld_block(0, 1).T)
    finally:
        eng.close()

    # two LD matrices, two panels: staged and handed over block by block
    eng = Engine(sizes, K=2, ld_of=[0, 1])
    try:
        for b in range(2):
            eng.geno_set_block(b, bed_ref.pack(A[b]), N)
            eng.geno_ld_factor(0, b)
            eng.geno_set_block(b, bed_ref.pack(B[b]), N)
            eng.geno_ld_factor(1, b)
        ya, yb = eng.ld_matvec(0, V), eng.ld_matvec(1, V)
        assert tg.maxrel(ya, product(A)) < tg.TOL and tg.maxrel(yb, product(B)) < tg.TOL
        assert not np.array_equal(ya, yb)
        with pytest.raises(hb.HipError, match=r"\(-4\)"):
            eng.geno_r(0, np.zeros(N))
        eng.geno_clear()
        np.testing.assert_array_equal(eng.ld_matvec(1, V), yb)
    finally:
        eng.close()


# ---- 4. one rank against two -----------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_one_rank_vs_two_ranks_bitwise():
    """test_gpu_geno_ld's harness on a factor source (tools/geno_factor_ranks_gpu.py):
    a 4-iteration solve -- pipelined CG, both CG solves and the gamw pass -- writes
    the same files, bit for bit, from two ranks as from one."""
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2",
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), SGV_EXCHANGE="host")
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(ROOT, "tools", "geno_factor_ranks_gpu.py")], env=env,
            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(out)
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, out[-4000:])
    assert "bitwise equal -> OK" in outs[0], outs[0][-3000:]


# ---- 5. solve parity with the stored form ----------------------------------------
def test_cli_solve_matches_stored_form(tmp_path, monkeypatch):
    """main.py on a 800-marker panel of N = 1027 (four blocks of 200, K = 2 sharing
    it: N > n_b, R well conditioned), 10 iterations with --ld-form factor and
    without: the same files, the last xhat within 1e-5 of the stored run's max-norm
    (the two forms differ by rounding, and possibly by one CG iteration at a stop
    test).  Measured: profiles/geno_factor/tolerances.txt."""
    import main
    import simulate

    M, N, iters = 800, 1027, 10
    codes = bed_ref.draw_codes(M, N, miss=0.03, seed=91)
    prefix = write_bed(str(tmp_path / "p"), codes, *bed_ref.bim_fam(M, N))
    simulate.main(["--bed", prefix, "--out", str(tmp_path / "sim"), "--h2", "0.8", "--lam", "0.1",
                   "--seed", "3"])
    made = []

    class Spy(main.VAMP):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    monkeypatch.setattr(main, "VAMP", Spy)

    def run(out, extra):
        (tmp_path / out).mkdir()
        main.main(["--ld-files", "%s.bed,%s.bed" % (prefix, prefix), "--r-files",
                   "%s,%s" % (tmp_path / "sim_r.npy", tmp_path / "sim_r.npy"),
                   "--true-signal-file", str(tmp_path / "sim_bet.npy"), "--out-dir",
                   str(tmp_path / out), "--out-name", "run", "--N", "%d,%d" % (N, N), "--M",
                   "%d,%d" % (M, M), "--K", "2", "--iterations", str(iters), "--seed", "11",
                   "--prior-probs", "0.9,0.1", "--ld-block-size", "200"] + extra)
        cg = [rec["cg_iters"] for rec in made[-1].history if "cg_iters" in rec]
        return sorted(os.listdir(tmp_path / out)), cg

    fa, cga = run("stored", [])
    fb, cgb = run("factor", ["--ld-form", "factor"])
    assert fa == fb and sum(fn.endswith(".bin") for fn in fa) == iters * 3
    last = "run_xhat_it_%d.bin" % (iters - 1)
    xa, xb = np.fromfile(tmp_path / "stored" / last), np.fromfile(tmp_path / "factor" / last)
    assert np.isfinite(xb).all() and xb.any()
    diff = float(np.max(np.abs(xa - xb)) / np.max(np.abs(xa)))
    print("factor vs stored, xhat of iteration %d: max |diff| / max |x| = %.3e" % (iters - 1, diff))
    print("CG iterations stored: %s" % cga)
    print("CG iterations factor: %s" % cgb)
    assert diff < 1e-5, diff
