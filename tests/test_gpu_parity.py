"""Parity of the HIP path (through the C ABI) with the oracle and with the
reference's golden outputs.  Run on an MI355X: python -m pytest tests -m gpu.

Tolerances (f64 everywhere; only the summation order differs from the oracle):
* LD pass, CG solution, denoiser, EM, generator: <= 1e-11 relative;
* full VAMP trajectories vs the reference fixtures: xhat/r1 <= 1e-8 relative to
  max|.| per iteration (the north-star bar is 1e-5), CG iteration counts and EM
  steps exact, cohort CSV values rtol 1e-5 (gam2 = gam1(1-a1)/a1 amplifies
  rounding when alpha1 -> 0; the oracle itself sits at 6e-7 there).
"""
import csv
import os

import numpy as np
import pytest

import hip_backend as hb
from engine import Engine
from oracle import synth_oracle as so
from oracle import vamp_oracle as vo
from sgvamp import VAMP, BlockLD
from tests.golden import Case, case_names

pytestmark = pytest.mark.gpu


def maxrel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


def rand_blocks(sizes, seed=0, nsamp=None, symmetric=True):
    rs = np.random.RandomState(seed)
    out = []
    for n in sizes:
        X = rs.normal(size=(nsamp or max(2 * n, 8), n))
        X /= np.sqrt(X.shape[0])
        B = X.T @ X
        if symmetric:
            B = (B + B.T) / 2          # exactly symmetric
        else:
            B = B + np.triu(rs.normal(scale=1e-3, size=(n, n)), 1)
        out.append(B)
    return out


# ---------------------------------------------------------------------------
# the LD pass (operator seam)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [[1], [7, 1, 130], [127, 128, 129], [300, 64, 1000, 33],
                                   [256, 257, 513], [1500, 2600]])
@pytest.mark.parametrize("ncol", [1, 2, 3, 5, 8, 12, 16])
@pytest.mark.parametrize("s", [0.0, 0.1])
@pytest.mark.parametrize("fmt", ["packed", "packed_valu", "dense", "nonsym"])
def test_ld_matvec_vs_numpy(sizes, ncol, s, fmt):
    """packed: f64 MFMA pass from 3 columns (sym_mfma.hip); packed_valu: VALU pass
    for every column count; dense/nonsym: full-square storage."""
    blocks = rand_blocks(sizes, seed=len(sizes) + ncol, symmetric=fmt != "nonsym")
    eng = Engine(sizes, K=1)
    eng.set_ld_packing(fmt.startswith("packed"))
    if fmt == "packed_valu":
        eng.set_mfma_min(0)
    for b, B in enumerate(blocks):
        eng.set_ld_block(0, b, B)
        assert eng.ld_block_format(0, b) == (1 if fmt.startswith("packed") else 0)
    eng.set_ridge(s)
    M = sum(sizes)
    V = np.random.RandomState(ncol).normal(size=(ncol, M))
    Y = eng.ld_matvec(0, V)
    L = vo.BlockLD(blocks, s=s)
    for j in range(ncol):
        ref = L.matvec_Rs(V[j])
        assert maxrel(Y[j], ref) < 1e-12, (j, maxrel(Y[j], ref))
    eng.close()


@pytest.mark.parametrize("packed", [True, False])
def test_ld_block_roundtrip(packed):
    sizes = [33, 200, 700]
    blocks = rand_blocks(sizes, 3)
    eng = Engine(sizes, K=1)
    eng.set_ld_packing(packed)
    for b, B in enumerate(blocks):
        eng.set_ld_block(0, b, B)
    for b, B in enumerate(blocks):
        np.testing.assert_array_equal(eng.get_ld_block(0, b), B)
    eng.close()


def test_ld_matvec_symmetry_and_linearity_large():
    """Size-independent properties at BASELINE block size (25k x 25k, 5 GB):
    u^T(Rv) = v^T(Ru) for symmetric R, linearity R(au+bv) = aRu + bRv."""
    sizes = [25000]
    eng = Engine(sizes, K=1)
    beta = np.zeros(25000)
    eng.synth_ld_g(0, 5, 2000, beta)        # R = G G^T, exactly symmetric by construction
    rs = np.random.RandomState(1)
    U = rs.normal(size=(3, 25000))
    U[2] = 0.3 * U[0] - 1.7 * U[1]
    Y = eng.ld_matvec(0, U)                 # 3 columns: the MFMA pass
    assert eng.ld_block_format(0, 0) == 1
    assert abs(U[0] @ Y[1] - U[1] @ Y[0]) <= 1e-11 * abs(U[0] @ Y[1])
    assert maxrel(Y[2], 0.3 * Y[0] - 1.7 * Y[1]) < 1e-11
    # 16 columns on the MFMA pass vs one column at a time on the VALU pass
    U16 = rs.normal(size=(16, 25000))
    Y16 = eng.ld_matvec(0, U16)
    eng.set_mfma_min(0)
    for j in (0, 7, 15):
        assert maxrel(Y16[j], eng.ld_matvec(0, U16[j:j + 1])[0]) < 1e-12
    eng.set_mfma_min(3)
    # the same block stored dense gives the same products
    B = eng.get_ld_block(0, 0)
    eng.close()
    np.testing.assert_array_equal(B, B.T)
    eng2 = Engine(sizes, K=1)
    eng2.set_ld_packing(False)
    eng2.set_ld_block(0, 0, B)
    assert eng2.ld_block_format(0, 0) == 0
    Y2 = eng2.ld_matvec(0, U)
    for j in range(3):
        assert maxrel(Y2[j], Y[j]) < 1e-12
    eng2.close()


def test_north_star_full_size_pass_properties():
    """The north-star LD (M = 1e6 in 64 blocks of 15,625, 63.5 GB packed) through
    the bench's 8-column MFMA pass: symmetry u^T(Rv) = v^T(Ru) and linearity over
    all of M, two columns against the one-column VALU pass, and the first and
    last blocks against numpy on the blocks read back."""
    sizes = [15625] * 64
    M = sum(sizes)
    eng = Engine(sizes, K=1)
    eng.synth_ld_g(0, 7, 2000, np.zeros(M))
    assert eng.ld_block_format(0, 0) == 1
    rs = np.random.RandomState(3)
    U = rs.normal(size=(8, M))
    U[7] = 0.3 * U[0] - 1.7 * U[1]
    Y = eng.ld_matvec(0, U)
    for i, j in ((0, 1), (2, 5), (3, 6)):
        assert abs(U[i] @ Y[j] - U[j] @ Y[i]) <= 1e-11 * abs(U[i] @ Y[j])
    assert maxrel(Y[7], 0.3 * Y[0] - 1.7 * Y[1]) < 1e-11
    eng.set_mfma_min(0)
    for j in (0, 6):
        assert maxrel(Y[j], eng.ld_matvec(0, U[j:j + 1])[0]) < 1e-12
    eng.set_mfma_min(3)
    for b in (0, 63):
        B = eng.get_ld_block(0, b)
        np.testing.assert_array_equal(B, B.T)
        sl = slice(b * 15625, (b + 1) * 15625)
        ref = U[:, sl] @ B                     # B symmetric: rows of (B U^T)^T
        del B
        assert maxrel(Y[:, sl], ref) < 1e-11
    eng.close()


def test_north_star_full_size_rerun_bitwise(tmp_path):
    """The bench's north-star problem (M = 1e6 in 64 blocks of 15,625, K = 4
    sharing the LD, N = 10,000, EM) for 3 iterations, twice on one engine: the
    second infer() restarts (r1 = r, xhat2 = Sigma2_u = 0, the probe streams
    from their seeds) and, with lam/omegas set back, reproduces the first run
    bit for bit, CG and EM counts included; the trajectory stays finite."""
    sizes = [15625] * 64
    K, N = 4, 10000
    M = sum(sizes)
    rs = np.random.RandomState(2025)
    cm = M // 2
    beta = np.zeros(M)
    beta[rs.choice(M, cm, replace=False)] = rs.normal(0, np.sqrt(0.8 / cm), cm)
    eng = Engine(sizes, K=K)
    g = eng.synth_ld_g(0, 2026, N, beta).sum(axis=0)
    for k in range(K):
        eng.synth_r(k, 2026, N, g + np.random.RandomState(3025 + k).normal(0, np.sqrt(0.2), N))
    v = VAMP(N=[N] * K, Nt=N * K, M=M, K=K, rho=0.5, gamw=5.0, gam1=1e-6, a=[1 / K] * K,
             prior_vars=[0.0, 0.8 / cm / K], prior_probs=[0.5, 0.5], out_dir=str(tmp_path),
             out_name="ns", seed=7, write_files=False)
    x0 = beta * np.sqrt(N)
    v.attach_engine(eng, x0=x0)
    lam0, om0 = v.lam, np.array(v.omegas, dtype=np.float64).copy()
    its = 3
    xa = [x.copy() for x in v.infer(None, None, its, x0=x0, lmmse_damp=False, prior_update="em")]
    ha = [(h["cg_iters"], h.get("em_steps")) for h in v.history]
    v.lam, v.omegas = lam0, om0.copy()
    xb = v.infer(None, None, its, x0=x0, lmmse_damp=False, prior_update="em")
    hb_ = [(h["cg_iters"], h.get("em_steps")) for h in v.history[its:]]   # history accumulates
    assert ha == hb_
    for it in range(its):
        assert np.isfinite(xa[it]).all()
        np.testing.assert_array_equal(xa[it], xb[it])
    eng.close()


# ---------------------------------------------------------------------------
# CG (operator seam con_grad)
# ---------------------------------------------------------------------------
def test_cg_solve_vs_oracle():
    sizes = [150, 90, 260]
    blocks = rand_blocks(sizes, 11, nsamp=100)   # rank-deficient blocks, like simulated LD
    M = sum(sizes)
    eng = Engine(sizes, K=1)
    for b, B in enumerate(blocks):
        eng.set_ld_block(0, b, B)
    eng.set_ridge(0.05)
    L = vo.BlockLD(blocks, s=0.05)
    rs = np.random.RandomState(2)
    c1 = np.array([4.0, 2.0, 1.0, 6.0])
    c2 = np.array([0.3, 0.05, 1.0, 0.0])
    Bm = rs.normal(size=(4, M))
    X0 = np.zeros((4, M))
    X0[1] = rs.normal(size=M) * 0.1
    X0[3] = rs.normal(size=M) * 0.01
    X, it, info = eng.cg_solve(0, c1, c2, Bm, X0, maxiter=500)
    for j in range(4):
        A = lambda p, j=j: c1[j] * L.matvec_Rs(p) + c2[j] * p
        xr, info_r, it_r, _ = vo.cg_scipy(A, Bm[j], X0[j], 500, vo.Reducer())
        res = np.linalg.norm(Bm[j] - A(X[j])) / np.linalg.norm(Bm[j])
        assert res < 1e-5
        if c2[j] > 0:
            assert (it[j], info[j]) == (it_r, info_r), j
            assert maxrel(X[j], xr) < 1e-7, j      # CG amplifies summation-order rounding
        else:
            # A = c1 (0.95 R + 0.05 I) with rank-deficient R: ~60 iterations, so the
            # stop test can flip by one iteration on summation-order rounding
            assert info[j] == info_r == 0 and abs(int(it[j]) - it_r) <= 2, (it[j], it_r)
    # maxiter exhaustion and a zero right-hand side
    X, it, info = eng.cg_solve(0, c1[:2], c2[:2], np.stack([Bm[0], np.zeros(M)]),
                               np.stack([np.zeros(M), np.ones(M)]), maxiter=2)
    assert (it[0], info[0]) == (2, 2)
    assert (it[1], info[1]) == (0, 0) and not X[1].any()
    eng.close()


def test_cg_solve_without_shift_exact_counts():
    """c2 = 0 columns (A = c1 R_s, no gam2 shift) on full-rank blocks (N > n_b):
    a few tens of iterations, iteration counts and info exact, x within 1e-7 --
    the +-2 of test_cg_solve_vs_oracle is only for the rank-deficient ~60-
    iteration column, whose stop test sits on summation-order rounding."""
    sizes = [150, 90, 260]
    blocks = rand_blocks(sizes, 12, nsamp=1200)
    M = sum(sizes)
    eng = Engine(sizes, K=1)
    for b, B in enumerate(blocks):
        eng.set_ld_block(0, b, B)
    eng.set_ridge(0.05)
    L = vo.BlockLD(blocks, s=0.05)
    rs = np.random.RandomState(4)
    c1 = np.array([1.0, 6.0, 0.5])
    c2 = np.zeros(3)
    Bm = rs.normal(size=(3, M))
    X0 = np.zeros((3, M))
    X0[2] = rs.normal(size=M) * 0.05
    X, it, info = eng.cg_solve(0, c1, c2, Bm, X0, maxiter=500)
    for j in range(3):
        A = lambda p, j=j: c1[j] * L.matvec_Rs(p)
        xr, info_r, it_r, _ = vo.cg_scipy(A, Bm[j], X0[j], 500, vo.Reducer())
        assert (it[j], info[j]) == (it_r, info_r), (j, it[j], it_r)
        assert maxrel(X[j], xr) < 1e-7, j
    eng.close()


# ---------------------------------------------------------------------------
# element-wise kernels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K,nslab", [(1, 1), (3, 3), (8, 8)])
def test_denoise_and_em_vs_oracle(K, nslab):
    sizes = [4000, 3000, 5000]
    M = sum(sizes)
    rs = np.random.RandomState(K * 10 + nslab)
    r1s = rs.normal(scale=3.0, size=(K, M)) * (rs.uniform(size=(K, M)) < 0.3)
    gam1s = rs.uniform(0.5, 3.0, size=K)
    a = rs.uniform(1, 2, size=K)
    a /= a.sum()
    sigmas = np.sort(rs.uniform(1, 50, size=nslab))
    omegas = rs.uniform(0.5, 1, size=nslab)
    omegas /= omegas.sum()
    lam = 0.12
    eng = Engine(sizes, K=K)
    for k in range(K):
        eng.set_vector(hb.VEC_R1, k, r1s[k])
    der = eng.denoise(gam1s, a, lam, omegas, sigmas, rho=0.5, damp=False)
    x = eng.get_vector(hb.VEC_XHAT1)
    assert maxrel(x, vo.denoiser_meta(r1s, gam1s, a, lam, omegas, sigmas)) < 1e-12
    ref_der = vo.der_denoiser_meta(r1s, gam1s, a, lam, omegas, sigmas).sum(axis=1)
    assert maxrel(der, ref_der) < 1e-11
    # damping (:275-276)
    eng.denoise(gam1s * 1.1, a, lam, omegas, sigmas, rho=0.5, damp=True)
    x2 = eng.get_vector(hb.VEC_XHAT1)
    ref2 = 0.5 * vo.denoiser_meta(r1s, gam1s * 1.1, a, lam, omegas, sigmas) + 0.5 * x
    assert maxrel(x2, ref2) < 1e-12
    # one EM step == oracle prior_update_em
    lam_g, om_g, steps, _ = eng.em(gam1s, a, sigmas, 1, lam, omegas)
    lam_r, om_r = vo.prior_update_em(r1s, gam1s, a, lam, omegas, sigmas)
    assert steps == 1
    assert abs(lam_g - lam_r) <= 1e-12 * abs(lam_r)
    assert maxrel(om_g, om_r) < 1e-12
    eng.close()


# ---------------------------------------------------------------------------
# full VAMP vs the reference's golden outputs
# ---------------------------------------------------------------------------
def run_vamp_case(c, out_dir, device=None, ld_packing=True, mfma_min=None, rs_recurrence=None):
    f = c.flags
    lds = [BlockLD(blocks, s=f["s"]) for blocks in c.ld_blocks]
    R = lds[0] if len(lds) == 1 else [lds[c.ld_of[k]] for k in range(c.K)]
    Nt = sum(c.N)
    a = np.array(c.N) / Nt
    v = VAMP(N=c.N, Nt=Nt, M=c.M, K=c.K, rho=f["rho"], gamw=f["gamw"], gam1=f["gam1"], a=a,
             prior_vars=f["prior_vars"], prior_probs=f["prior_probs"], out_dir=str(out_dir),
             out_name=c.name, seed=f["seed"], device=device, ld_packing=ld_packing,
             mfma_min=mfma_min, rs_recurrence=rs_recurrence)
    xh = v.infer(R, c.r, f["iterations"], x0=c.x0, cg_maxit=f["cg_maxit"],
                 em_prior_maxit=f["em_prior_maxit"], learn_gamw=f["learn_gamw"],
                 lmmse_damp=f["lmmse_damp"], prior_update=f["prior_update"],
                 update_prior_from=f["update_prior_from"])
    return v, xh


def read_tsv(path):
    with open(path) as fh:
        text = fh.read()
    rows = [[float(x) for x in ln.split("\t")] for ln in text.splitlines()[1:]]
    return text, np.array(rows)


@pytest.mark.parametrize("packing", [True, False, "valu", "direct", "hostcg"])
@pytest.mark.parametrize("name", case_names())
def test_vamp_matches_reference_golden(name, packing, tmp_path, monkeypatch):
    """packing True: packed storage (MFMA pass for K >= 2, i.e. >= 3 CG columns),
    R_s x carried through the CG (default); "valu": packed storage, VALU pass
    only; False: dense storage; "direct": R_s xhat2 / R_s Sigma2_u by a separate
    LD pass, as the reference computes them (src/sgvamp.py:352,359); "hostcg":
    the CG's stop test on the host every iteration instead of the pipelined
    device-side control (SGV_CG_PIPE=0)."""
    c = Case(name)
    if packing == "hostcg":
        monkeypatch.setenv("SGV_AB", "1")
        monkeypatch.setenv("SGV_CG_PIPE", "0")
    if packing == "valu" and c.K == 1:
        pytest.skip("K = 1 never reaches 3 columns: same as packing=True")
    v, xh = run_vamp_case(c, tmp_path, ld_packing=bool(packing),
                          mfma_min=0 if packing == "valu" else None,
                          rs_recurrence=False if packing == "direct" else None)
    fmts = {v.engine.ld_block_format(l, b) for l in range(v.engine.nld)
            for b in range(len(v.engine.block_sizes))}
    assert fmts == {1 if packing else 0}
    its = c.flags["iterations"]
    Nt = sum(c.N)
    for it in range(its):
        xb = np.fromfile(tmp_path / ("%s_xhat_it_%d.bin" % (name, it)), dtype=np.float64)
        assert xb.shape == (c.M,)
        assert maxrel(xb, c.xhat[it]) < 1e-8, (it, maxrel(xb, c.xhat[it]))
        assert maxrel(xh[it].ravel() / np.sqrt(Nt), c.xhat[it]) < 1e-8
        for k in range(c.K):
            rb = np.fromfile(tmp_path / ("%s_r1_cohort_%d_it_%d.bin" % (name, k + 1, it)))
            assert maxrel(rb, c.r1[k][it]) < 1e-8, (it, k)
    cg = np.array([h["cg_iters"] for h in v.history]).transpose(1, 0, 2)
    np.testing.assert_array_equal(cg, c.cg_iters)
    info = np.array([h["cg_info"] for h in v.history]).transpose(1, 0, 2)
    np.testing.assert_array_equal(info, c.cg_info)
    em = [h["em_steps"] for h in v.history if "em_steps" in h]
    assert em == list(c.em_steps)
    assert [h["mle_warning"] for h in v.history if "mle_warning" in h] == c.warnings
    for k in range(c.K):
        text, rows = read_tsv(tmp_path / ("%s_cohort_%d.csv" % (name, k + 1)))
        assert text.splitlines()[0] == c.cohort_csv_text[k].splitlines()[0]
        np.testing.assert_allclose(rows, c.cohort_csv[k], rtol=1e-5, atol=0)
        # row 0 is written before any EM update: lam prints exactly as the reference's
        assert text.splitlines()[1].split("\t")[-1] == c.cohort_csv_text[k].splitlines()[1].split("\t")[-1]
    text, rows = read_tsv(tmp_path / ("%s_metrics.csv" % name))
    assert text.splitlines()[0] == c.metrics_csv_text.splitlines()[0]
    np.testing.assert_allclose(rows, c.metrics_csv, rtol=1e-7, atol=1e-12)
    v.engine.close()


@pytest.mark.parametrize("name", ["k1_defaults", "k1_L3", "k1_blocks_csr_s_damp", "k2_shared",
                                  "k4_shared_s_damp"])
def test_cg_pipeline_matches_host_loop(name, tmp_path, monkeypatch):
    """Pipelined CG (device-side stop test/beta, next iteration enqueued ahead)
    and device EM loop (k_em_ctl) vs the host-tested loops: identical CG and EM
    step counts; at K = 1 (VALU passes, whose per-column sums do not depend on
    the column count) bitwise identical trajectories and CSV files."""
    c = Case(name)
    out = {}
    monkeypatch.setenv("SGV_AB", "1")
    for mode in ("0", "1"):
        monkeypatch.setenv("SGV_CG_PIPE", mode)
        d = tmp_path / mode
        d.mkdir()
        v, xh = run_vamp_case(c, d)
        out[mode] = (v, xh, [h["cg_iters"] for h in v.history], [h["cg_info"] for h in v.history],
                     [h.get("em_steps") for h in v.history],
                     [(d / ("%s_cohort_%d.csv" % (name, k + 1))).read_text() for k in range(c.K)])
        v.engine.close()
    assert out["0"][2] == out["1"][2] and out["0"][3] == out["1"][3]
    assert out["0"][4] == out["1"][4]
    if c.K == 1:
        assert out["0"][5] == out["1"][5]
    for a_, b_ in zip(out["0"][1], out["1"][1]):
        if c.K == 1:
            np.testing.assert_array_equal(a_, b_)
        else:
            assert maxrel(b_, a_) < 1e-10


@pytest.mark.parametrize("name", ["k1_defaults", "k2_shared", "k4_shared_s_damp", "k4_long50"])
def test_cg_exact_columns_vs_lookahead(name, tmp_path, monkeypatch):
    """Pipelined CG with exact column sets (default: each pass carries only the
    columns still active after its own stop test) vs the one-iteration look-ahead
    form (SGV_CG_EXACT=0: a column that stops at that test rides along): the
    same CG and EM counts and iterates equal to rounding (bitwise where no pass
    changes kernel family); the default path's match with the reference fixtures
    is test_vamp_matches_reference_golden's."""
    c = Case(name)
    monkeypatch.setenv("SGV_AB", "1")
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("SGV_CG_EXACT", mode)
        d = tmp_path / mode
        d.mkdir()
        v, xh = run_vamp_case(c, d)
        out[mode] = (xh, [h["cg_iters"] for h in v.history], [h["cg_info"] for h in v.history],
                     [h.get("em_steps") for h in v.history])
        v.engine.close()
    assert out["0"][1] == out["1"][1] and out["0"][2] == out["1"][2]
    assert out["0"][3] == out["1"][3]
    worst = max(maxrel(b_, a_) for a_, b_ in zip(out["0"][0], out["1"][0]))
    print("%s: exact vs look-ahead max rel %.3g" % (name, worst))
    assert worst < 1e-10


@pytest.mark.parametrize("name", ["k1_defaults", "k1_L3", "k2_shared", "k4_shared_s_damp",
                                  "k1_mle", "k2_mle_L3", "k1_blocks_csr_s_damp"])
def test_step_driver_matches_phases(name, tmp_path, monkeypatch):
    """VAMP.step through sgv_step on the library's worker thread -- chained (the
    next step queued behind the running one, its scalars taken from it on the
    device side; MLE prior updates too, inside the step: SGV_STEP_MLE) and
    unchained -- against one host call per phase (SGV_STEP=phases): every output
    file byte-identical, same CG/EM counts and MLE outcomes."""
    c = Case(name)
    res = {}
    monkeypatch.setenv("SGV_AB", "1")
    for mode in ("phases", "nochain", ""):
        monkeypatch.setenv("SGV_STEP", mode)
        d = tmp_path / (mode or "chain")
        d.mkdir()
        v, xh = run_vamp_case(c, d)
        files = sorted(p.name for p in d.iterdir())
        res[mode] = ({f: (d / f).read_bytes() for f in files},
                     [(h["cg_iters"], h["cg_info"], h.get("em_steps"), h.get("mle_warning"))
                      for h in v.history],
                     [np.asarray(x) for x in xh])
        v.engine.close()
    ref = res["phases"]
    assert len(ref[0]) >= c.flags["iterations"]
    for mode in ("nochain", ""):
        assert res[mode][0].keys() == ref[0].keys()
        for f, b in ref[0].items():
            assert res[mode][0][f] == b, (mode, f)
        assert res[mode][1] == ref[1]
        for a_, b_ in zip(res[mode][2], ref[2]):
            np.testing.assert_array_equal(a_, b_)


def test_mle_gam_carries_over_infer_calls(tmp_path, monkeypatch):
    """Two infer() calls on one VAMP object, the second with a different R (a new
    engine), MLE prior from iteration 1: the MLE step chained behind iteration 0
    starts fsolve from the gam the first call left on the object, as the
    reference's self.gam does (src/sgvamp.py:175-178,194) -- chained, unchained
    and per-phase runs write byte-identical files and take the same MLE
    outcomes (the chained step started from x0[-1] = 1)."""
    c = Case("k1_mle")
    f = c.flags
    monkeypatch.setenv("SGV_AB", "1")
    res = {}
    for mode in ("phases", "nochain", ""):
        monkeypatch.setenv("SGV_STEP", mode)
        d = tmp_path / (mode or "chain")
        d.mkdir()
        v, _ = run_vamp_case(c, d)
        gam_first = v.gam
        # the same LD as a new object: _restart builds a new engine
        R2 = BlockLD(c.ld_blocks[0], s=f["s"])
        v.setup_io(str(d), c.name + "_2")
        v.infer(R2, c.r, f["iterations"], x0=c.x0, cg_maxit=f["cg_maxit"],
                em_prior_maxit=f["em_prior_maxit"], learn_gamw=f["learn_gamw"],
                lmmse_damp=f["lmmse_damp"], prior_update="mle", update_prior_from=1)
        files = sorted(p.name for p in d.iterdir())
        res[mode] = ({p: (d / p).read_bytes() for p in files}, gam_first, v.gam,
                     [(h.get("mle_warning"), h["cg_iters"]) for h in v.history])
        v.engine.close()
    assert res["phases"][1] is not None, "the first run's MLE must converge for this test"
    for mode in ("nochain", ""):
        assert res[mode][0].keys() == res["phases"][0].keys()
        for p, b in res["phases"][0].items():
            assert res[mode][0][p] == b, (mode, p)
        assert res[mode][1:] == res["phases"][1:], mode


def test_vamp_is_deterministic(tmp_path):
    c = Case("k2_shared")
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    v1, x1 = run_vamp_case(c, tmp_path / "a")
    v2, x2 = run_vamp_case(c, tmp_path / "b")
    for a_, b_ in zip(x1, x2):
        np.testing.assert_array_equal(a_, b_)
    for k in range(c.K):
        f = "%s_cohort_%d.csv" % (c.name, k + 1)
        assert (tmp_path / "a" / f).read_text() == (tmp_path / "b" / f).read_text()
    v1.engine.close()
    v2.engine.close()


# ---------------------------------------------------------------------------
# synthetic generator vs its CPU restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [True, False])
def test_synth_generator_vs_oracle(packed):
    sizes = [50, 130, 257, 700]
    nsamp = 500
    M = sum(sizes)
    rs = np.random.RandomState(9)
    beta = np.zeros(M)
    idx = rs.choice(M, 40, replace=False)
    beta[idx] = rs.normal(0, 0.1, 40)
    w = rs.normal(0, 0.5, nsamp)
    Rb, r, g, gb = so.synth_problem(sizes, nsamp, beta, 77, w)
    eng = Engine(sizes, K=1)
    eng.set_ld_packing(packed)
    g_dev = eng.synth_ld_g(0, 77, nsamp, beta)
    assert {eng.ld_block_format(0, b) for b in range(len(sizes))} == {1 if packed else 0}
    for b in range(len(sizes)):
        assert maxrel(g_dev[b], gb[b]) < 1e-12
        Rd = eng.get_ld_block(0, b)
        assert maxrel(Rd, Rb[b]) < 1e-12
        np.testing.assert_array_equal(Rd, Rd.T)                  # mirrored tiles
        np.testing.assert_allclose(np.diag(Rd), 1.0, rtol=1e-12)  # standardised markers
    y = g_dev.sum(axis=0) + w
    eng.synth_r(0, 77, nsamp, y)
    assert maxrel(eng.get_vector(hb.VEC_R, 0), r) < 1e-12
    eng.close()


# ---------------------------------------------------------------------------
# medium scale: HIP VAMP vs oracle on device-generated data
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rs", [True, False])
@pytest.mark.parametrize("prior", ["matched", "cli_default"])
def test_vamp_medium_scale_vs_oracle(prior, rs, tmp_path):
    """Rank-deficient blocks (n_b > N) like C2.  With the CLI default prior
    (slab variance 1*Nt, far above the simulated effect size) the trajectory
    degenerates; the oracle does the same, step for step.  rs: R_s x carried
    through the CG (oracle cg_track) or by direct products."""
    sizes = [3000, 2500, 3500, 3000]
    nsamp = 2000
    M = sum(sizes)
    rs = np.random.RandomState(5)
    cm = M // 10
    beta = np.zeros(M)
    beta[rs.choice(M, cm, replace=False)] = rs.normal(0, np.sqrt(0.8 / cm), cm)
    eng = Engine(sizes, K=1)
    g = eng.synth_ld_g(0, 123, nsamp, beta)
    y = g.sum(axis=0) + rs.normal(0, np.sqrt(0.2), nsamp)
    eng.synth_r(0, 123, nsamp, y)
    blocks = [eng.get_ld_block(0, b) for b in range(len(sizes))]
    r = eng.get_vector(hb.VEC_R, 0)
    prior_vars = [0.0, 0.8 / cm] if prior == "matched" else [0.0, 1.0]
    prior_probs = [0.9, 0.1] if prior == "matched" else [0.99, 0.01]
    x0 = beta * np.sqrt(nsamp)
    v = VAMP(N=nsamp, Nt=nsamp, M=M, K=1, rho=0.5, gamw=5.0, gam1=1e-6, a=[1.0],
             prior_vars=prior_vars, prior_probs=prior_probs, out_dir=str(tmp_path), out_name="m",
             seed=3, write_files=False)
    v.attach_engine(eng, x0=x0)
    eng.set_rs_recurrence(rs)
    its = 6
    xh = v.infer(None, None, its, x0=x0, lmmse_damp=False, prior_update="em")
    L = vo.BlockLD(blocks)
    t = vo.infer([L], [0], [r], [nsamp], its, rho=0.5, gamw=5.0, gam1=1e-6,
                 prior_vars=prior_vars, prior_probs=prior_probs, x0=x0, seed=3,
                 lmmse_damp=False, reducer=vo.Reducer("blocked", bounds=L.bounds),
                 rs_recurrence=rs)
    for it in range(its):
        ref = np.asarray(t["xhat"][it])
        got = xh[it].ravel() / np.sqrt(nsamp)
        if np.isnan(ref).any():
            assert np.array_equal(np.isnan(ref), np.isnan(got)), it
            continue
        assert maxrel(got, ref) < 1e-8, it
    assert [h["cg_iters"][0] for h in v.history] == [list(x[0]) for x in t["cg_iters"]]
    assert [h.get("em_steps") for h in v.history][1:] == list(t["em_steps"])
    eng.close()


@pytest.mark.parametrize("K,ridge,damp", [(4, 0.05, True), (8, 0.05, True), (4, 0.0, False),
                                          (8, 0.0, False), (12, 0.05, True), (17, 0.0, False)])
def test_vamp_medium_scale_shared_ld_vs_oracle(K, ridge, damp, tmp_path):
    """C3/C5-like: K cohorts sharing one LD (2K CG columns -> the f64 MFMA passes
    over multi-panel, multi-chunk blocks: 4x4x4 groups, 16x16x4 at 13..16
    columns), ridge s and LMMSE damping on, R_s x carried through the CG; vs the
    oracle with the same algebra (cg_track).  With s = 0 the blocks are rank
    deficient (n_b > N): 5-9 CG iterations, columns stopping at different
    iterations, so one solve walks through several column counts / kernels.
    K = 12 / 17: more than 8 cohorts -- the LMMSE runs them in groups of 8
    (16 CG columns per pass), then 4 / 8 + 1."""
    sizes = [1300, 700, 1100]
    nsamp = 900
    M = sum(sizes)
    rs = np.random.RandomState(8)
    cm = M // 10
    beta = np.zeros(M)
    beta[rs.choice(M, cm, replace=False)] = rs.normal(0, np.sqrt(0.8 / cm), cm)
    eng = Engine(sizes, K=K)
    g = eng.synth_ld_g(0, 77, nsamp, beta).sum(axis=0)
    rvec = []
    for k in range(K):
        y = g + np.random.RandomState(100 + k).normal(0, np.sqrt(0.2), nsamp)
        eng.synth_r(k, 77, nsamp, y)
        rvec.append(eng.get_vector(hb.VEC_R, k).copy())
    blocks = [eng.get_ld_block(0, b) for b in range(len(sizes))]
    assert {eng.ld_block_format(0, b) for b in range(len(sizes))} == {1}
    N = [float(nsamp)] * K
    prior = dict(prior_vars=[0.0, 0.8 / cm / K], prior_probs=[0.9, 0.1])
    v = VAMP(N=N, Nt=sum(N), M=M, K=K, rho=0.5, gamw=5.0, gam1=1e-6, a=[1 / K] * K,
             out_dir=str(tmp_path), out_name="kk", seed=5, write_files=False, **prior)
    v.attach_engine(eng, x0=beta * np.sqrt(nsamp))
    eng.set_ridge(ridge)
    its = 6
    xh = v.infer(None, None, its, x0=beta * np.sqrt(nsamp), lmmse_damp=damp, prior_update="em")
    L = vo.BlockLD(blocks, s=ridge)
    t = vo.infer([L], [0] * K, rvec, N, its, rho=0.5, gamw=5.0, gam1=1e-6, x0=beta * np.sqrt(nsamp),
                 seed=5, lmmse_damp=damp, reducer=vo.Reducer("blocked", bounds=L.bounds),
                 rs_recurrence=True, **prior)
    for it in range(its):
        assert maxrel(xh[it].ravel() / np.sqrt(sum(N)), np.asarray(t["xhat"][it])) < 1e-8, it
    assert [h["cg_iters"] for h in v.history] == [[list(c) for c in x] for x in t["cg_iters"]]
    assert [h.get("em_steps") for h in v.history][1:] == list(t["em_steps"])
    eng.close()


@pytest.mark.parametrize("K", [1, 4])
def test_vamp_50_iterations_vs_oracle(K, tmp_path):
    """The north-star accuracy bar (BASELINE.json): xhat within 1e-5 relative of
    the reference algorithm after 50 iterations.  K = 4 cohorts share one LD, so
    the CG runs 8 columns through the f64 MFMA pass; K = 1 uses the VALU pass.
    EM prior learning, the R_s x recurrence and LMMSE damping are on, as in a
    production run.  Oracle: oracle/vamp_oracle.py (pinned to the reference's
    golden fixtures by tests/test_oracle_golden.py)."""
    tol = 1e-5                       # north_star: "<= 1e-5 rel error vs reference xhat"
    sizes = [1300, 700, 1100]
    nsamp = 900
    M = sum(sizes)
    rs = np.random.RandomState(21)
    cm = M // 10
    beta = np.zeros(M)
    beta[rs.choice(M, cm, replace=False)] = rs.normal(0, np.sqrt(0.8 / cm), cm)
    eng = Engine(sizes, K=K)
    g = eng.synth_ld_g(0, 91, nsamp, beta).sum(axis=0)
    rvec = []
    for k in range(K):
        y = g + np.random.RandomState(200 + k).normal(0, np.sqrt(0.2), nsamp)
        eng.synth_r(k, 91, nsamp, y)
        rvec.append(eng.get_vector(hb.VEC_R, k).copy())
    blocks = [eng.get_ld_block(0, b) for b in range(len(sizes))]
    N = [float(nsamp)] * K
    prior = dict(prior_vars=[0.0, 0.8 / cm / K], prior_probs=[0.9, 0.1])
    ridge = 0.05
    v = VAMP(N=N, Nt=sum(N), M=M, K=K, rho=0.5, gamw=5.0, gam1=1e-6, a=[1 / K] * K,
             out_dir=str(tmp_path), out_name="n50", seed=9, write_files=False, **prior)
    x0 = beta * np.sqrt(nsamp)
    v.attach_engine(eng, x0=x0)
    eng.set_ridge(ridge)
    its = 50
    xh = v.infer(None, None, its, x0=x0, lmmse_damp=True, prior_update="em")
    L = vo.BlockLD(blocks, s=ridge)
    t = vo.infer([L], [0] * K, rvec, N, its, rho=0.5, gamw=5.0, gam1=1e-6, x0=x0, seed=9,
                 lmmse_damp=True, reducer=vo.Reducer("blocked", bounds=L.bounds),
                 rs_recurrence=True, **prior)
    worst = max(maxrel(xh[it].ravel() / np.sqrt(sum(N)), np.asarray(t["xhat"][it]))
                for it in range(its))
    final = maxrel(xh[-1].ravel() / np.sqrt(sum(N)), np.asarray(t["xhat"][-1]))
    print("K=%d: worst maxrel over 50 iterations %.3e, final %.3e" % (K, worst, final))
    assert worst < tol, worst
    assert final < tol, final
    eng.close()


@pytest.mark.parametrize("strip", [8])
@pytest.mark.parametrize("ncol", [4, 5, 8, 16])
def test_mfma_strips_vs_numpy(strip, ncol):
    """MFMA pass work items are strips of up to 8 panels of one parity sharing
    a 512-column chunk (sym_mfma.hip); a block of 40 panels (20 per parity:
    chunks of 8 + 8 + 4-panel strips), ragged and one-marker blocks."""
    sizes = [10000, 513, 2600, 1]
    blocks = rand_blocks(sizes, seed=strip + ncol, symmetric=True)
    eng = Engine(sizes, K=1)
    for b, B in enumerate(blocks):
        eng.set_ld_block(0, b, B)
    eng.set_ridge(0.1)
    V = np.random.RandomState(ncol).normal(size=(ncol, sum(sizes)))
    Y = eng.ld_matvec(0, V)
    L = vo.BlockLD(blocks, s=0.1)
    for j in range(ncol):
        assert maxrel(Y[j], L.matvec_Rs(V[j])) < 1e-12, j
    eng.close()


@pytest.mark.parametrize("strip", [8])
def test_mfma_pair_kernel_bitwise(strip, monkeypatch):
    """The wave-pair MFMA kernel (k_sym_mfma_pair: two waves per 128-column
    segment, the row chains handed from one to the other through LDS) gives
    products bitwise identical to the 4-wave kernel's for 3-8 columns -- which
    is what lets a plan pick either by its launch tail -- and both match numpy
    (both read Pk paired at 5-8 columns)."""
    monkeypatch.setenv("SGV_AB", "1")
    sizes = [5000, 513, 2600, 1, 4097]
    blocks = rand_blocks(sizes, seed=strip, symmetric=True)
    L = vo.BlockLD(blocks, s=0.1)
    out = {}
    for form in ("0", "1"):
        monkeypatch.setenv("SGV_MF_PAIR", form)
        eng = Engine(sizes, K=1)
        for b, B in enumerate(blocks):
            eng.set_ld_block(0, b, B)
        eng.set_ridge(0.1)
        out[form] = {}
        for ncol in range(3, 9):
            V = np.random.RandomState(ncol).normal(size=(ncol, sum(sizes)))
            assert eng.ld_pass_form(0, ncol).kind == ("pair" if form == "1" else "strip4"), (
                form, ncol, eng.ld_pass_form(0, ncol))
            out[form][ncol] = eng.ld_matvec(0, V)
        eng.close()
    for ncol in range(3, 9):
        np.testing.assert_array_equal(out["1"][ncol], out["0"][ncol])
        V = np.random.RandomState(ncol).normal(size=(ncol, sum(sizes)))
        for j in range(ncol):
            assert maxrel(out["1"][ncol][j], L.matvec_Rs(V[j])) < 1e-12, (ncol, j)


def _infer_again(v, c, out_dir):  # noqa: ARG001
    f = c.flags
    lds = [BlockLD(blocks, s=f["s"]) for blocks in c.ld_blocks]
    R = lds[0] if len(lds) == 1 else [lds[c.ld_of[k]] for k in range(c.K)]
    return v.infer(R, c.r, f["iterations"], x0=c.x0, cg_maxit=f["cg_maxit"],
                   em_prior_maxit=f["em_prior_maxit"], learn_gamw=f["learn_gamw"],
                   lmmse_damp=f["lmmse_damp"], prior_update=f["prior_update"],
                   update_prior_from=f["update_prior_from"])


@pytest.mark.parametrize("name", ["k1_noem_fixgamw", "k4_shared_s_damp"])
def test_second_infer_restarts(name, tmp_path):
    """A second infer() on the same VAMP object restarts from r1 = r, xhat2 = 0,
    Sigma2_u_prev = 0 (src/sgvamp.py:198-217); lam/omegas carry over as object
    attributes, as in the reference.  Without a prior update the second run
    matches the golden fixture again; with EM it equals a fresh object started
    from the first run's lam/omegas (the device state left by run 1 is gone)."""
    c = Case(name)
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    v, _ = run_vamp_case(c, tmp_path / "a")
    lam1, om1 = v.lam, np.array(v.omegas, dtype=np.float64).copy()
    v.setup_io(str(tmp_path / "b"), c.name)      # run 2's files in their own directory
    xh2 = _infer_again(v, c, tmp_path / "b")
    its = c.flags["iterations"]
    Nt = sum(c.N)
    if c.flags["prior_update"] in (None, "none"):
        for it in range(its):
            xb = np.fromfile(tmp_path / "b" / ("%s_xhat_it_%d.bin" % (name, it)))
            assert maxrel(xb, c.xhat[it]) < 1e-8, (it, maxrel(xb, c.xhat[it]))
            assert maxrel(xh2[it].ravel() / np.sqrt(Nt), c.xhat[it]) < 1e-8
    else:
        f = c.flags
        (tmp_path / "c").mkdir()
        lds = [BlockLD(blocks, s=f["s"]) for blocks in c.ld_blocks]
        R = lds[0] if len(lds) == 1 else [lds[c.ld_of[k]] for k in range(c.K)]
        a = np.array(c.N) / Nt
        w = VAMP(N=c.N, Nt=Nt, M=c.M, K=c.K, rho=f["rho"], gamw=f["gamw"], gam1=f["gam1"], a=a,
                 prior_vars=f["prior_vars"], prior_probs=f["prior_probs"],
                 out_dir=str(tmp_path / "c"), out_name=c.name, seed=f["seed"])
        w.lam, w.omegas = lam1, om1
        xh3 = w.infer(R, c.r, its, x0=c.x0, cg_maxit=f["cg_maxit"],
                      em_prior_maxit=f["em_prior_maxit"], learn_gamw=f["learn_gamw"],
                      lmmse_damp=f["lmmse_damp"], prior_update=f["prior_update"],
                      update_prior_from=f["update_prior_from"])
        for it in range(its):
            np.testing.assert_array_equal(xh2[it], xh3[it])
        w.engine.close()
    v.engine.close()


# ---------------------------------------------------------------------------
# non-block-diagonal (banded / windowed) LD: packed band storage
# ---------------------------------------------------------------------------
_BAND_CACHE = {}


def _band_matrix(parts, seed=0):
    """Block-diagonal matrix of banded blocks: parts = [(n, bw)] (bw None: a
    dense random block).  Cached: the parametrized tests share them."""
    import scipy.sparse

    key = (tuple(parts), seed)
    if key in _BAND_CACHE:
        return _BAND_CACHE[key]
    mats = []
    for i, (n, bw) in enumerate(parts):
        if bw is None:
            mats.append(scipy.sparse.csr_matrix(rand_blocks([n], seed=seed + i)[0]))
        else:
            mats.append(vo.banded_ld(n, bw, seed=seed + i))
    _BAND_CACHE[key] = scipy.sparse.block_diag(mats, format="csr")
    return _BAND_CACHE[key]


@pytest.mark.parametrize("parts", [[(5000, 300)], [(2100, 100), (700, None), (3000, 1000)],
                                   [(1030, 5), (4000, 40)], [(4000, 1200)], [(3000, 0), (2050, 1)]])
@pytest.mark.parametrize("ncol", [1, 2, 3, 5, 8, 13, 16])
@pytest.mark.parametrize("s", [0.0, 0.1])
@pytest.mark.parametrize("kern", ["packed", "packed_valu"])
def test_ld_matvec_band_vs_scipy(parts, ncol, s, kern):
    """Sparse symmetric LD uploaded as CSR (sgv_set_ld_block_csr): a block whose
    band is narrower than its triangle is stored as a packed band (format 2),
    otherwise as the packed triangle (1); the pass equals scipy's CSR mat-vec
    (the reference's operator, src/sgvamp.py:316) to 1e-12."""
    A = _band_matrix(parts, seed=3)
    L = BlockLD.from_csr(A, s=s)
    eng = Engine(L.block_sizes, K=1)
    eng.set_ridge(s)
    if kern == "packed_valu":
        eng.set_mfma_min(0)
    for b in range(len(L.block_sizes)):
        L.upload(eng, 0, b)
    if all(bw is None or bw >= 5 for _, bw in parts):   # one detected block per part
        assert L.block_sizes == [n for n, _ in parts]
        for b, (n, bw) in enumerate(parts):
            band = bw is not None and -(-(256 + bw) // 256) * 256 < n
            assert eng.ld_block_format(0, b) == (2 if band else 1), (b, n, bw)
    else:   # R = I splits into 1-marker blocks, merged into >= 128-marker blocks
        assert min(L.block_sizes[:-2]) >= 128 and L.block_sizes[-1] == 2050
        assert {eng.ld_block_format(0, b) for b in range(len(L.block_sizes))} <= {1, 2}
    rs = np.random.RandomState(ncol)
    V = rs.normal(size=(ncol, A.shape[0]))
    Y = eng.ld_matvec(0, V)
    ref = vo.CsrLD(A, s=s)
    for j in range(ncol):
        want = ref.matvec_Rs(V[j])
        assert maxrel(Y[j], want) < 1e-12, (j, maxrel(Y[j], want))
    eng.close()


def test_finalize_forms_bitwise(monkeypatch):
    """The strip finalize's two forms -- FIN_Q threads per panel row
    (k_sym_finalize_strip) and one thread per row holding the FIN_Q parts in
    registers (k_sym_finalize_strip1, the default for band plans at <= 8
    columns) -- add the same terms in the same order: products bitwise equal
    on a plan mixing dense and band blocks, 3..16 columns (the band VAMP tests
    run the default form end to end)."""
    monkeypatch.setenv("SGV_AB", "1")
    A = _band_matrix([(3000, 300), (1500, None), (2600, 40)], seed=5)
    L = BlockLD.from_csr(A, s=0.05)
    out = {}
    for form in ("1", "4"):
        monkeypatch.setenv("SGV_FIN_FORM", form)
        eng = Engine(L.block_sizes, K=1)
        eng.set_ridge(0.05)
        for b in range(len(L.block_sizes)):
            L.upload(eng, 0, b)
        assert {eng.ld_block_format(0, b) for b in range(len(L.block_sizes))} == {1, 2}
        # the triangle wide with the bands' strips behind it, or every block on 16x16x4
        for nc in (3, 5, 8, 11, 16):
            f = eng.ld_pass_form(0, nc)
            want = ("wide", "strip4") if nc <= 8 else ("strip16", "none")
            assert (f.kind, f.rest_kind, f.fin_form) == want + (int(form),), (form, nc, f)
        out[form] = [eng.ld_matvec(0, np.random.RandomState(nc).normal(size=(nc, A.shape[0])))
                     for nc in (3, 5, 8, 11, 16)]
        eng.close()
    ref = vo.CsrLD(A, s=0.05)
    for i, nc in enumerate((3, 5, 8, 11, 16)):
        np.testing.assert_array_equal(out["1"][i], out["4"][i])
        V = np.random.RandomState(nc).normal(size=(nc, A.shape[0]))
        assert maxrel(out["1"][i][nc - 1], ref.matvec_Rs(V[nc - 1])) < 1e-12


@pytest.mark.parametrize("ncol", [1, 2, 3, 8, 16])
def test_ld_matvec_coupled_pieces_vs_scipy(ncol):
    """One band block cut into coupled pieces (sgvamp.band_cuts / BlockLD.pieces,
    sgv_set_ld_coupling: the layout that lets ranks share one chromosome): the
    pieces' passes plus the corner couplings equal scipy's CSR mat-vec of the
    whole band (src/sgvamp.py:316) to 1e-12, on the VALU (1-2 columns) and MFMA
    passes."""
    from sgvamp import band_cuts

    A = vo.banded_ld(70000, 700, seed=5, taps=12)
    L = BlockLD.from_csr(A)
    cuts = band_cuts([L], L.block_sizes, piece=16384)
    assert [len(c) for c in cuts] == [4]
    P, cpl = L.pieces(cuts)
    assert sorted(cpl) == [0, 1, 2]
    eng = Engine(P.block_sizes, K=1)
    for b in range(len(P.block_sizes)):
        P.upload(eng, 0, b)
        assert eng.ld_block_format(0, b) == 2
    for gb, (nr, nc, C) in cpl.items():
        eng.set_ld_coupling(0, gb, nr, nc, C)
    V = np.random.RandomState(ncol).normal(size=(ncol, A.shape[0]))
    Y = eng.ld_matvec(0, V)
    for j in range(ncol):
        want = A @ V[j]
        assert maxrel(Y[j], want) < 1e-12, (j, maxrel(Y[j], want))
    eng.close()


@pytest.mark.parametrize("M,bw,piece,taps", [(33333, 1200, 5120, 7), (20001, 3, 4096, 2),
                                              (41000, 1024, 4096, 12)])
def test_coupled_pieces_ragged_vs_scipy(M, bw, piece, taps):
    """Coupled band pieces on awkward shapes: an odd M whose last piece is not a
    whole number of panels and a bandwidth just under piece / 4 (1,200 x 1,200
    corners), a 3-wide band (3 x 3 corners), and a bandwidth
    that is an exact panel multiple -- all against scipy's CSR mat-vec at 1, 3,
    8 and 16 columns."""
    from sgvamp import band_cuts

    A = vo.banded_ld(M, bw, seed=M % 97, taps=taps)
    L = BlockLD.from_csr(A)
    cuts = band_cuts([L], L.block_sizes, piece=piece)
    assert len(cuts[0]) >= 2, cuts
    P, cpl = L.pieces(cuts)
    eng = Engine(P.block_sizes, K=1)
    for b in range(len(P.block_sizes)):
        P.upload(eng, 0, b)
    for gb, (nr, nc, C) in cpl.items():
        eng.set_ld_coupling(0, gb, nr, nc, C)
    for ncol in (1, 3, 8, 16):
        V = np.random.RandomState(ncol).normal(size=(ncol, M))
        Y = eng.ld_matvec(0, V)
        for j in range(ncol):
            assert maxrel(Y[j], A @ V[j]) < 1e-12, (ncol, j)
    eng.close()


def test_coupling_widths_vs_scipy():
    """The corner-coupling sums of coupled band pieces (k_coupling_lds: 8 inner
    parts per 64 output rows, the source values staged through LDS) at 1..16
    columns and a bandwidth that leaves partial LDS chunks and unroll tails:
    every column of the pass against scipy's CSR product of the whole matrix."""
    from sgvamp import band_cuts

    A = vo.banded_ld(50000, 613, seed=7, taps=9)
    L = BlockLD.from_csr(A)
    cuts = band_cuts([L], L.block_sizes, piece=16384)
    P, cpl = L.pieces(cuts)
    assert len(cpl) >= 2
    eng = Engine(P.block_sizes, K=1)
    for b in range(len(P.block_sizes)):
        P.upload(eng, 0, b)
    for gb, (nr, nc, C) in cpl.items():
        eng.set_ld_coupling(0, gb, nr, nc, C)
    for nc in (1, 2, 5, 8, 16):
        V = np.random.RandomState(nc).normal(size=(nc, A.shape[0]))
        Y = eng.ld_matvec(0, V)
        for j in range(nc):
            assert maxrel(Y[j], A @ V[j]) < 1e-12, (nc, j)
    eng.close()


def test_band_block_roundtrip():
    """get_ld_block of a band block: the stored band, zeros outside it."""
    A = _band_matrix([(1500, 200)], seed=11)
    L = BlockLD.from_csr(A)
    eng = Engine(L.block_sizes, K=1)
    L.upload(eng, 0, 0)
    assert eng.ld_block_format(0, 0) == 2
    np.testing.assert_array_equal(eng.get_ld_block(0, 0), A.toarray())
    eng.close()


@pytest.mark.parametrize("K,s,damp,prior", [(1, 0.0, False, "em"), (1, 0.05, True, "em"),
                                             (4, 0.05, True, "em"), (8, 0.05, True, "em"),
                                             (2, 0.0, False, "mle")])
def test_vamp_band_ld_vs_oracle(K, s, damp, prior, tmp_path):
    """Whole VAMP iterations on one banded (not block-diagonal) LD matrix of
    8,000 markers, bw = 600 -- the shape the reference's .npz / PLINK .ld paths
    produce (src/main.py:199-200,251-257) -- against the oracle running scipy's
    CSR mat-vec on the same matrix: xhat <= 1e-8 relative, CG counts and EM
    steps exact.  K = 8: 16-column band passes (k_sym_mfma16); "mle": the MLE
    prior update (src/sgvamp.py:139-194) on band passes."""
    M, bw, N = 8000, 600, 5000
    A = vo.banded_ld(M, bw, seed=21)
    rs = np.random.RandomState(4)
    cm = M // 20
    beta = np.zeros(M)
    beta[rs.choice(M, cm, replace=False)] = rs.normal(0, np.sqrt(0.5 / cm), cm) * np.sqrt(N)
    r = [A @ beta + rs.normal(size=M) * np.sqrt(0.5) for _ in range(K)]
    Ns = [float(N)] * K
    Nt = sum(Ns)
    a = np.array(Ns) / Nt
    prior_vars, prior_probs = [0.0, 0.5 / cm], [0.95, 0.05]
    L = BlockLD.from_csr(A, s=s)
    v = VAMP(N=Ns, Nt=Nt, M=M, K=K, rho=0.5, gamw=2.0, gam1=1e-6, a=a, prior_vars=prior_vars,
             prior_probs=prior_probs, out_dir=str(tmp_path), out_name="band", seed=9,
             write_files=False)
    its = 6
    xh = v.infer(L, np.stack(r), its, x0=beta, lmmse_damp=damp, prior_update=prior)
    assert v.engine.ld_block_format(0, 0) == 2
    t = vo.infer([vo.CsrLD(A, s=s)], [0] * K, r, Ns, its, rho=0.5, gamw=2.0, gam1=1e-6,
                 prior_vars=prior_vars, prior_probs=prior_probs, x0=beta, seed=9,
                 lmmse_damp=damp, reducer=vo.Reducer("blocked", bounds=np.array([0, M])),
                 rs_recurrence=True, prior_update=prior)
    for it in range(its):
        ref = np.asarray(t["xhat"][it]).ravel()
        got = xh[it].ravel() / np.sqrt(Nt)
        assert maxrel(got, ref) < 1e-8, (it, maxrel(got, ref))
    assert [h["cg_iters"] for h in v.history] == [[list(c) for c in x] for x in t["cg_iters"]]
    if prior == "em":
        assert [h.get("em_steps") for h in v.history][1:] == list(t["em_steps"])
    v.engine.close()


@pytest.mark.parametrize("s,damp", [(0.0, False), (0.05, True)])
def test_vamp_distinct_band_pieces_vs_oracle(s, damp, tmp_path, monkeypatch):
    """Two cohorts each with its own windowed LD (the reference's
    ld_fpaths_list[rank] layout, src/main.py:173) over one chromosome of 60,000
    markers, bandwidths 400 and 700: both bands cut at the same 16,384-marker
    pieces, each piece with its own couplings per LD matrix -- whole VAMP
    iterations against the oracle running scipy's CSR mat-vec on each cohort's
    matrix: xhat <= 1e-8 relative, CG counts and EM steps exact."""
    import sgvamp

    monkeypatch.setattr(sgvamp, "BAND_PIECE", 16384)
    M, N, K = 60000, 5000, 2
    As = [vo.banded_ld(M, 400, seed=31, taps=10), vo.banded_ld(M, 700, seed=32, taps=10)]
    rs = np.random.RandomState(6)
    cm = M // 25
    beta = np.zeros(M)
    beta[rs.choice(M, cm, replace=False)] = rs.normal(0, np.sqrt(0.5 / cm), cm) * np.sqrt(N)
    r = [As[k] @ beta + rs.normal(size=M) * np.sqrt(0.5) for k in range(K)]
    Ns = [float(N)] * K
    Nt = sum(Ns)
    prior_vars, prior_probs = [0.0, 0.5 / cm], [0.95, 0.05]
    Ls = [BlockLD.from_csr(A, s=s) for A in As]
    v = VAMP(N=Ns, Nt=Nt, M=M, K=K, rho=0.5, gamw=2.0, gam1=1e-6, a=np.array(Ns) / Nt,
             prior_vars=prior_vars, prior_probs=prior_probs, out_dir=str(tmp_path),
             out_name="dband", seed=9, write_files=False)
    its = 5
    xh = v.infer(Ls, np.stack(r), its, x0=beta, lmmse_damp=damp, prior_update="em")
    pieces = list(v.engine.block_sizes)
    assert len(pieces) == 3 and v.engine.nld == 2
    assert {v.engine.ld_block_format(l, b) for l in range(2) for b in range(3)} == {2}
    v.engine.close()
    t = vo.infer([vo.CsrLD(A, s=s) for A in As], [0, 1], r, Ns, its, rho=0.5, gamw=2.0,
                 gam1=1e-6, prior_vars=prior_vars, prior_probs=prior_probs, x0=beta, seed=9,
                 lmmse_damp=damp, rs_recurrence=True,
                 reducer=vo.Reducer("blocked", bounds=np.concatenate([[0], np.cumsum(pieces)])))
    for it in range(its):
        ref = np.asarray(t["xhat"][it]).ravel()
        got = xh[it].ravel() / np.sqrt(Nt)
        assert maxrel(got, ref) < 1e-8, (it, maxrel(got, ref))
    assert [h["cg_iters"] for h in v.history] == [[list(c) for c in x] for x in t["cg_iters"]]
    assert [h.get("em_steps") for h in v.history][1:] == list(t["em_steps"])


@pytest.mark.parametrize("name", ["k1_long50", "k4_long50", "c1"])
def test_north_star_gate_vs_reference(name, tmp_path):
    """The north star's accuracy gate pinned to the reference itself: xhat
    within 1e-5 relative of the reference's after 50 iterations (K = 1 over
    three blocks, and K = 4 sharing one LD through the f64 MFMA pass; ridge,
    damping, EM), and the C1 configuration (M = 5,000, N = 10,000, one dense
    block, 20 iterations).  CG iteration counts and EM steps exact.  The
    observed error is printed."""
    c = Case(name)
    v, xh = run_vamp_case(c, tmp_path)
    its = c.flags["iterations"]
    Nt = sum(c.N)
    errs = [maxrel(xh[it].ravel() / np.sqrt(Nt), c.xhat[it]) for it in range(its)]
    print("%s: max rel xhat error over %d iterations %.3e (last %.3e)"
          % (name, its, max(errs), errs[-1]))
    assert max(errs) < 1e-5
    cg = np.array([h["cg_iters"] for h in v.history]).transpose(1, 0, 2)
    np.testing.assert_array_equal(cg, c.cg_iters)
    assert [h["em_steps"] for h in v.history if "em_steps" in h] == list(c.em_steps)
    v.engine.close()


def test_c5_shape_divergence_matches_oracle(tmp_path):
    """Why the C5 bench trajectory blows up (profiles/r01s6_c5_run.log): a
    reduced C5 -- K = 8 cohorts sharing one LD, s = 0.1, LMMSE damping, EM, the
    bench's prior (0.8/cm/K, probs 0.5/0.5), 50 % causal markers, the bench
    generator's data with n_b / N = 1.5625 (15,625 / 10,000) at one block of
    6,000 markers and N = 3,840 -- run by the HIP path and by the oracle on the
    same device-generated inputs.  The oracle (pinned to the reference) grows
    l2 from 0.9 to ~5e3 by iteration 8 with 1-iteration CG solves, so the
    divergence is the algorithm's (src/sgvamp.py:322-323 damps xhat2 only);
    HIP follows it step for step: CG and EM counts exact, l2 and xhat to 1e-8
    relative before the blow-up and within the north star's 1e-5 through it
    (observed 2.6e-7 at l2 = 5e3: rounding differences grow with the unstable
    mode)."""
    n, nsamp, K, s = 6000, 3840, 8, 0.1
    M = n
    rs = np.random.RandomState(2025)
    cm = M // 2
    beta = np.zeros(M)
    beta[rs.choice(M, cm, replace=False)] = rs.normal(0, np.sqrt(0.8 / cm), cm)
    eng = Engine([n], K=K)
    g = eng.synth_ld_g(0, 2026, nsamp, beta).sum(axis=0)
    rvec = []
    for k in range(K):
        y = g + np.random.RandomState(2025 + 1000 + k).normal(0.0, np.sqrt(0.2), nsamp)
        eng.synth_r(k, 2026, nsamp, y)
        rvec.append(eng.get_vector(hb.VEC_R, k).copy())
    blocks = [eng.get_ld_block(0, 0)]
    N = [float(nsamp)] * K
    prior = dict(prior_vars=[0.0, 0.8 / cm / K], prior_probs=[0.5, 0.5])
    x0 = beta * np.sqrt(nsamp)
    v = VAMP(N=N, Nt=sum(N), M=M, K=K, rho=0.5, gamw=5.0, gam1=1e-6, a=[1 / K] * K,
             out_dir=str(tmp_path), out_name="c5", seed=2025, write_files=False, **prior)
    v.attach_engine(eng, x0=x0)
    eng.set_ridge(s)
    its = 9
    xh = v.infer(None, None, its, x0=x0, lmmse_damp=True, prior_update="em")
    L = vo.BlockLD(blocks, s=s)
    t = vo.infer([L], [0] * K, rvec, N, its, rho=0.5, gamw=5.0, gam1=1e-6, x0=x0, seed=2025,
                 lmmse_damp=True, reducer=vo.Reducer("blocked", bounds=L.bounds),
                 rs_recurrence=True, **prior)
    l2 = [h["metrics"][1] for h in v.history]
    errs = [maxrel(xh[it].ravel() / np.sqrt(sum(N)), np.asarray(t["xhat"][it])) for it in range(its)]
    print("c5-shape l2 per iteration:", ["%.4g" % x for x in l2])
    print("c5-shape xhat rel error vs oracle:", ["%.2g" % e for e in errs])
    for it in range(its):
        # rounding differences grow with the unstable mode once l2 takes off:
        # 1e-8 before, the north star's 1e-5 bar during the blow-up
        assert errs[it] < (1e-8 if l2[it] < 1.5 else 1e-5), (it, errs[it])
    assert [h["cg_iters"] for h in v.history] == [[list(c) for c in x] for x in t["cg_iters"]]
    assert [h.get("em_steps") for h in v.history][1:] == list(t["em_steps"])
    for it, m in enumerate(t["metrics"]):
        assert abs(l2[it] - m[2]) <= (1e-8 if l2[it] < 1.5 else 1e-5) * abs(m[2]), it
    assert l2[-1] > 100 * l2[2]          # the blow-up is in both
    eng.close()


@pytest.mark.parametrize("K,nslab,gam", [(1, 1, None), (3, 2, 0.7), (12, 3, None), (40, 2, 1.3)])
def test_mle_update_matches_scipy_on_device_sums(K, nslab, gam):
    """sgv_mle_update (the whole MLE prior update in the library) against
    scipy.optimize.fsolve driven from Python on the same device sums
    (sgv_mle_exp_max / sgv_mle_terms), as the reference drives it
    (src/sgvamp.py:162-194): bitwise the same prior, the same outcome."""
    from scipy import optimize

    sizes = [700, 300]
    M = sum(sizes)
    rs = np.random.RandomState(K * 7 + nslab)
    eng = Engine(sizes, K=K)
    lam = 0.2
    for k in range(K):
        z = rs.rand(M) < lam
        eng.set_vector(hb.VEC_R1, k, np.where(z, rs.normal(0, 1.5, M), 0.0) + rs.normal(0, .4, M))
    gam1s = rs.uniform(3.0, 8.0, K)
    a = np.full(K, 1.0 / K)
    sig = np.sort(rs.uniform(0.5, 3.0, nslab))
    omegas = rs.dirichlet(np.ones(nslab))
    L = nslab + 1
    omega0 = np.concatenate([[1 - lam], lam * omegas])
    sigma2 = np.concatenate([[1e-16], sig])
    exp_max = eng.mle_exp_max(gam1s, sigma2)

    def lagrangian(x):                                  # src/sgvamp.py:139-160
        y = np.zeros(L + 1)
        y[:L] = eng.mle_terms(a, gam1s, sigma2, x[:L], exp_max) + (omega0 - 1) / x[:L] + x[L]
        y[L] = sum(x[:L]) - 1.0
        return y

    x0 = np.concatenate([omega0, [1.0 if gam is None else gam]])
    x, _, ier, _ = optimize.fsolve(lagrangian, x0, full_output=True)
    status, lam2, om2, gam2 = eng.mle_update(gam1s, a, sig, lam, omegas, gam)
    if ier != 1:
        assert status == hb.MLE_NOT_CONVERGED
    elif any(v <= 0 for v in x[:-1]):
        assert status == hb.MLE_NEGATIVE
    else:
        assert status == 0
        x[:-1] /= sum(x[:-1])                           # :190-193
        assert lam2 == 1 - x[0]
        np.testing.assert_array_equal(om2, [w / sum(x[1:-1]) for w in x[1:-1]])
        assert gam2 == x[L]
    eng.close()


def test_mle_prior_many_cohorts_vs_oracle(tmp_path):
    """--prior-update mle (src/sgvamp.py:139-194) with K = 10 cohorts (more than
    one LMMSE group; the MLE sums over all cohorts on the device, fsolve in the
    library) against the oracle on the same device-generated inputs."""
    sizes = [600, 500]
    nsamp, K = 700, 10
    M = sum(sizes)
    rs = np.random.RandomState(31)
    cm = M // 10
    beta = np.zeros(M)
    beta[rs.choice(M, cm, replace=False)] = rs.normal(0, np.sqrt(0.8 / cm), cm)
    eng = Engine(sizes, K=K)
    g = eng.synth_ld_g(0, 55, nsamp, beta).sum(axis=0)
    rvec = []
    for k in range(K):
        y = g + np.random.RandomState(300 + k).normal(0, np.sqrt(0.2), nsamp)
        eng.synth_r(k, 55, nsamp, y)
        rvec.append(eng.get_vector(hb.VEC_R, k).copy())
    blocks = [eng.get_ld_block(0, b) for b in range(len(sizes))]
    N = [float(nsamp)] * K
    prior = dict(prior_vars=[0.0, 0.8 / cm / K], prior_probs=[0.9, 0.1])
    x0 = beta * np.sqrt(nsamp)
    v = VAMP(N=N, Nt=sum(N), M=M, K=K, rho=0.5, gamw=5.0, gam1=1e-6, a=[1 / K] * K,
             out_dir=str(tmp_path), out_name="mle", seed=8, write_files=False, **prior)
    v.attach_engine(eng, x0=x0)
    its = 4
    xh = v.infer(None, None, its, x0=x0, lmmse_damp=False, prior_update="mle")
    L = vo.BlockLD(blocks)
    t = vo.infer([L], [0] * K, rvec, N, its, rho=0.5, gamw=5.0, gam1=1e-6, x0=x0, seed=8,
                 lmmse_damp=False, prior_update="mle",
                 reducer=vo.Reducer("blocked", bounds=L.bounds), rs_recurrence=True, **prior)
    for it in range(its):
        assert maxrel(xh[it].ravel() / np.sqrt(sum(N)), np.asarray(t["xhat"][it])) < 1e-8, it
    assert [h["cg_iters"] for h in v.history] == [[list(c) for c in x] for x in t["cg_iters"]]
    assert [h.get("mle_warning") for h in v.history if h.get("mle_warning")] == t["mle_warnings"]
    eng.close()


@pytest.mark.parametrize("K,update", [(40, "em"), (40, "mle"), (70, "em")])
def test_more_cohorts_than_one_launch_vs_oracle(K, update, tmp_path):
    """More than 32 cohorts (the marker kernels' per-launch bound): the denoiser,
    EM and MLE run in cohort groups of 32 (np.inner continued group to group,
    EM partials added group after group, MLE totals in group order), the LMMSE
    in groups of 8; against the oracle on the same device-generated inputs
    (src/main.py:62,90-93: the reference's K is its MPI world size)."""
    sizes = [600, 500]
    nsamp = 700
    M = sum(sizes)
    rs = np.random.RandomState(41)
    cm = M // 10
    beta = np.zeros(M)
    beta[rs.choice(M, cm, replace=False)] = rs.normal(0, np.sqrt(0.8 / cm), cm)
    eng = Engine(sizes, K=K)
    g = eng.synth_ld_g(0, 56, nsamp, beta).sum(axis=0)
    rvec = []
    for k in range(K):
        y = g + np.random.RandomState(400 + k).normal(0, np.sqrt(0.2), nsamp)
        eng.synth_r(k, 56, nsamp, y)
        rvec.append(eng.get_vector(hb.VEC_R, k).copy())
    blocks = [eng.get_ld_block(0, b) for b in range(len(sizes))]
    N = [float(nsamp)] * K
    prior = dict(prior_vars=[0.0, 0.8 / cm / K], prior_probs=[0.9, 0.1])
    x0 = beta * np.sqrt(nsamp)
    v = VAMP(N=N, Nt=sum(N), M=M, K=K, rho=0.5, gamw=5.0, gam1=1e-6, a=[1 / K] * K,
             out_dir=str(tmp_path), out_name="wide", seed=9, write_files=False, **prior)
    v.attach_engine(eng, x0=x0)
    its = 4
    xh = v.infer(None, None, its, x0=x0, lmmse_damp=False, prior_update=update)
    L = vo.BlockLD(blocks)
    t = vo.infer([L], [0] * K, rvec, N, its, rho=0.5, gamw=5.0, gam1=1e-6, x0=x0, seed=9,
                 lmmse_damp=False, prior_update=update,
                 reducer=vo.Reducer("blocked", bounds=L.bounds), rs_recurrence=True, **prior)
    for it in range(its):
        assert maxrel(xh[it].ravel() / np.sqrt(sum(N)), np.asarray(t["xhat"][it])) < 1e-8, it
    assert [h["cg_iters"] for h in v.history] == [[list(c) for c in x] for x in t["cg_iters"]]
    if update == "em":
        assert [h.get("em_steps") for h in v.history][1:] == list(t["em_steps"])
    eng.close()
