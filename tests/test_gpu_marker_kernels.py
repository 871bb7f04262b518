"""The marker gate: the marker-wise kernels of vec.hip, the ordered reductions
and the pipelined CG / EM control against references that do not share their
formulas or their summation order (tests/marker_ref.py; premise proved on the
CPU by tests/test_marker_ref.py).

  a  every k_denoise instantiation and the cohort-group path against the
     spike-and-slab posterior, in every regime;
  b  every EM_DISPATCH arm and the accumulating groups against the model's EM
     step; the device loop against the host loop, bitwise, on both control forms;
  c  the MLE sums;
  d  exact integer sums over every partition shape, on both reduction paths;
     per-marker results independent of the partition;
  e  the CG control over the same shapes: counts and iterates against the
     oracle, pipelined against host loop bitwise.

Tolerances: marker_ref's rule, from the f64 oracle's own distance on the very
inputs.  Every figure is printed before it is asserted (pytest -s)."""
import numpy as np
import pytest

import hip_backend as hb
from engine import Engine
from oracle import vamp_oracle as vo
from tests import marker_ref as mr

pytestmark = pytest.mark.gpu

EDGES = mr.PARTS["edges"]
M_EDGES = sum(EDGES)


def _engine(sizes, c):
    eng = Engine(sizes, K=c["r1s"].shape[0])
    for k, r in enumerate(c["r1s"]):
        eng.set_vector(hb.VEC_R1, k, r)
    return eng


def _prior(c):
    return c["gam1s"], c["a"], c["lam"], c["omegas"], c["sigmas"]


# ---------------------------------------------------------------------------
# a. denoiser forms
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", mr.DEN_KS)
def test_denoiser_vs_posterior(K):
    """xhat1 per marker and every cohort's derivative sum against the posterior
    mean and a_k gam1_k sum_m Var(x | r1); then the damped call from a known
    xhat1 is rho new + (1 - rho) old bitwise, with the same derivative sums."""
    cases = [c for c in mr.DEN_CASES if c[2] == K]
    assert cases
    rho = 0.3
    old = np.random.RandomState(K).normal(size=M_EDGES)
    eng = None
    for cs in cases:
        c = mr.case(cs, M_EDGES)
        if eng is None:
            eng = _engine(EDGES, c)
        else:
            for k, r in enumerate(c["r1s"]):
                eng.set_vector(hb.VEC_R1, k, r)
        gam1s, a, lam, omegas, sigmas = _prior(c)
        dx, dd, post = mr.den_distances(c)
        eng.set_vector(hb.VEC_XHAT1, 0, old)
        der = eng.denoise(gam1s, a, lam, omegas, sigmas, rho=rho, damp=False)
        x = eng.get_vector(hb.VEC_XHAT1)
        ex, ed = mr.dist_xhat(x, post), mr.dist_rel(der, post["der"])
        print("%s: xhat1 %.3e (oracle %.3e, tol %.3e)  der %.3e (oracle %.3e, tol %.3e)"
              % (mr.case_id(cs), ex, dx, mr.tolerance(dx, mr.CAP_X), ed, dd,
                 mr.tolerance(dd, mr.CAP_DER)))
        assert np.isfinite(x).all() and np.isfinite(der).all(), mr.case_id(cs)
        assert ex <= mr.tolerance(dx, mr.CAP_X), mr.case_id(cs)
        errs = np.abs(der - post["der"].astype(np.float64)) / np.abs(post["der"].astype(np.float64))
        assert ed <= mr.tolerance(dd, mr.CAP_DER), (mr.case_id(cs), "cohort", int(np.argmax(errs)))
        assert x[0] == 0.0                                   # the planted r1 = 0
        # the planted head (one sign in every cohort: no cancellation) plainly relative
        nh = len(mr.HEAD)
        ref_h = post["mean"][1:nh]
        dh = mr.dist_rel(vo.denoiser_meta(**c)[1:nh], ref_h)
        eh = mr.dist_rel(x[1:nh], ref_h)
        print("    head, relative: %.3e (oracle %.3e)" % (eh, dh))
        assert eh <= mr.tolerance(dh, mr.CAP_X), mr.case_id(cs)
        eng.set_vector(hb.VEC_XHAT1, 0, old)
        der2 = eng.denoise(gam1s, a, lam, omegas, sigmas, rho=rho, damp=True)
        x2 = eng.get_vector(hb.VEC_XHAT1)
        np.testing.assert_array_equal(x2, rho * x + (1 - rho) * old, err_msg=mr.case_id(cs))
        np.testing.assert_array_equal(der2, der, err_msg=mr.case_id(cs))
    eng.close()


# ---------------------------------------------------------------------------
# b. EM
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cs", mr.EM_CASES, ids=mr.case_id)
def test_em_step_vs_model(cs):
    """One EM step (device loop and host loop: bitwise the same) against the
    model's responsibilities."""
    c = mr.case(cs, M_EDGES)
    gam1s, a, lam, omegas, sigmas = _prior(c)
    dl, do, (lam_r, om_r) = mr.em_distances(c)
    eng = _engine(EDGES, c)
    got = {}
    for pipe in (True, False):
        eng.set_cg_pipeline(pipe)
        got[pipe] = eng.em(gam1s, a, sigmas, 1, lam, omegas)
    eng.close()
    lam_g, om_g, steps, _ = got[True]
    el, eo = mr.dist_rel(lam_g, lam_r), mr.dist_rel(om_g, om_r)
    print("%s: lam %.3e (oracle %.3e, tol %.3e)  omegas %.3e (oracle %.3e, tol %.3e)"
          % (mr.case_id(cs), el, dl, mr.tolerance(dl, mr.CAP_X), eo, do,
             mr.tolerance(do, mr.CAP_X)))
    assert steps == 1
    assert el <= mr.tolerance(dl, mr.CAP_X)
    assert eo <= mr.tolerance(do, mr.CAP_X)
    _same_em(got[True], got[False])


def _same_em(p, h):
    assert (p[0], p[2], p[3]) == (h[0], h[2], h[3]), (p, h)
    np.testing.assert_array_equal(p[1], h[1])


def _oracle_em_err(c, steps):
    """max(omegas, lam relative change) of the oracle's EM step number `steps`."""
    lam, om = c["lam"], c["omegas"]
    for _ in range(steps):
        lam_n, om_n = vo.prior_update_em(c["r1s"], c["gam1s"], c["a"], lam, om, c["sigmas"])
        err = max(np.linalg.norm(om_n - om) / np.linalg.norm(om), abs(lam_n - lam) / lam_n)
        lam, om = lam_n, om_n
    return err


@pytest.mark.parametrize("K,nslab", [(3, 3), (33, 2)])
@pytest.mark.parametrize("part", ["edges", "mixed12", "mixed13"])
def test_em_device_loop_matches_host_loop_bitwise(part, K, nslab):
    """The EM loop with the control on the device (one fused reduction +
    control launch up to 12 LD blocks, k_reduce_local + k_em_ctl from 13) and on
    the host: (lam, omegas, steps, err) bitwise, at 25 steps, at one, and where
    the step limit ends the loop."""
    sizes = mr.PARTS[part]
    c = mr.case(("benign", 0, K, nslab), sum(sizes))
    gam1s, a, lam, omegas, sigmas = _prior(c)
    assert _oracle_em_err(c, 3) > 1e-4          # three steps do not converge (1e-6)
    eng = _engine(sizes, c)
    for maxit in (25, 1, 3):
        got = {}
        for pipe in (True, False):
            eng.set_cg_pipeline(pipe)
            got[pipe] = eng.em(gam1s, a, sigmas, maxit, lam, omegas)
        print(part, K, nslab, maxit, got[True][2], got[True][3])
        _same_em(got[True], got[False])
        assert 1 <= got[True][2] <= maxit
        if maxit == 3:
            assert got[True][2] == 3 and got[True][3] > 1e-6
    eng.close()


# ---------------------------------------------------------------------------
# c. MLE sums
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cs", mr.MLE_CASES, ids=mr.case_id)
def test_mle_sums_vs_model(cs):
    c = mr.case(cs, M_EDGES, mle=True)
    sigma2, omega = mr.mle_inputs(c)
    d, ref = mr.mle_distance(c)
    em_o, _ = mr.mle_oracle_sums(c)
    eng = _engine(EDGES, c)
    em = eng.mle_exp_max(c["gam1s"], sigma2)
    S = eng.mle_terms(c["a"], c["gam1s"], sigma2, omega, em)
    # with the planted r1 = 0 the maximum is 0; without the two smallest markers
    # it is attained at a cohort- and component-dependent place
    r2 = c["r1s"].copy()
    r2[:, :2] = 0.37 * r2[:, 2:4]
    for k, r in enumerate(r2):
        eng.set_vector(hb.VEC_R1, k, r)
    em2 = eng.mle_exp_max(c["gam1s"], sigma2)
    eng.close()
    em2_o = vo.mle_exp_max(r2, c["gam1s"], sigma2)
    assert em2 == em2_o and em2 < 0.0, (em2, em2_o)
    e = mr.dist_rel(S, ref)
    print("%s: exp_max %r (oracle %r)  S %.3e (oracle %.3e, tol %.3e)"
          % (mr.case_id(cs), em, float(em_o), e, d, mr.tolerance(d, mr.CAP_X)))
    assert em == em_o                           # a max of one expression: the same bits
    assert np.isfinite(S).all()
    assert e <= mr.tolerance(d, mr.CAP_X)


# ---------------------------------------------------------------------------
# d. partition shapes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("exchange", [None, "host"], ids=["local", "rehearsal"])
@pytest.mark.parametrize("part", list(mr.PARTS))
def test_metrics_sums_exact_on_every_partition(part, exchange):
    """metrics() over integer vectors whose sums are exact in any order equals
    the integer sums: k_reduce_local (one rank) and k_reduce_blocks +
    k_reduce_total (the one-rank exchange rehearsal) drop, double or misplace no
    chunk and no block."""
    sizes = mr.PARTS[part]
    x, x0, sums = mr.exact_vectors(sum(sizes), 7)
    eng = Engine(sizes, K=1, exchange=exchange)
    eng.set_vector(hb.VEC_XHAT1, 0, x)
    eng.set_vector(hb.VEC_X0, 0, x0)
    got = eng.metrics()
    eng.close()
    np.testing.assert_array_equal(got, sums)


def test_denoiser_is_partition_independent():
    """The same markers cut into mixed9's blocks, into the edges blocks and a
    remainder, and into one block: xhat1 per marker bitwise the same, the
    derivative sums within the tolerance."""
    M = sum(mr.PARTS["mixed9"])
    cuts = {"mixed9": mr.PARTS["mixed9"], "edges+rest": EDGES + [M - M_EDGES], "one block": [M]}
    cs = ("late", 0, 4, 3)
    c = mr.case(cs, M)
    gam1s, a, lam, omegas, sigmas = _prior(c)
    dx, dd, post = mr.den_distances(c)
    xs = {}
    for name, sizes in cuts.items():
        assert sum(sizes) == M
        eng = _engine(sizes, c)
        der = eng.denoise(gam1s, a, lam, omegas, sigmas, rho=0.5, damp=False)
        xs[name] = eng.get_vector(hb.VEC_XHAT1)
        eng.close()
        e = mr.dist_rel(der, post["der"])
        print(name, "der %.3e (oracle %.3e, tol %.3e)" % (e, dd, mr.tolerance(dd, mr.CAP_DER)))
        assert e <= mr.tolerance(dd, mr.CAP_DER), name
    assert mr.dist_xhat(xs["one block"], post) <= mr.tolerance(dx, mr.CAP_X)
    for name in cuts:
        np.testing.assert_array_equal(xs[name], xs["one block"], err_msg=name)


@pytest.mark.parametrize("part", ["c64", "c65"])
def test_em_loop_bitwise_across_the_lane_round(part):
    """A block of 64 and of 65 chunks: the fused control's per-block lane loop
    (lb_reduce) takes a second round exactly where k_reduce_local's does."""
    sizes = mr.PARTS[part]
    cs = ("benign", 0, 1, 2)
    c = mr.case(cs, sum(sizes))
    gam1s, a, lam, omegas, sigmas = _prior(c)
    dl, do, (lam_r, om_r) = mr.em_distances(c)
    eng = _engine(sizes, c)
    for maxit in (1, 5):
        got = {}
        for pipe in (True, False):
            eng.set_cg_pipeline(pipe)
            got[pipe] = eng.em(gam1s, a, sigmas, maxit, lam, omegas)
        _same_em(got[True], got[False])
        if maxit == 1:   # a chunk that drops out of both sums alike shows here
            assert mr.dist_rel(got[True][0], lam_r) <= mr.tolerance(dl, mr.CAP_X)
            assert mr.dist_rel(got[True][1], om_r) <= mr.tolerance(do, mr.CAP_X)
    eng.close()


# ---------------------------------------------------------------------------
# e. CG control over the shapes
# ---------------------------------------------------------------------------
CG_SHAPES = ["mixed8", "mixed9", "b17", "b1025", "c65"]
CG_RTOL_X = 1e-7          # the project's bound for CG iterates against the oracle
CG_RTOL_LOOKAHEAD = 1e-10  # test_cg_exact_columns_vs_lookahead's
_CG = {}


def _offdiag(b, n):
    """Block b's first off-diagonal: distinct per block, so even 1,025 blocks of
    1-3 markers give A many distinct eigenvalues."""
    return 0.2 + 0.25 * ((b * 7) % 17) / 17.0 + 0.01 * np.cos(np.arange(max(n - 1, 0)))


def _cg_system(part):
    """(engine, matvec_R, bounds) of R for partition `part`, built once: unit
    diagonal, |off-diagonal| row sums < 0.95, so c1 R + c2 I is strictly
    diagonally dominant (symmetric positive definite) for any c1 > 0, c2 >= 0."""
    if part in _CG:
        return _CG[part]
    import scipy.sparse

    sizes = mr.PARTS[part]
    eng = Engine(sizes, K=1)
    rs = np.random.RandomState(len(sizes))
    mats = []
    for b, n in enumerate(sizes):
        if part == "c65":        # a narrow band, stored from its upper triangle
            d1 = 0.35 + 0.01 * np.cos(np.arange(n - 1))
            U = scipy.sparse.diags([np.ones(n), d1, np.full(n - 2, -0.1)], [0, 1, 2], format="csr")
            eng.set_ld_block_csr(0, b, U)
            R = (U + scipy.sparse.triu(U, 1).T).tocsr()
            rows = np.asarray(abs(R).sum(axis=1)).ravel() - 1.0
        else:                    # dense: the same band under a small dense symmetric part
            N = rs.uniform(-1, 1, (n, n)) * (0.02 / n)
            R = (N + N.T) / 2
            i = np.arange(n)
            R[i, i] = 1.0
            R[i[:-1], i[1:]] += _offdiag(b, n)
            R[i[1:], i[:-1]] += _offdiag(b, n)
            eng.set_ld_block(0, b, R)
            rows = np.abs(R).sum(axis=1) - 1.0
        assert rows.max() < 0.95
        mats.append(R)
    bounds = np.cumsum([0] + list(sizes))
    if part == "c65":
        A = scipy.sparse.block_diag(mats, format="csr")
        mv = vo.CsrLD(A).matvec_Rs
    else:
        mv = vo.BlockLD(mats).matvec_Rs
    _CG[part] = (eng, mv, bounds)
    return _CG[part]


@pytest.fixture(scope="module", autouse=True)
def _close_cg_engines():
    yield
    for eng, _, _ in _CG.values():
        eng.close()
    _CG.clear()


def _solve(eng, pipe, exact, c1, c2, B, X0, maxiter):
    eng.set_cg_pipeline(pipe)
    eng.ctx.sgv_set_cg_exact(exact)
    return eng.cg_solve(0, c1, c2, B, X0, maxiter)


def _same_cg(p, h, what):
    np.testing.assert_array_equal(p[1], h[1], err_msg="iters, %s" % (what,))
    np.testing.assert_array_equal(p[2], h[2], err_msg="info, %s" % (what,))
    np.testing.assert_array_equal(p[0], h[0], err_msg="X, %s" % (what,))


def _maxrel(a, b):
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


def _columns(M, ncol):
    """c1, c2, B, X0: c2 from 1e7 (one iteration) down to 0.05 (more than two
    turns of the 4-slot mirror ring); at 6 columns a zero right-hand side; the
    last column warm-started."""
    rs = np.random.RandomState(M + ncol)
    if ncol == 2:
        c1, c2 = np.array([1.0, 1.5]), np.array([1e7, 0.05])
    else:
        c1 = np.array([1.0, 2.0, 0.5, 1.0, 1.0, 1.5])
        c2 = np.array([1e7, 1.0, 0.3, 0.05, 0.5, 0.05])
    B = rs.normal(size=(ncol, M))
    X0 = np.zeros((ncol, M))
    X0[-1] = rs.normal(size=M) * 0.1
    if ncol == 6:
        B[4] = 0.0
    return c1, c2, B, X0


@pytest.mark.parametrize("ncol", [2, 6])
@pytest.mark.parametrize("part", CG_SHAPES)
def test_cg_control_vs_oracle_and_host_loop(part, ncol):
    """Iteration counts and info equal the oracle's (per-block sums in block
    order), X within 1e-7; pipelined against host loop bitwise where both run
    the same column sets (2 columns; 6 with exact sets), equal counts and X
    within 1e-10 in look-ahead mode."""
    eng, mv, bounds = _cg_system(part)
    M = int(bounds[-1])
    c1, c2, B, X0 = _columns(M, ncol)
    red = vo.Reducer("blocked", bounds)
    ref = [vo.cg_scipy(lambda p, j=j: c1[j] * mv(p) + c2[j] * p, B[j], X0[j], 500, red)
           for j in range(ncol)]
    its = [r[2] for r in ref]
    print(part, ncol, "oracle iterations", its)
    assert min(i for j, i in enumerate(its) if B[j].any()) <= 2 and max(its) >= 10
    run = {(pipe, exact): _solve(eng, pipe, exact, c1, c2, B, X0, 500)
           for pipe in (True, False) for exact in ((0, 1) if ncol == 6 else (0,))}
    for key, (X, it, info) in run.items():
        assert it.tolist() == its and info.tolist() == [r[1] for r in ref], (key, it, info)
        for j in range(ncol):
            e = _maxrel(X[j], ref[j][0])
            assert e < CG_RTOL_X, (key, j, e)
    if ncol == 6:
        assert not run[(True, 0)][0][4].any()                # the zero right-hand side
        _same_cg(run[(True, 1)], run[(False, 1)], "exact column sets")
        for j in range(ncol):
            e = _maxrel(run[(True, 0)][0][j], run[(False, 0)][0][j])
            print("look-ahead vs host loop, column", j, e)
            assert e < CG_RTOL_LOOKAHEAD, (j, e)
    else:
        _same_cg(run[(True, 0)], run[(False, 0)], "2 columns")


@pytest.mark.parametrize("part", CG_SHAPES)
def test_cg_maxiter_at_the_ring_boundary(part):
    """maxiter below, at and past the 4 mirror slots with a column that does not
    converge (and one that does at iteration 1): counts and info the oracle's,
    pipelined against host loop bitwise."""
    eng, mv, bounds = _cg_system(part)
    M = int(bounds[-1])
    c1, c2, B, X0 = _columns(M, 2)
    red = vo.Reducer("blocked", bounds)
    for maxiter in (0, 1, 3, 4, 5, 8):
        ref = [vo.cg_scipy(lambda p, j=j: c1[j] * mv(p) + c2[j] * p, B[j], X0[j], maxiter, red)
               for j in range(2)]
        p = _solve(eng, True, 0, c1, c2, B, X0, maxiter)
        h = _solve(eng, False, 0, c1, c2, B, X0, maxiter)
        assert (ref[1][2], ref[1][1]) == (maxiter, maxiter)
        assert p[1].tolist() == [r[2] for r in ref] and p[2].tolist() == [r[1] for r in ref], \
            (maxiter, p[1], p[2])
        _same_cg(p, h, "maxiter %d" % maxiter)
        for j in range(2):
            assert _maxrel(p[0][j], ref[j][0]) < CG_RTOL_X, (maxiter, j)


@pytest.mark.parametrize("part", CG_SHAPES)
def test_cg_scaled_columns_stop_together(part):
    """Six columns that are power-of-two multiples of one right-hand side: every
    scalar scales exactly, all stop at the same iteration, and the column sets
    of the two loops coincide in every mode -- bitwise in both."""
    eng, mv, bounds = _cg_system(part)
    M = int(bounds[-1])
    b = np.random.RandomState(M).normal(size=M)
    scale = np.array([1.0, 2.0, 0.5, 8.0, 0.25, 4.0])
    B = scale[:, None] * b[None, :]
    X0 = np.zeros((6, M))
    c1, c2 = np.full(6, 1.0), np.full(6, 0.05)
    red = vo.Reducer("blocked", bounds)
    _, info_r, it_r, _ = vo.cg_scipy(lambda p: mv(p) + 0.05 * p, b, X0[0], 500, red)
    for exact in (0, 1):
        p = _solve(eng, True, exact, c1, c2, B, X0, 500)
        h = _solve(eng, False, exact, c1, c2, B, X0, 500)
        assert p[1].tolist() == [it_r] * 6 and p[2].tolist() == [info_r] * 6, (exact, p[1], p[2])
        _same_cg(p, h, "scaled columns, exact=%d" % exact)


@pytest.mark.parametrize("part", ["mixed8", "mixed9"])
def test_pass_ledger_is_the_same_in_every_loop(part):
    """The pass counters of timers() over one six-column solve, in the four
    (pipelined, exact) arms, on the fused (mixed8) and the two-launch (mixed9)
    control path: ld_launches is the warm-start pass of the last column plus one
    pass per CG iteration of the slowest column -- the pipelined loop's no-op
    look-ahead iteration is rolled back, not counted; ld_bytes is the same in
    every arm, rhs_bytes in the two exact arms (the same column sets)."""
    eng, _, bounds = _cg_system(part)
    c1, c2, B, X0 = _columns(int(bounds[-1]), 6)
    led = {}
    for pipe in (True, False):
        for exact in (0, 1):
            eng.timers(reset=True)
            _, it, _ = _solve(eng, pipe, exact, c1, c2, B, X0, 500)
            t = eng.timers()
            print(part, pipe, exact, "iters", it.tolist(), "launches", t["ld_launches"],
                  "ld_bytes", t["ld_bytes"], "rhs_bytes", t["rhs_bytes"])
            assert t["ld_launches"] == 1 + int(it.max()), (pipe, exact, t["ld_launches"], it)
            led[(pipe, exact)] = t
    assert len({t["ld_bytes"] for t in led.values()}) == 1, led
    assert led[(True, 1)]["rhs_bytes"] == led[(False, 1)]["rhs_bytes"], led
