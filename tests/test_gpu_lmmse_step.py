"""The LMMSE gate: Engine.lmmse (sgv_lmmse: k_unpack_i8, the warm-start pass,
k_lmmse_init, the CG, k_lmmse_post, the ordered reductions, k_r1_update and the
host scalars) against references that share neither its formulas' code nor its
summation order (tests/lmmse_ref.py; premises proved on the CPU by
tests/test_lmmse_ref.py).

  tier 1  cg_maxit = 0 on exact data: every output, r1 and the vectors bit for
          bit against integer sums, in all sixteen mode combinations, every
          cohort grouping and through the one-rank exchange;
  tier 2  converged at rtol 1e-13 against the refined dense solve over three
          consecutive calls (cold; warm and damped; new gamw / gam2), carried
          products and direct ones, pipelined and host loop;
  tier 3  state set from outside between calls (set_vector, set_rs_recurrence,
          reset_solver, a zero right-hand side), the queued metrics and the
          argument checks.

Bounds: lmmse_ref's rule, from the f64 oracle's own distance under the cap
2 kappa rtol.  Every figure is printed before it is asserted (pytest -s)."""
import numpy as np
import pytest

import hip_backend as hb
from engine import Engine
from tests import lmmse_ref as lr
from tests import marker_ref as mr

pytestmark = pytest.mark.gpu

CG_RTOL_LOOKAHEAD = 1e-10   # the marker gate's bound of look-ahead against host loop
_ENG = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for eng in _ENG.values():
        eng.close()
    _ENG.clear()


def _modes():
    return [(rs, pipe, damp, learn) for rs in (True, False) for pipe in (True, False)
            for damp in (False, True) for learn in (False, True)]


# ---------------------------------------------------------------------------
# tier 1
# ---------------------------------------------------------------------------
def _t1_engine(shape, cfg, exchange):
    key = ("t1", shape, cfg, exchange)
    if key not in _ENG:
        ld_of = lr.COHORTS[cfg]
        eng = Engine(mr.PARTS[shape], K=len(ld_of), ld_of=ld_of, exchange=exchange)
        for ld in sorted(set(ld_of)):
            for b, B in enumerate(lr.t1_blocks(shape, ld)):
                if hasattr(B, "indptr"):
                    eng.set_ld_block_csr(ld, b, B)
                else:
                    eng.set_ld_block(ld, b, B)
        _ENG[key] = eng
    return _ENG[key]


def _t1_set(eng, c, x2=None, s2u=None):
    """r1, XHAT2 and SIG2U of every cohort from outside (x2 / s2u: {k: vector}
    overrides)."""
    for k in range(c["K"]):
        eng.set_vector(hb.VEC_R1, k, c["r1"][k])
        eng.set_vector(hb.VEC_XHAT2, k, c["x2"][k] if x2 is None or k not in x2 else x2[k])
        eng.set_vector(hb.VEC_SIG2U, k, c["s2u"][k] if s2u is None or k not in s2u else s2u[k])


def _t1_call(eng, c, damp, learn):
    K = c["K"]
    return eng.lmmse(0, c["gamw"], c["gam2"], [lr.ALPHA1] * K, c["a2prev"], np.stack(c["u"]), 0,
                     damp, lr.RHO1, learn)


def _t1_assert(eng, c, got, exp, what, x2=None, s2u=None):
    out, cg, _ = got
    eo, er1 = exp
    for i, name in enumerate(lr.OUT_NAMES):
        np.testing.assert_array_equal(out[:, i], eo[:, i], err_msg="%s %s" % (what, name))
    np.testing.assert_array_equal(cg, np.zeros((c["K"], 4), dtype=np.int32), err_msg=str(what))
    for k in range(c["K"]):
        np.testing.assert_array_equal(eng.get_vector(hb.VEC_R1, k), er1[k], err_msg="%s r1 %d" % (what, k))
        np.testing.assert_array_equal(eng.get_vector(hb.VEC_XHAT2, k),
                                      c["x2"][k] if x2 is None or k not in x2 else x2[k],
                                      err_msg="%s XHAT2 %d" % (what, k))
        np.testing.assert_array_equal(eng.get_vector(hb.VEC_SIG2U, k),
                                      c["s2u"][k] if s2u is None or k not in s2u else s2u[k],
                                      err_msg="%s SIG2U %d" % (what, k))


T1_CASES = [(shape, cfg, None) for shape in lr.T1_SHAPES for cfg in lr.COHORTS] + \
           [(shape, cfg, "host") for shape in lr.T1_SHAPES for cfg in ("K2", "K9")]


@pytest.mark.parametrize("shape,cfg,exchange", T1_CASES,
                         ids=["%s-%s-%s" % (s, c, e or "local") for s, c, e in T1_CASES])
def test_zero_iteration_step_is_exact(shape, cfg, exchange):
    """cg_maxit = 0: TRSIGMA2, XR, XRX, TRRSIGMA2 equal the integer sums, ALPHA2,
    GAM1, Z (clamped in the last cohort), GAMW the f64 expressions of them, r1
    the update, XHAT2 (damped with itself) and SIG2U untouched, no CG iteration
    counted -- bit for bit, for both ridges and all sixteen combinations of
    carried products, pipelined control, damping and gamw learning (so they all
    agree); through the one-rank exchange (reduce_exchange) the same.

    Each (carried, pipelined) setting first runs a real CG, so a finished
    solve's control state is on the device.  That exposed a second bug: with a
    communicator the pipelined prologue's sums ride in iteration 0's exchange
    (merge0), and with cg_maxit = 0 there is no iteration 0 -- nothing set the CG
    state and cg_out reported the previous solve's counts ([2, 0, 3, 0] instead
    of zeros).  merge0 now needs cg_maxit > 0."""
    eng = _t1_engine(shape, cfg, exchange)
    for s in lr.RIDGES:
        c = lr.t1_case(shape, cfg, s)
        eng.set_ridge(s)
        for k in range(c["K"]):
            eng.set_cohort_n(k, c["N"][k])
            eng.set_vector(hb.VEC_R, k, c["r"][k])
        eng.set_vector(hb.VEC_XHAT1, 0, c["xhat1"])
        for rs, pipe, damp, learn in _modes():
            eng.set_rs_recurrence(rs)
            eng.set_cg_pipeline(pipe)
            if not damp and not learn:
                # a finished CG (A next to 64 I: a few iterations) leaves its control
                # state and iteration counts behind; the vectors are set again below
                _t1_set(eng, c)
                K = c["K"]
                _, cg, _ = eng.lmmse(0, [2.0 ** -10] * K, [64.0] * K, [lr.ALPHA1] * K, c["a2prev"],
                                     np.stack(c["u"]), 50, False, lr.RHO1, False)
                assert cg[:, [0, 2]].min() >= 1 and not cg[:, [1, 3]].any(), cg
            _t1_set(eng, c)
            got = _t1_call(eng, c, damp, learn)
            what = (shape, cfg, exchange, s, "rs %d pipe %d damp %d learn %d" % (rs, pipe, damp, learn))
            exp = lr.t1_expected(c, damp, learn)
            print(what, "passes", got[2], "out[0]", got[0][0].tolist())
            _t1_assert(eng, c, got, exp, what)
            assert got[2] == lr.expected_passes(c["ld_of"], True, learn, rs), what
    if (shape, cfg, exchange) != ("edges", "K2", None):   # that one serves the next test too
        _ENG.pop(("t1", shape, cfg, exchange)).close()


@pytest.mark.parametrize("rs", [True, False], ids=["carried", "direct"])
@pytest.mark.parametrize("which", ["SIG2U", "XHAT2"])
def test_zero_iteration_step_after_a_vector_is_zeroed(which, rs):
    """After a step that left R_s X behind, set_vector(zeros) for cohort 0: the
    zeroed column's products are exactly 0 (TRRSIGMA2 for SIG2U; XR, XRX for
    XHAT2), everything else as before, bit for bit.  This is the cold column
    whose RX0 nothing used to zero: with the carried products TRRSIGMA2 came out
    as the previous step's u.R_s Sigma2_u."""
    shape, cfg, s = "edges", "K2", 0.25
    eng = _t1_engine(shape, cfg, None)
    c = lr.t1_case(shape, cfg, s)
    eng.set_ridge(s)
    for k in range(c["K"]):
        eng.set_cohort_n(k, c["N"][k])
        eng.set_vector(hb.VEC_R, k, c["r"][k])
    eng.set_vector(hb.VEC_XHAT1, 0, c["xhat1"])
    eng.set_rs_recurrence(rs)
    zeros = np.zeros(c["M"])
    for pipe in (True, False):
        eng.set_cg_pipeline(pipe)
        _t1_set(eng, c)
        _t1_assert(eng, c, _t1_call(eng, c, True, True), lr.t1_expected(c, True, True), "before")
        sums = [dict(sm) for sm in c["sums"]]
        if which == "SIG2U":
            sums[0]["TrS"] = sums[0]["TrRS"] = 0.0
            over = dict(s2u={0: zeros})
        else:
            sums[0]["XR"] = sums[0]["XRX"] = 0.0
            over = dict(x2={0: zeros})
        for k in range(c["K"]):
            eng.set_vector(hb.VEC_R1, k, c["r1"][k])
        eng.set_vector(hb.VEC_SIG2U if which == "SIG2U" else hb.VEC_XHAT2, 0, zeros)
        got = _t1_call(eng, c, True, True)
        print(which, rs, pipe, "TRRSIGMA2", got[0][0][lr.O_TRRSIGMA2], "XRX", got[0][0][lr.O_XRX])
        exp = lr.t1_expected(c, True, True, sums=sums, x2=[over.get("x2", {}).get(k, c["x2"][k])
                                                           for k in range(c["K"])])
        _t1_assert(eng, c, got, exp, (which, rs, pipe), **over)


def test_zero_iteration_step_divides_by_the_global_marker_count():
    """A context that holds a slice of a larger problem (M_total = M + 1000, no
    communicator): alpha2 is gam2 TrSigma2 / M_total on the host and in
    k_r1_update alike (pipelined and host loop), bit for bit."""
    shape, cfg, s = "edges", "K2", 0.25
    c = lr.t1_case(shape, cfg, s)
    Mtot = c["M"] + 1000
    eng = Engine(c["sizes"], K=c["K"], ld_of=c["ld_of"])
    try:
        eng.ctx.close()
        eng.ctx = hb.Context(0, c["K"], eng.ld_of, eng.local_sizes, 0, len(c["sizes"]), Mtot)
        for b, B in enumerate(lr.t1_blocks(shape, 0)):
            eng.set_ld_block(0, b, B)
        eng.set_ridge(s)
        for k in range(c["K"]):
            eng.set_cohort_n(k, c["N"][k])
            eng.set_vector(hb.VEC_R, k, c["r"][k])
        eng.set_vector(hb.VEC_XHAT1, 0, c["xhat1"])
        exp = lr.t1_expected(dict(c, M=Mtot), True, True)
        assert (exp[0][:, lr.O_ALPHA2] != lr.t1_expected(c, True, True)[0][:, lr.O_ALPHA2]).all()
        for pipe in (True, False):
            eng.set_cg_pipeline(pipe)
            _t1_set(eng, c)
            _t1_assert(eng, c, _t1_call(eng, c, True, True), exp, ("M_total", pipe))
    finally:
        eng.close()


# ---------------------------------------------------------------------------
# tier 2
# ---------------------------------------------------------------------------
def _t2_engine(shape, K, fresh=False, exchange=None):
    key = ("t2", shape, K, exchange)
    if fresh or key not in _ENG:
        S = lr.system(shape)
        ld_of = lr.T2_LD_OF[:K]
        eng = Engine(S.sizes, K=K, ld_of=ld_of, exchange=exchange)
        S.upload(eng, sorted(set(ld_of)))
        eng.set_ridge(S.s)
        if fresh:
            return eng
        _ENG[key] = eng
    return _ENG[key]


def _run(eng, seq, K, rs_modes, pipe, events=None, reset=True, ncall=None, inp_override=None):
    """The calls of a sequence on the device.  events: {n: [(which, k, vector or
    callable(eng))]} applied before call n.  Returns per call dict(out, cg,
    passes, x2, s2u, r1 [K])."""
    if reset:
        eng.reset_solver()
    eng.set_cg_pipeline(pipe)
    eng.set_rs_recurrence(rs_modes[0])
    res = []
    for n in range(len(seq["inp"]) if ncall is None else ncall):
        inps = seq["inp"][n][:K]
        if inp_override and n in inp_override:
            inps = inp_override[n][:K]
        if n > 0 and rs_modes[n] != rs_modes[n - 1]:
            eng.set_rs_recurrence(rs_modes[n])
        for which, k, v in (events or {}).get(n, []):
            eng.set_vector(which, k, v(eng) if callable(v) else v)
        eng.set_vector(hb.VEC_XHAT1, 0, inps[0]["xhat1"])
        for k, inp in enumerate(inps):
            eng.set_cohort_n(k, inp["N"])
            eng.set_vector(hb.VEC_R, k, inp["r"])
            eng.set_vector(hb.VEC_R1, k, inp["r1"])
        out, cg, passes = eng.lmmse(n, [i["gamw"] for i in inps], [i["gam2"] for i in inps],
                                    [i["alpha1"] for i in inps], [i["a2prev"] for i in inps],
                                    np.stack([i["u"] for i in inps]), lr.T2_MAXIT, seq["damp"][n],
                                    lr.T2_RHO, True, rtol=lr.T2_RTOL)
        res.append(dict(out=out, cg=cg, passes=passes,
                        x2=[eng.get_vector(hb.VEC_XHAT2, k) for k in range(K)],
                        s2u=[eng.get_vector(hb.VEC_SIG2U, k) for k in range(K)],
                        r1=[eng.get_vector(hb.VEC_R1, k) for k in range(K)]))
    return res


def _cohort(res, k):
    return dict(out=res["out"][k], x2=res["x2"][k], s2u=res["s2u"][k], r1=res["r1"][k])


def _check_run(res, seq, K, mode, what, calls=None):
    """Every call and cohort against the reference by the rule, info 0 and the
    oracle's iteration counts."""
    for n, rn in enumerate(res):
        if calls is not None and n not in calls:
            continue
        for k in range(K):
            ref = seq["ref"][n][k]
            if ref is None:
                continue
            ora = seq["ora"][mode][n][k]
            print("%s call %d cohort %d: cg %s (oracle %s) passes %d" % (
                what, n, k, rn["cg"][k].tolist(), ora["cg"], rn["passes"]))
            assert np.isfinite(rn["out"][k]).all()
            lr.check(_cohort(rn, k), ref, seq["dist"][mode][n][k], "%s call %d cohort %d" % (what, n, k))
            assert rn["cg"][k].tolist() == ora["cg"], (what, n, k)


def _host_passes(rn, ld_of, rs, extra):
    """LD passes of a host-loop call: per LD matrix one per CG iteration in which
    one of its columns still runs, the gamw passes without the carried products,
    and `extra` warm-start passes."""
    n = 0
    for ld in set(ld_of):
        n += max(max(rn["cg"][k][0], rn["cg"][k][2]) for k in range(len(ld_of)) if ld_of[k] == ld)
    return n + (0 if rs else len(set(ld_of))) + extra


def _same(a, b, what):
    for n, (x, y) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(x["out"], y["out"], err_msg="%s out, call %d" % (what, n))
        np.testing.assert_array_equal(x["cg"], y["cg"], err_msg="%s cg, call %d" % (what, n))
        for key in ("x2", "s2u", "r1"):
            for k, (u, v) in enumerate(zip(x[key], y[key])):
                np.testing.assert_array_equal(u, v, err_msg="%s %s %d, call %d" % (what, key, k, n))


def _maxrel(a, b):
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("shape", list(lr.T2_SHAPES))
def test_converged_steps_vs_dense_solve(shape, K):
    """Three consecutive calls (cold; warm and damped; new gamw and gam2) with
    the carried products and with direct ones, pipelined and host loop: every
    output, XHAT2, SIG2U and r1 within the rule's bound of the dense reference
    -- XRX and TRRSIGMA2 from the carried products against xhat2.R_s xhat2 and
    u.R_s Sigma2_u of the reference by the same bound as the direct ones --
    info 0, the oracle's iteration counts, the host loop's pass count.
    Pipelined against host loop: bitwise at K = 1 and with exact column sets,
    within 1e-10 in look-ahead mode."""
    eng = _t2_engine(shape, K)
    seq = lr.sequence(shape)
    ld_of = lr.T2_LD_OF[:K]
    runs = {}
    for rs in (True, False):
        for pipe in (True, False):
            what = "%s K%d %s %s" % (shape, K, "carried" if rs else "direct", "pipe" if pipe else "host")
            runs[(rs, pipe)] = res = _run(eng, seq, K, [rs] * 3, pipe)
            _check_run(res, seq, K, "rs" if rs else "direct", what)
            if not pipe:
                for n, rn in enumerate(res):
                    assert rn["passes"] == _host_passes(rn, ld_of, rs, 0), (what, n, rn["passes"])
        p, h = runs[(rs, True)], runs[(rs, False)]
        if K == 1:
            _same(p, h, "pipelined vs host loop")
        else:
            for n in range(3):
                np.testing.assert_array_equal(p[n]["cg"], h[n]["cg"])
                e = max([_maxrel(p[n][key][k], h[n][key][k]) for key in ("x2", "s2u", "r1")
                         for k in range(K)] + [_maxrel(p[n]["out"], h[n]["out"])])
                print("look-ahead vs host loop, call", n, e)
                assert e < CG_RTOL_LOOKAHEAD, (rs, n, e)
            eng.ctx.sgv_set_cg_exact(1)
            try:
                pe, he = _run(eng, seq, K, [rs] * 3, True), _run(eng, seq, K, [rs] * 3, False)
            finally:
                eng.ctx.sgv_set_cg_exact(eng.cg_exact)
            _same(pe, he, "exact column sets")
            _check_run(pe, seq, K, "rs" if rs else "direct", "exact sets", calls=[2])


@pytest.mark.parametrize("rs", [True, False], ids=["carried", "direct"])
def test_converged_steps_through_the_one_rank_exchange(rs):
    """K = 1 on a one-rank host exchange: the pipelined prologue's sums ride in
    iteration 0's exchange (merge0) and every reduction goes through
    reduce_exchange; the three calls match the reference and are bitwise the
    run without a communicator, pipelined and host loop."""
    seq = lr.sequence(lr.T3_SHAPE)
    local, xchg = _t2_engine(lr.T3_SHAPE, 1), _t2_engine(lr.T3_SHAPE, 1, exchange="host")
    for pipe in (True, False):
        a = _run(local, seq, 1, [rs] * 3, pipe)
        b = _run(xchg, seq, 1, [rs] * 3, pipe)
        _check_run(b, seq, 1, "rs" if rs else "direct", "exchange %s" % ("pipe" if pipe else "host"))
        _same(a, b, "one-rank exchange vs none")


# ---------------------------------------------------------------------------
# tier 3
# ---------------------------------------------------------------------------
T3_K = 2


@pytest.mark.parametrize("pipe", [True, False], ids=["pipe", "host"])
@pytest.mark.parametrize("rs", [True, False], ids=["carried", "direct"])
@pytest.mark.parametrize("name", ["x2zero", "s2uzero", "x2set"])
def test_vector_set_from_outside(name, rs, pipe):
    """After two steps cohort 0's XHAT2 or SIG2U is set to zeros, or XHAT2 to
    another vector; the third step matches the reference whose x_prev is that
    vector (0: a cold column, whose R_s x must be 0 too; non-zero: R_s v is
    re-derived by one more pass).

    The zeros cases are the suspect of the issue, and it was real: a column
    zeroed from outside kept the previous step's R_s x in RX0, the carried
    recurrence added to it and the damping saved it, so XRX, TRRSIGMA2 and the
    learned gamw of the next step were wrong (measured before the fix: see
    profiles/lmmse_gate/tolerances.txt).  sgv_set_vector now zeroes the
    column's RX0 with it."""
    eng = _t2_engine(lr.T3_SHAPE, T3_K)
    seq = lr.t3_sequence(name)
    M = lr.system(lr.T3_SHAPE).M
    which = hb.VEC_SIG2U if name == "s2uzero" else hb.VEC_XHAT2
    v = lr.t3_vector(lr.T3_SHAPE) if name == "x2set" else np.zeros(M)
    res = _run(eng, seq, T3_K, [rs] * 3, pipe, events={2: [(which, 0, v)]})
    _check_run(res, seq, T3_K, "rs" if rs else "direct", "%s %s" % (name, "carried" if rs else "direct"))
    if not pipe:
        extra = 1 if name == "x2set" else 0
        assert res[2]["passes"] == _host_passes(res[2], lr.T2_LD_OF[:T3_K], rs, extra), res[2]["passes"]


@pytest.mark.parametrize("rs", [True, False], ids=["carried", "direct"])
def test_same_vector_set_from_outside_costs_one_pass(rs):
    """XHAT2 read back and set again before the third call (host loop): the same
    iteration counts as without the set, one LD pass more, the same bounds."""
    eng = _t2_engine(lr.T3_SHAPE, T3_K)
    seq = lr.sequence(lr.T3_SHAPE)
    plain = _run(eng, seq, T3_K, [rs] * 3, False)
    again = _run(eng, seq, T3_K, [rs] * 3, False,
                 events={2: [(hb.VEC_XHAT2, 0, lambda e: e.get_vector(hb.VEC_XHAT2, 0))]})
    _same(plain[:2], again[:2], "before the set")
    _check_run(again, seq, T3_K, "rs" if rs else "direct", "set again", calls=[2])
    np.testing.assert_array_equal(again[2]["cg"], plain[2]["cg"])
    print("passes", plain[2]["passes"], again[2]["passes"])
    assert again[2]["passes"] == plain[2]["passes"] + 1


@pytest.mark.parametrize("pipe", [True, False], ids=["pipe", "host"])
def test_carried_products_toggled_between_steps(pipe):
    """set_rs_recurrence on, off, on between the steps: every step matches the
    reference (R_s x0 is re-derived once after each switch)."""
    eng = _t2_engine(lr.T3_SHAPE, T3_K)
    seq = lr.t3_sequence("toggle")
    res = _run(eng, seq, T3_K, [True, False, True], pipe)
    _check_run(res, seq, T3_K, "toggle", "toggle")


@pytest.mark.parametrize("pipe", [True, False], ids=["pipe", "host"])
@pytest.mark.parametrize("rs", [True, False], ids=["carried", "direct"])
def test_zero_right_hand_side_for_one_cohort(rs, pipe):
    """r = 0, r1 = 0 and xhat1 = 0 for cohort 0 of two (their LD matrices
    differ): its xhat2 is exactly 0, XR = 0, Z = N; cohort 1 is bitwise what it is
    when cohort 0 is ordinary; the ordinary step that follows is right."""
    eng = _t2_engine(lr.T3_SHAPE, T3_K)
    seq = lr.t3_sequence("zero_rhs")
    res = _run(eng, seq, T3_K, [rs] * 2, pipe)
    r0 = res[0]
    assert not r0["x2"][0].any()
    assert r0["out"][0][lr.O_XR] == 0.0 and r0["out"][0][lr.O_XRX] == 0.0
    assert r0["out"][0][lr.O_Z] == seq["inp"][0][0]["N"]
    assert r0["cg"][0][:2].tolist() == [0, 0]
    _check_run(res, seq, T3_K, "rs" if rs else "direct", "zero rhs")
    # the same first call with an ordinary cohort 0 (xhat1 = 0 for both, as above)
    main = lr.sequence(lr.T3_SHAPE)
    ordinary = [dict(i, xhat1=np.zeros_like(i["xhat1"])) for i in main["inp"][0]]
    ordinary[1] = seq["inp"][0][1]
    other = _run(eng, seq, T3_K, [rs] * 2, pipe, ncall=1, inp_override={0: ordinary})[0]
    assert other["x2"][0].any()
    np.testing.assert_array_equal(other["out"][1], r0["out"][1])
    np.testing.assert_array_equal(other["cg"][1], r0["cg"][1])
    for key in ("x2", "s2u", "r1"):
        np.testing.assert_array_equal(other[key][1], r0[key][1], err_msg=key)


@pytest.mark.parametrize("pipe", [True, False], ids=["pipe", "host"])
def test_reset_solver_replays_the_sequence_bitwise(pipe):
    """Three steps on a new engine, reset_solver, the three steps again: bitwise
    the first run."""
    seq = lr.sequence(lr.T3_SHAPE)
    eng = _t2_engine(lr.T3_SHAPE, 3, fresh=True)
    try:
        first = _run(eng, seq, 3, [True] * 3, pipe, reset=False)
        second = _run(eng, seq, 3, [True] * 3, pipe)
    finally:
        eng.close()
    _same(first, second, "after reset_solver")


@pytest.mark.parametrize("exchange", [None, "host"], ids=["local", "rehearsal"])
def test_queued_metrics_and_argument_checks(exchange):
    """metrics_begin / metrics_end give metrics() and the integer sums of
    marker_ref's exact vectors; metrics_end without begin, and sgv_lmmse with a
    null pointer or cg_maxit < 0, return SGV_ERR_ARG and touch nothing."""
    sizes = mr.PARTS["mixed9"]
    M = sum(sizes)
    x, x0, sums = mr.exact_vectors(M, 7)
    eng = Engine(sizes, K=1, exchange=exchange)
    try:
        lib, h = eng.ctx.lib, eng.ctx.h
        four = np.zeros(4)
        assert lib.sgv_metrics_end(h, hb.dptr(four)) == -2      # nothing begun
        eng.set_vector(hb.VEC_XHAT1, 0, x)
        eng.set_vector(hb.VEC_X0, 0, x0)
        np.testing.assert_array_equal(eng.metrics(), sums)
        eng.metrics_begin()
        np.testing.assert_array_equal(eng.metrics_end(), sums)
        assert lib.sgv_metrics_end(h, hb.dptr(four)) == -2      # consumed
        assert lib.sgv_metrics_end(h, None) == -2
        eng.metrics_begin()
        eng.metrics_begin()                                      # begun twice: the last one counts
        np.testing.assert_array_equal(eng.metrics_end(), sums)

        r1 = np.arange(M, dtype=np.float64)
        x2 = np.ones(M)
        eng.set_vector(hb.VEC_R1, 0, r1)
        eng.set_vector(hb.VEC_XHAT2, 0, x2)
        one, half, out = np.ones(1), np.full(1, 0.5), np.full((1, hb.LMMSE_NOUT), 7.0)
        cg, passes = np.full((1, 4), 7, dtype=np.int32), np.full(1, 7, dtype=np.int32)
        u = np.ones((1, M), dtype=np.int8)
        good = [hb.dptr(one), hb.dptr(one), hb.dptr(half), hb.dptr(half),
                u.ctypes.data_as(hb._c_i8_p), 5, 1e-5, 1, 0.5, 1, hb.dptr(out), hb.iptr(cg),
                hb.iptr(passes)]
        bad = []
        for i in (0, 1, 2, 3, 4, 10, 11):
            a = list(good)
            a[i] = None
            bad.append(a)
        a = list(good)
        a[5] = -1
        bad.append(a)
        for a in bad:
            assert lib.sgv_lmmse(h, 0, *a) == -2, a
            assert b"sgv_lmmse" in lib.sgv_last_error(h)
        assert (out == 7.0).all() and (cg == 7).all() and passes[0] == 7
        np.testing.assert_array_equal(eng.get_vector(hb.VEC_R1, 0), r1)
        np.testing.assert_array_equal(eng.get_vector(hb.VEC_XHAT2, 0), x2)
    finally:
        eng.close()
