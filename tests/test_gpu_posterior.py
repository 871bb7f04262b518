"""The posterior gate: k_posterior (posterior.hip), sgv_posterior and the
SGV_STEP_POSTERIOR step flag against references that share neither its f64
arithmetic nor its summation order (tests/posterior_ref.py; premise proved on the
CPU by tests/test_posterior_ref.py).

  a  every KM instantiation and the cohort-group path, 1/2/3/8 slabs, every
     regime: lodds, pip, var, resp and the sums against the references, the count
     exactly; two cross-checks against kernels written independently
     (sgv_denoise's derivative sums, one sgv_em step);
  b  per-marker results independent of the partition, the sums exact on data
     whose sums do not depend on the order;
  c  the step flag: slot rows and res sums bitwise sgv_posterior's at the same
     state, on a chained pair of steps; everything else bitwise the unflagged run;
  d  the exact edges lam = 0 and lam = 1.

M = 1,793 over the blocks [1025, 1, 767]: a chunk boundary, a one-marker block and
a ragged chunk.  Tolerances: posterior_ref's rule, from the f64 restatement's own
distance on the very inputs.  Every figure is printed before it is asserted
(pytest -s); SGV_POSTERIOR_TOL=<file> appends the device's distances there."""
import os

import numpy as np
import pytest

import hip_backend as hb
from engine import Engine
from tests import marker_ref as mr
from tests import posterior_ref as pr

pytestmark = pytest.mark.gpu

EDGES = mr.PARTS["edges"]
M_EDGES = sum(EDGES)
THR = 0.95


def _engine(sizes, r1s, **kw):
    eng = Engine(sizes, K=r1s.shape[0], **kw)
    for k, r in enumerate(r1s):
        eng.set_vector(hb.VEC_R1, k, r)
    return eng


def _prior(c):
    return c["gam1s"], c["a"], c["lam"], c["omegas"], c["sigmas"]


def _as_got(p):
    """Engine.posterior's dict in posterior_ref.distances' layout."""
    return dict(lodds=p["lodds"], pip=p["pip"], var=p["var"], resp=p["resp"].T,
                sum_pip=p["sums"][0], sum_var=p["sums"][1], count=int(p["sums"][2]))


def _record(lines):
    path = os.environ.get("SGV_POSTERIOR_TOL")
    if path:
        with open(path, "a") as f:
            f.write("".join(l + "\n" for l in lines))


# ---------------------------------------------------------------------------
# a. against the references
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", mr.DEN_KS)
def test_posterior_vs_references(K):
    """Every DEN_CASES entry of K cohorts through Engine.posterior: each quantity
    within the rule's tolerance of its reference, the count exact (no reference
    pip lies within the pip tolerance of the threshold: asserted on the data), no
    NaN, finite log-odds at +-40 sd.  Then a_k gam1_k sum var against sgv_denoise's
    derivative sums within the sum of the two tolerances, and at K = 1 (a = [1])
    one sgv_em step's new lam against sum pip / M."""
    cases = [c for c in mr.DEN_CASES if c[2] == K]
    assert cases
    eng = None
    out = []
    for cs in cases:
        c, ref, f64, d = pr.case_reference(cs, M_EDGES, THR)
        if eng is None:
            eng = _engine(EDGES, c["r1s"])
        else:
            for k, r in enumerate(c["r1s"]):
                eng.set_vector(hb.VEC_R1, k, r)
        gam1s, a, lam, omegas, sigmas = _prior(c)
        p = eng.posterior(gam1s, a, lam, omegas, sigmas, THR, resp=True)
        got = _as_got(p)
        e = pr.distances(got, ref)
        for q in pr.QUANTITIES:
            line = "%-8s %-28s device %.3e (host %.3e, tol %.3e)" % (
                q, mr.case_id(cs), e[q], d[q], pr.tolerance(d[q]))
            print(line)
            out.append(line)
        for q in ("lodds", "pip", "var"):
            assert np.isfinite(p[q]).all(), (q, mr.case_id(cs))
        assert not np.isnan(p["resp"]).any()
        for q in pr.QUANTITIES:
            assert e[q] <= pr.tolerance(d[q]), (q, mr.case_id(cs), e[q], pr.tolerance(d[q]))
        assert pr.count_is_decided(ref, THR, pr.tolerance(d["pip"])), mr.case_id(cs)
        assert got["count"] == ref["count"], mr.case_id(cs)
        assert np.abs(p["resp"].sum(axis=0) - 1).max() <= 8 * 2.0 ** -52
        # cross-check 1: the denoiser's derivative sums are a_k gam1_k sum_m var_m
        dx, dd, post = mr.den_distances(c)
        der = eng.denoise(gam1s, a, lam, omegas, sigmas, rho=0.5, damp=False)
        ex = np.max(np.abs(a * gam1s * got["sum_var"] - der) / np.abs(der))
        tol = min(1e-11, pr.tolerance(d["sum_var"]) + mr.tolerance(dd, mr.CAP_DER))
        print("    a gam1 sum var vs sgv_denoise: %.3e (tol %.3e)" % (ex, tol))
        assert ex <= tol, (mr.case_id(cs), ex, tol)
        # cross-check 2: the EM step's new lam is mean_m pip_m at one cohort
        if K == 1:
            assert a.tolist() == [1.0]
            dl, _, _ = mr.em_distances(c)
            lam_em = eng.em(gam1s, a, sigmas, 1, lam, omegas)[0]
            el = abs(got["sum_pip"] / M_EDGES - lam_em) / lam_em
            tol = pr.tolerance(d["sum_pip"]) + mr.tolerance(dl, mr.CAP_X)
            print("    sum pip / M vs sgv_em's lam: %.3e (tol %.3e)" % (el, tol))
            assert el <= tol, (mr.case_id(cs), el, tol)
    eng.close()
    _record(out)


# ---------------------------------------------------------------------------
# b. partitions
# ---------------------------------------------------------------------------
PART_NAMES = ["one", "edges", "mixed9", "b17"]


def test_per_marker_outputs_are_partition_independent():
    """The first sum(P) of the same markers under each partition P: pip, lodds,
    var and resp bitwise those of one block holding them all."""
    M = sum(mr.PARTS["b17"])
    cs = ("late", 0, 4, 3)
    c = mr.case(cs, M)
    gam1s, a, lam, omegas, sigmas = _prior(c)
    eng = _engine([M], c["r1s"])
    whole = eng.posterior(gam1s, a, lam, omegas, sigmas, THR, resp=True)
    eng.close()
    _, ref, _, d = pr.case_reference(cs, M, THR)
    assert pr.dist_pip(whole["pip"], ref) <= pr.tolerance(d["pip"])
    for name in PART_NAMES:
        sizes = mr.PARTS[name]
        n = sum(sizes)
        eng = _engine(sizes, c["r1s"][:, :n])
        p = eng.posterior(gam1s, a, lam, omegas, sigmas, THR, resp=True)
        eng.close()
        for q in ("pip", "lodds", "var"):
            np.testing.assert_array_equal(p[q], whole[q][:n], err_msg="%s %s" % (name, q))
        np.testing.assert_array_equal(p["resp"], whole["resp"][:, :n], err_msg=name)


def _exact_case(M, seed):
    """Integer r1 of 16 .. 40 sd (K = 1, a = gam1 = sigma = 1, lam = 1/2): every pip
    is exactly 1 and every var exactly 1/2 in f64 -- asserted on the data with the
    restatement -- so the three sums are M, M / 2 and M in any order or grouping."""
    rs = np.random.RandomState([seed, M])
    r1 = rs.randint(16, 41, size=M).astype(np.float64) * rs.choice([-1.0, 1.0], size=M)
    c = dict(r1s=r1[None, :], gam1s=np.array([1.0]), a=np.array([1.0]), lam=0.5,
             omegas=np.array([1.0]), sigmas=np.array([1.0]))
    f64 = pr.kernel_f64(thr=1.0, **c)
    assert (f64["pip"] == 1.0).all() and (f64["var"] == 0.5).all() and f64["count"] == M
    assert np.isfinite(f64["lodds"]).all() and f64["lodds"].min() > 37.0
    assert M < mr.EXACT_LIMIT
    return c, np.array([float(M), M / 2.0, float(M)])


@pytest.mark.parametrize("exchange", [None, "host"], ids=["local", "rehearsal"])
@pytest.mark.parametrize("part", PART_NAMES)
def test_sums_exact_on_every_partition(part, exchange):
    """On data whose sums cannot depend on the order, the three sums are the
    exact integers (halves) on every partition, through k_reduce_local (one
    rank) and k_reduce_blocks + k_reduce_total (the one-rank exchange
    rehearsal): no chunk or block dropped, doubled or misplaced; threshold 1.0,
    so the count takes pip >= thr at equality."""
    sizes = mr.PARTS[part]
    c, sums = _exact_case(sum(sizes), 5)
    eng = _engine(sizes, c["r1s"], exchange=exchange)
    p = eng.posterior(*_prior(c), 1.0)
    eng.close()
    assert (p["pip"] == 1.0).all() and (p["var"] == 0.5).all()
    np.testing.assert_array_equal(p["sums"], sums)


def test_sums_bitwise_across_cuts_of_the_same_markers():
    """The same markers cut as b17, as mixed9 and a remainder, and as one block:
    the sums bitwise equal on the exact data; on drawn data within the
    tolerance of the reference."""
    M = sum(mr.PARTS["b17"])
    cuts = {"b17": mr.PARTS["b17"], "mixed9+rest": mr.PARTS["mixed9"] + [M - sum(mr.PARTS["mixed9"])],
            "one block": [M]}
    cx, sums = _exact_case(M, 9)
    cs = ("benign", 0, 4, 3)
    c, ref, _, d = pr.case_reference(cs, M, THR)
    for name, sizes in cuts.items():
        assert sum(sizes) == M
        eng = _engine(sizes, cx["r1s"])
        np.testing.assert_array_equal(eng.posterior(*_prior(cx), 1.0)["sums"], sums, err_msg=name)
        eng.close()
        eng = _engine(sizes, c["r1s"])
        s = eng.posterior(*_prior(c), THR)["sums"]
        eng.close()
        e = (pr.dist_sum(s[0], ref["sum_pip"]), pr.dist_sum(s[1], ref["sum_var"]))
        print(name, "sum pip %.3e sum var %.3e" % e)
        assert e[0] <= pr.tolerance(d["sum_pip"]) and e[1] <= pr.tolerance(d["sum_var"]), name
        assert int(s[2]) == ref["count"], name


# ---------------------------------------------------------------------------
# c. the step flag
# ---------------------------------------------------------------------------
def _problem(K, seed):
    """A small VAMP problem on the EDGES blocks: LD blocks, r_k, probes."""
    rs = np.random.RandomState(seed)
    N = 1500
    blocks = []
    for n in EDGES:
        X = rs.normal(size=(2 * n, n)) / np.sqrt(2 * n)
        blocks.append(X.T @ X)
    cm = M_EDGES // 20
    beta = np.zeros(M_EDGES)
    beta[rs.choice(M_EDGES, cm, replace=False)] = rs.normal(0, np.sqrt(0.6 / cm), cm)
    r = np.empty((K, M_EDGES))
    o = 0
    for B in blocks:
        n = B.shape[0]
        for k in range(K):
            r[k, o:o + n] = B @ (beta[o:o + n] * np.sqrt(N)) + rs.normal(size=n) * np.sqrt(0.4)
        o += n
    probes = [(rs.binomial(1, 0.5, size=(K, M_EDGES)) * 2 - 1).astype(np.int8) for _ in range(2)]
    return dict(K=K, N=N, blocks=blocks, r=r, probes=probes, sigmas=np.array([0.6 / cm * N]),
                a=np.full(K, 1.0 / K), x0=beta * np.sqrt(N))


def _step_engine(pb):
    K = pb["K"]
    eng = Engine(EDGES, K=K)
    for b, B in enumerate(pb["blocks"]):
        eng.set_ld_block(0, b, B)
    for k in range(K):
        eng.set_vector(hb.VEC_R, k, pb["r"][k])
        eng.set_vector(hb.VEC_R1, k, pb["r"][k])
        eng.set_cohort_n(k, pb["N"])
    eng.set_vector(hb.VEC_X0, 0, pb["x0"])
    return eng


def _run_pair(pb, post):
    """Two steps, the second chained behind the first, with or without the
    posterior flag; returns the steps' results and copies of their output slots."""
    K = pb["K"]
    eng = _step_engine(pb)
    if post:
        eng.set_posterior_outputs(True, THR)
    base = hb.STEP_LEARN_GAMW | hb.STEP_LMMSE_DAMP | hb.STEP_METRICS | \
        (hb.STEP_POSTERIOR if post else 0)
    f1 = base | hb.STEP_EM | hb.STEP_DENOISE_DAMP | hb.STEP_ALPHA1_DAMP | hb.STEP_CHAIN
    z = [0.0] * K
    args = (5, pb["sigmas"], pb["a"], 0.05, np.array([1.0]), np.full(K, 1e-6), 0.5, [2.0] * K, z, z)
    h0 = eng.step_begin(0, base, *args, pb["probes"][0], 200, 0)
    h1 = eng.step_begin(1, f1, *args, pb["probes"][1], 200, 1)
    res = [eng.step_end(h0), eng.step_end(h1)]
    slots = [eng.outputs_wait(s).copy() for s in (0, 1)]
    raw = [h0["res"].copy(), h1["res"].copy()]
    eng.close()
    return res, slots, raw


@pytest.mark.parametrize("K", [1, 2])
def test_step_flag_equals_sgv_posterior_and_changes_nothing_else(K):
    pb = _problem(K, 20 + K)
    res, slots, raw = _run_pair(pb, True)
    res0, slots0, raw0 = _run_pair(pb, False)
    gam1s = [np.full(K, 1e-6), res[0]["out"][:, hb.O_GAM1].copy()]
    for i in range(2):
        assert slots[i].shape == (K + 4, M_EDGES) and slots0[i].shape == (K + 1, M_EDGES)
        assert raw[i].shape == (1 + 2 * K + 4 + 3,) and raw0[i].shape == (1 + 2 * K + 4,)
        # everything the unflagged run computes, bitwise
        np.testing.assert_array_equal(slots[i][:K + 1], slots0[i])
        np.testing.assert_array_equal(raw[i][:1 + 2 * K + 4], raw0[i])
        assert np.isfinite(raw0[i]).all() and (raw0[i][1 + 2 * K:] != 0).all()   # the metrics
        np.testing.assert_array_equal(res[i]["out"], res0[i]["out"])
        np.testing.assert_array_equal(res[i]["cg"], res0[i]["cg"])
        assert res[i]["lam"] == res0[i]["lam"]
        np.testing.assert_array_equal(res[i]["omegas"], res0[i]["omegas"])
        # sgv_posterior at the step's state: the r1 the denoiser saw (the slot's
        # rows 1 .. K), its gam1s, the prior after the step's EM update
        eng = _engine(EDGES, slots[i][1:K + 1])
        p = eng.posterior(gam1s[i], pb["a"], res[i]["lam"], res[i]["omegas"], pb["sigmas"], THR)
        eng.close()
        for j, q in enumerate(("pip", "lodds", "var")):
            np.testing.assert_array_equal(slots[i][K + 1 + j], p[q], err_msg="step %d %s" % (i, q))
        np.testing.assert_array_equal(res[i]["posterior_sums"], p["sums"])
        assert 0.0 < p["sums"][0] < M_EDGES and np.isfinite(p["lodds"]).all()
    assert res[1]["em_steps"] >= 1 and res[0]["lam"] != res[1]["lam"]   # the prior moved


def test_step_flag_needs_the_slots_sized_first():
    """SGV_STEP_POSTERIOR without sgv_set_posterior_outputs fails, and sgv_posterior
    fails while a step is queued (as sgv_reset_solver does)."""
    pb = _problem(1, 31)
    eng = _step_engine(pb)
    args = (5, pb["sigmas"], pb["a"], 0.05, np.array([1.0]), np.array([1e-6]), 0.5, [2.0], [0.0],
            [0.0], pb["probes"][0], 200, 0)
    h = eng.step_begin(0, hb.STEP_POSTERIOR, *args)
    with pytest.raises(hb.HipError, match="sgv_set_posterior_outputs"):
        eng.step_end(h)
    h = eng.step_begin(0, 0, *args)
    with pytest.raises(hb.HipError, match="queued"):
        eng.posterior(np.array([1e-6]), pb["a"], 0.05, np.array([1.0]), pb["sigmas"])
    with pytest.raises(hb.HipError, match="queued"):
        eng.set_posterior_outputs(True, THR)
    eng.step_end(h)
    eng.set_posterior_outputs(True, THR)     # resizes the slot the step has used
    assert eng.posterior(np.array([1e-6]), pb["a"], 0.05, np.array([1.0]),
                         pb["sigmas"])["sums"][0] > 0
    eng.outputs_begin(0)
    assert eng.outputs_wait(0).shape == (1 + 4, M_EDGES)
    eng.close()


# ---------------------------------------------------------------------------
# d. exact edges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [0.0, 1.0])
@pytest.mark.parametrize("K,nslab", [(4, 3), (33, 2)])
def test_exact_edges(lam, K, nslab):
    """lam == 0: pip = 0, lodds = -inf, var = 0, count 0; lam == 1: pip = 1, lodds =
    +inf, var = the slab mixture's variance; resp the slabs' own mixture; no NaN."""
    c = dict(mr.case(("benign", 0, K, nslab), M_EDGES))
    c["lam"] = lam
    ref = pr.reference(thr=THR, **c)
    d = pr.distances(pr.kernel_f64(thr=THR, **c), ref)
    eng = _engine(EDGES, c["r1s"])
    p = eng.posterior(*_prior(c), THR, resp=True)
    eng.close()
    for q in ("pip", "lodds", "var", "resp", "sums"):
        assert not np.isnan(p[q]).any(), q
    assert (p["pip"] == lam).all()
    assert (p["lodds"] == (np.inf if lam else -np.inf)).all()
    e = pr.distances(_as_got(p), ref)
    print(lam, K, nslab, e)
    for q in pr.QUANTITIES:
        assert e[q] <= pr.tolerance(d[q]), (q, e[q])
    if lam == 0.0:
        assert (p["var"] == 0.0).all()
        np.testing.assert_array_equal(p["sums"], [0.0, 0.0, 0.0])
    else:
        assert (p["var"] > 0.0).all() and p["sums"][0] == M_EDGES and p["sums"][2] == M_EDGES
