"""The premise of the posterior gate (tests/posterior_ref.py), proved on the CPU:
the longdouble references of lodds, pip, var, resp and kappa3 agree with a
50-digit evaluation of the model's own formulas on the planted head markers (0
.. +-40 sd) of every regime; the f64 restatement of the kernel's expressions is
within cap / 8 of the references on every case the GPU gate runs (so the rule's
tolerance is reachable); and the exact edges lam = 0 and lam = 1 are defined.

SGV_POSTERIOR_TOL=<file>: the measured host distances and the tolerances the
rule derives are appended there (profiles/posterior/tolerances.txt)."""
import os

import mpmath
import numpy as np
import pytest

from tests import marker_ref as mr
from tests import posterior_ref as pr

mp = mpmath.mp
BOUND = 2.0 ** -58
EDGES = mr.PARTS["edges"]
M_EDGES = sum(EDGES)


def _mpf(v):
    return [mpmath.mpf(float(x)) for x in np.ravel(v)]


def _ld(x):
    """A longdouble as an exact mpf: the mantissa in two f64 pieces (64 = 53 + 11
    bits), the exponent apart (1 - pip lies below f64's range at 40 sd)."""
    m, e = np.frexp(np.longdouble(x))
    hi = float(m)
    lo = float(m - np.longdouble(hi))
    assert np.longdouble(hi) + np.longdouble(lo) == m
    return mpmath.ldexp(mpmath.mpf(hi) + mpmath.mpf(lo), int(e))


def _mp_marker(c, m, dps):
    """Direct evaluation at one marker: slab weights W_l = lam omega_l sqrt(q_l)
    exp(h s2_l) against the spike's 1 - lam; raw moments of the mixture."""
    with mp.workdps(dps):
        K = c["r1s"].shape[0]
        a, g, om, sg = _mpf(c["a"]), _mpf(c["gam1s"]), _mpf(c["omegas"]), _mpf(c["sigmas"])
        lam = mpmath.mpf(c["lam"])
        ag = [a[k] * g[k] for k in range(K)]
        G = mpmath.fsum(ag)
        t = mpmath.fsum(mpmath.mpf(float(c["r1s"][k, m])) * ag[k] for k in range(K))
        n = len(sg)
        q = [1 / (G * s + 1) for s in sg]
        s2 = [sg[l] * q[l] for l in range(n)]
        h = t * t / 2
        W = [lam * om[l] * mpmath.sqrt(q[l]) * mpmath.exp(h * s2[l]) for l in range(n)]
        SW = mpmath.fsum(W)
        Z = (1 - lam) + SW
        mu = [t * s for s in s2]
        e1 = mpmath.fsum(W[l] * mu[l] for l in range(n)) / Z
        e2 = mpmath.fsum(W[l] * (mu[l] ** 2 + s2[l]) for l in range(n)) / Z
        # central third moment from the deviations (the spike: mean 0, variance 0)
        p = [(1 - lam) / Z] + [w / Z for w in W]
        dev = [-e1] + [mu[l] - e1 for l in range(n)]
        v = [mpmath.mpf(0)] + s2
        k3t = [p[l] * (dev[l] ** 3 + 3 * dev[l] * v[l]) for l in range(n + 1)]
        A = max(abs(mpmath.log(lam * om[l] / (1 - lam))) + abs(h * s2[l]) + abs(mpmath.log(q[l]) / 2)
                for l in range(n))
        return dict(lodds=mpmath.log(SW / (1 - lam)), pip=SW / Z, omp=(1 - lam) / Z,
                    var=e2 - e1 ** 2, resp=[w / SW for w in W], k3=mpmath.fsum(k3t),
                    k3abs=mpmath.fsum(abs(x) for x in k3t), A=A)


@pytest.mark.parametrize("K,nslab", [(1, 1), (4, 3), (3, 8), (33, 2)])
@pytest.mark.parametrize("regime,li", mr.regime_cases())
def test_references_agree_with_50_digits(regime, li, K, nslab):
    """lodds, pip, 1 - pip, var and resp within 2**-58 of mpmath at 50 digits, each on
    its own scale without the t part (t is formed exactly on both sides); kappa3
    (at 450 digits: it cancels down to the spike's 1e-347 at 40 sd) within 2**-58
    of the sum of its terms' absolute values; on the 8 planted head markers and 8
    drawn ones."""
    mp.dps = 50
    c = mr.draw(regime, K, nslab, 16, seed=1, lam_index=li)
    ref = pr.reference(**c)
    for m in range(16):
        x = _mp_marker(c, m, 50)
        S = abs(x["lodds"]) + x["A"]
        assert abs(_ld(ref["lodds"][m]) - x["lodds"]) <= BOUND * S, ("lodds", m)
        assert abs(_ld(ref["pip"][m]) - x["pip"]) <= BOUND * x["pip"] * (1 + x["omp"] * S), ("pip", m)
        assert abs(_ld(ref["omp"][m]) - x["omp"]) <= BOUND * x["omp"] * (1 + x["pip"] * S), ("omp", m)
        assert abs(_ld(ref["var"][m]) - x["var"]) <= BOUND * x["var"], ("var", m)
        assert abs(_ld(ref["A"][m]) - x["A"]) <= BOUND * x["A"], ("A", m)
        for l in range(nslab):
            assert abs(_ld(ref["resp"][m, l]) - x["resp"][l]) <= \
                BOUND * x["resp"][l] * (1 + x["A"]) + mpmath.mpf(2) ** -970, ("resp", m, l)
        y = _mp_marker(c, m, 450)
        # (a scale of the var distance only; the weights carry A roundings)
        assert abs(_ld(ref["k3"][m]) - y["k3"]) <= BOUND * y["k3abs"] * (1 + y["A"]), ("k3", m)
    assert np.isfinite(ref["lodds"].astype(np.float64)).all()
    # the moments are marker_ref.posterior's
    post = mr.posterior(**c)
    assert np.array_equal(ref["var"], post["var"])


def _record(lines):
    path = os.environ.get("SGV_POSTERIOR_TOL")
    if path:
        with open(path, "a") as f:
            f.write("".join(l + "\n" for l in lines))


def test_restatement_distances_set_the_tolerances():
    """On every case of the GPU gate, at its M and partition, the f64 restatement
    is finite and within cap / 8 of the reference in every quantity (the rule's
    tolerance is reachable), its count equals the reference's, and no reference
    pip lies within the pip tolerance of the threshold."""
    out = ["# host: the f64 restatement's distance d, tol = min(1e-12, 8 max(d, 2**-50))",
           "# quantity case distance tolerance"]
    worst = {}
    for cs in mr.DEN_CASES:
        c, ref, f64, d = pr.case_reference(cs, M_EDGES)
        for q in ("lodds", "pip", "var", "resp"):
            assert np.isfinite(f64[q]).all(), (q, mr.case_id(cs))
        for q in pr.QUANTITIES:
            out.append("%-8s %-28s %.3e %.3e" % (q, mr.case_id(cs), d[q], pr.tolerance(d[q])))
            worst[q] = max(worst.get(q, 0.0), d[q])
            assert d[q] <= pr.CAP / mr.TOL_FACTOR, (q, mr.case_id(cs), d[q])
        assert pr.count_is_decided(ref, 0.95, pr.tolerance(d["pip"])), mr.case_id(cs)
        assert f64["count"] == ref["count"], mr.case_id(cs)
        # the planted tail: pip rounds to 1 in f64, the log-odds stay finite
        assert f64["pip"][6] == 1.0 or ref["omp"][6] > 2.0 ** -54
        assert np.isfinite(f64["lodds"]).all()
    out.append("# worst host: " + ", ".join("%s %.3e" % kv for kv in sorted(worst.items())))
    print("\n".join(out))
    _record(out)


@pytest.mark.parametrize("lam", [0.0, 1.0])
def test_exact_edges(lam):
    """lam == 0: pip = 0, lodds = -inf, var = 0; lam == 1: pip = 1, lodds = +inf, var =
    the slab mixture's variance; resp sums to 1; no NaN in reference or restatement."""
    c = dict(mr.case(("benign", 0, 4, 3), 64))
    c["lam"] = lam
    ref = pr.reference(**c)
    f64 = pr.kernel_f64(**c)
    for d in (ref, f64):
        for q in ("lodds", "pip", "var", "resp"):
            assert not np.isnan(np.asarray(d[q], dtype=np.float64)).any(), q
        assert (d["pip"] == lam).all()
        assert (d["lodds"] == (np.inf if lam else -np.inf)).all()
        assert np.abs(np.asarray(d["resp"], dtype=np.float64).sum(axis=-1) - 1).max() < 1e-15
    if lam == 0.0:
        assert (f64["var"] == 0).all() and f64["count"] == 0
    else:
        assert (f64["var"] > 0).all() and f64["count"] == 64
        # the slab-only mixture: Var(x | r1) with the spike's weight exactly 0
        near = dict(c, lam=1.0 - 2.0 ** -53)
        assert mr.dist_rel(ref["var"], pr.reference(**near)["var"]) < 1e-12
    dist = pr.distances(f64, ref)
    print(lam, dist)
    assert max(dist.values()) <= pr.CAP / mr.TOL_FACTOR
