"""The premise of the marker gate (tests/marker_ref.py), proved on the CPU:
the longdouble references agree with a 50-digit evaluation of the model's own
formulas, the f64 oracle is finite on every case the GPU gate runs and its
distance from the reference (which sets the gate's tolerances) is measured, and
the exact vectors' sums do not depend on the order.

SGV_MARKER_TOL=<file>: the measured distances and the tolerances the rule
derives from them are appended there (profiles/marker_gate/tolerances.txt)."""
import os

import mpmath
import numpy as np
import pytest

from tests import marker_ref as mr

mp = mpmath.mp
BOUND = 2.0 ** -58
M_EDGES = sum(mr.PARTS["edges"])


def _mpf(v):
    return [mpmath.mpf(float(x)) for x in np.ravel(v)]


def _close(x, ref):
    """|x - ref| <= 2**-58 |ref| for a longdouble x and an mpf ref."""
    hi = float(x)                                   # x = hi + lo exactly (64 = 53 + 11 bits)
    lo = float(np.longdouble(x) - np.longdouble(hi))
    assert np.longdouble(hi) + np.longdouble(lo) == x
    return abs(mpmath.mpf(hi) + mpmath.mpf(lo) - ref) <= BOUND * abs(ref)


def _mp_posterior(c):
    """Direct evaluation: weights lam omega_l N(t / G; 0, sigma_l + 1 / G) up to the
    common factor, W_l = lam omega_l sqrt(s2_l / sigma_l) exp(mu_l^2 / (2 s2_l))."""
    K, M = c["r1s"].shape
    a, g, om, sg = _mpf(c["a"]), _mpf(c["gam1s"]), _mpf(c["omegas"]), _mpf(c["sigmas"])
    lam = mpmath.mpf(c["lam"])
    ag = [a[k] * g[k] for k in range(K)]
    G = mpmath.fsum(ag)
    mean, var = [], []
    for m in range(M):
        t = mpmath.fsum(mpmath.mpf(float(c["r1s"][k, m])) * ag[k] for k in range(K))
        s2 = [1 / (G + 1 / s) for s in sg]
        mu = [t * s for s in s2]
        W = [lam * om[l] * mpmath.sqrt(s2[l] / sg[l]) * mpmath.exp(mu[l] ** 2 / (2 * s2[l]))
             for l in range(len(sg))]
        Z = (1 - lam) + mpmath.fsum(W)
        e1 = mpmath.fsum(W[l] * mu[l] for l in range(len(sg))) / Z
        e2 = mpmath.fsum(W[l] * (mu[l] ** 2 + s2[l]) for l in range(len(sg))) / Z
        mean.append(e1)
        var.append(e2 - e1 ** 2)
    return mean, var, [ag[k] * mpmath.fsum(var) for k in range(K)]


def _mp_density(r, v):
    return mpmath.exp(-r * r / (2 * v)) / mpmath.sqrt(v)


def _mp_em(c):
    K, M = c["r1s"].shape
    a, g, om, sg = _mpf(c["a"]), _mpf(c["gam1s"]), _mpf(c["omegas"]), _mpf(c["sigmas"])
    lam = mpmath.mpf(c["lam"])
    num = [mpmath.mpf(0)] * len(sg)
    den = mpmath.mpf(0)
    for k in range(K):
        for m in range(M):
            r = mpmath.mpf(float(c["r1s"][k, m]))
            xi = [lam * om[l] * _mp_density(r, sg[l] + 1 / g[k]) for l in range(len(sg))]
            tot = (1 - lam) * _mp_density(r, 1 / g[k]) + mpmath.fsum(xi)
            num = [num[l] + a[k] * xi[l] / tot for l in range(len(sg))]
            den += a[k] * mpmath.fsum(xi) / tot
    return den / mpmath.fsum(a) / M, [n / den for n in num]


def _mp_mle(c, sigma2, omega):
    K, M = c["r1s"].shape
    a, g, om, sg = _mpf(c["a"]), _mpf(c["gam1s"]), _mpf(omega), _mpf(sigma2)
    S = [mpmath.mpf(0)] * len(sg)
    for k in range(K):
        for m in range(M):
            r = mpmath.mpf(float(c["r1s"][k, m]))
            f = [_mp_density(r, s + 1 / g[k]) for s in sg]
            D = mpmath.fsum(om[l] * f[l] for l in range(len(sg)))
            S = [S[l] + a[k] * f[l] / D for l in range(len(sg))]
    return S


@pytest.mark.parametrize("K,nslab", [(1, 1), (4, 3), (3, 8), (33, 2)])
@pytest.mark.parametrize("regime,li", mr.regime_cases())
def test_references_agree_with_50_digits(regime, li, K, nslab):
    """posterior, em_step and mle_sums within 2**-58 relative of mpmath at 50
    digits on 64 markers, the planted head (0 .. +-40 sd) among them."""
    mp.dps = 50
    c = mr.draw(regime, K, nslab, 64, seed=1, lam_index=li)
    post = mr.posterior(**c)
    mean, var, der = _mp_posterior(c)
    for m in range(64):
        assert _close(post["mean"][m], mean[m]), ("mean", m)
        assert _close(post["var"][m], var[m]), ("var", m)
    assert post["mean"][0] == 0 and mean[0] == 0          # the planted r1 = 0
    for k in range(K):
        assert _close(post["der"][k], der[k]), ("der", k)
    lam_l, om_l = mr.em_step(**c)
    lam_m, om_m = _mp_em(c)
    assert _close(lam_l, lam_m)
    for l in range(nslab):
        assert _close(om_l[l], om_m[l]), ("omega", l)
    sigma2, omega = mr.mle_inputs(c)
    S_l = mr.mle_sums(c["r1s"], c["gam1s"], c["a"], sigma2, omega)
    S_m = _mp_mle(c, sigma2, omega)
    for l in range(nslab + 1):
        assert _close(S_l[l], S_m[l]), ("S", l)


def _record(lines):
    path = os.environ.get("SGV_MARKER_TOL")
    if path:
        with open(path, "a") as f:
            f.write("".join(l + "\n" for l in lines))


def test_oracle_distances_set_the_tolerances():
    """On every case of the GPU gate the f64 oracle is finite; its distance
    from the reference is printed and (SGV_MARKER_TOL) recorded with the
    tolerance the rule derives.  The rule is satisfiable by the oracle itself:
    every distance is within its cap / 8."""
    out = ["# quantity case distance tolerance"]
    worst = {}

    def note(q, c, d, cap):
        out.append("%-8s %-28s %.3e %.3e" % (q, mr.case_id(c), d, mr.tolerance(d, cap)))
        worst[q] = max(worst.get(q, 0.0), d)
        assert d <= cap / mr.TOL_FACTOR, (q, mr.case_id(c), d)

    for c in mr.DEN_CASES:
        dx, dd, _ = mr.den_distances(mr.case(c, M_EDGES))
        note("xhat1", c, dx, mr.CAP_X)
        note("der", c, dd, mr.CAP_DER)
    for c in mr.EM_CASES:
        dl, do, _ = mr.em_distances(mr.case(c, M_EDGES))
        note("em_lam", c, dl, mr.CAP_X)
        note("em_om", c, do, mr.CAP_X)
    for c in mr.MLE_CASES:
        d, _ = mr.mle_distance(mr.case(c, M_EDGES, mle=True))
        note("mle_S", c, d, mr.CAP_X)
    out.append("# worst: " + ", ".join("%s %.3e" % kv for kv in sorted(worst.items())))
    print("\n".join(out))
    _record(out)


def test_uncapped_tail_breaks_the_reference_mle_formula():
    """Why the MLE cases cap the planted tail: at |z| = 40 the reference's own
    formula (global exp_max, attained at the planted r1 = 0) is 0 / 0."""
    c = mr.case(("first_iter", 0, 12, 3), M_EDGES)
    with np.errstate(all="ignore"):
        _, S = mr.mle_oracle_sums(c)
    assert not np.isfinite(S).all()


@pytest.mark.parametrize("part", list(mr.PARTS))
def test_exact_vectors_sums_are_order_independent(part):
    """The metrics sums of exact_vectors over every partition's marker count:
    unchanged under random permutations, chunked sums and in longdouble."""
    M = sum(mr.PARTS[part])
    x, x0, sums = mr.exact_vectors(M, 7)
    rs = np.random.RandomState(3)
    L = np.longdouble

    def four(a, b, dt):
        a, b = a.astype(dt), b.astype(dt)
        return np.array([(a * b).sum(), (a * a).sum(), ((a - b) * (a - b)).sum(), (b * b).sum()])

    for _ in range(3):
        p = rs.permutation(M)
        np.testing.assert_array_equal(four(x[p], x0[p], np.float64), sums)
        cut = np.sort(rs.choice(np.arange(1, M), size=min(9, M - 1), replace=False)) if M > 1 \
            else np.array([], dtype=int)
        parts = [four(x[q], x0[q], np.float64) for q in np.split(p, cut)]
        np.testing.assert_array_equal(sum(parts[::-1]), sums)
    assert np.array_equal(four(x, x0, L), sums.astype(L))
    # sequential f64 accumulation, the order a single thread would use
    np.testing.assert_array_equal(np.cumsum(x * x)[-1], sums[1])
    assert sums[1] > 0 and (M == 1 or len(set(np.abs(x))) > 1)


def test_partitions_cross_the_loop_bounds():
    P = mr.PARTS
    assert [len(P[k]) for k in ("mixed8", "mixed9", "mixed12", "mixed13", "b17", "b1025")] == \
        [8, 9, 12, 13, 17, 1025]
    assert -(-P["c64"][0] // 1024) == 64 and -(-P["c65"][0] // 1024) == 65
    assert set(P["b1025"]) == {1, 2, 3}
