"""Independent references of the marker-wise kernels (vec.hip), derived from the
model and not from the reference's expressions, in np.longdouble and the log
domain, vectorised over markers; plus the parameter regimes, the partitions and
the exact data the marker gate (tests/test_gpu_marker_kernels.py) runs on.
tests/test_marker_ref.py proves them against 50-digit arithmetic on the CPU.

The model.  A marker's effect x has the prior (1 - lam) delta_0 + lam sum_l
omega_l N(0, sigma_l).  A Gaussian observation t / G of x with precision G turns
component l (the spike is component 0: sigma_0 = 0, weight 1 - lam) into

    weight_l ~ w_l sqrt(q_l) exp(t^2 sigma_l q_l / 2),   q_l = 1 / (G sigma_l + 1),
    x | l    ~ N(t sigma_l q_l, sigma_l q_l).

* The meta denoiser observes K cohorts: G = sum_k a_k gam1_k, t = sum_k r1_k a_k
  gam1_k.  xhat1 is the mixture's mean; d xhat1 / d r1_k = a_k gam1_k Var(x | r1).
* The EM step and the MLE sums look at one cohort at a time: G = gam1_k, t = r1_k
  gam1_k; the weights are then the responsibilities of r1_k's marginal
  (1 - lam) N(0, 1/gam1_k) + lam sum_l omega_l N(0, sigma_l + 1/gam1_k).

Only ratios of weights are ever formed, each from ONE expression whose size is
the log-ratio itself,

    log(weight_l / weight_j) = log(w_l / w_j) + (t^2 / 2) q_l q_j (sigma_l - sigma_j)
                               + log(q_l / q_j) / 2,

(sigma_l q_l - sigma_j q_j = q_l q_j (sigma_l - sigma_j)), never as a difference
of two large exponents; t is a compensated dot product of the exact products
r1_k a_k gam1_k; the variance is the sum of the non-negative terms of the law of
total variance.  So the result carries a few longdouble roundings whatever the
regime (tails of 40 sd, slabs 1e-9 apart, lam next to 0 or 1).

Tolerance rule (the one place it is stated).  Per quantity and regime,

    tol = 8 * max(d, 2**-50),   d = the f64 oracle's distance from the reference
                                    on the very inputs of the test (CPU, numpy),

the factor 8 for the device's exp / sqrt differing from numpy's by an ulp and
another summation order; never more than CAP_X = 1e-12 (xhat1, EM, MLE) and
CAP_DER = 1e-11 (derivative sums), the bounds of test_denoise_and_em_vs_oracle.
tolerance() returns min(cap, tol): where the rule would ask for more than the
cap, the cap holds.  Distances: relative for sums of one sign (derivative, EM,
MLE); for xhat1 per marker against |xhat1| + Var(x | r1) sum_k |r1_k a_k gam1_k|,
the first-order effect of one relative rounding in t (with more than one cohort
the inner product can cancel; at a marker with xhat1 = 0 this is the absolute
part of the check).
"""
import numpy as np

L_ = np.longdouble
assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble is not extended precision here"

CAP_X = 1e-12
CAP_DER = 1e-11
TOL_FLOOR = 2.0 ** -50
TOL_FACTOR = 8.0


def tolerance(dist, cap):
    return min(cap, TOL_FACTOR * max(float(dist), TOL_FLOOR))


# ---------------------------------------------------------------------------
# error-free transforms in longdouble (64-bit significand: split at 32 bits)
# ---------------------------------------------------------------------------
_SPLIT = L_(2 ** 32 + 1)


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = _SPLIT * a
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _ag(a, gam1s):
    """a_k gam1_k exactly, as a (hi, lo) pair of longdoubles."""
    return _two_prod(np.asarray(a, dtype=L_), np.asarray(gam1s, dtype=L_))


def _dot_ag(r1s, a, gam1s):
    """sum_k r1_k a_k gam1_k per marker, compensated (the result of twice the
    working precision, rounded once), and sum_k |r1_k a_k gam1_k|."""
    hi, lo = _ag(a, gam1s)
    r = np.asarray(r1s, dtype=L_)
    s = np.zeros(r.shape[1], dtype=L_)
    e = np.zeros(r.shape[1], dtype=L_)
    sa = np.zeros(r.shape[1], dtype=L_)
    for k in range(r.shape[0]):
        p, pe = _two_prod(r[k], hi[k])
        s, se = _two_sum(s, p)
        e = e + (pe + se + r[k] * lo[k])
        sa = sa + np.abs(p)
    return s + e, sa


def _weights(t, G, sig, logw):
    """Normalised component weights p [..., L] (they sum to 1) of the mixture
    sum_l w_l N(0, sig_l) seen through t with precision G (module docstring);
    sig, logw: [L], t: any shape.  Also returns q [L]."""
    sig = np.asarray(sig, dtype=L_)
    logw = np.asarray(logw, dtype=L_)
    t = np.asarray(t, dtype=L_)
    q = 1 / (G * sig + 1)
    h = t * t / 2
    # the reference component: the largest weight (from the ratios against a
    # virtual sigma = 0 component; only its identity is used)
    j = np.argmax(logw + h[..., None] * (sig * q) + np.log(q) / 2, axis=-1)
    D = (logw - logw[j][..., None]) + (h * q[j])[..., None] * q * (sig - sig[j][..., None]) \
        + (np.log(q) - np.log(q[j])[..., None]) / 2
    E = np.exp(D)
    return E / E.sum(axis=-1, keepdims=True), q


def _mix(lam, omegas, sigmas):
    """(sig [L], logw [L]) of the prior with the spike as component 0."""
    lam = L_(lam)
    sig = np.concatenate([[L_(0)], np.asarray(sigmas, dtype=L_)])
    logw = np.concatenate([[np.log(1 - lam)], np.log(lam * np.asarray(omegas, dtype=L_))])
    return sig, logw


def posterior(r1s, gam1s, a, lam, omegas, sigmas):
    """Spike-and-slab posterior of the meta denoiser.  r1s [K][M].  Returns
    dict(mean [M] (xhat1), var [M], der [K] (cohort k's derivative sum: a_k
    gam1_k sum_m var_m), cond [M] (var_m sum_k |r1_km a_k gam1_k|)), longdouble."""
    hi, lo = _ag(a, gam1s)
    G = (hi + lo).sum()
    t, tabs = _dot_ag(r1s, a, gam1s)
    sig, logw = _mix(lam, omegas, sigmas)
    p, q = _weights(t, G, sig, logw)
    s2 = sig * q                                   # Var(x | l); E(x | l) = t s2_l
    mean = t * (p * s2).sum(axis=-1)
    # law of total variance: E Var(x | l) + Var E(x | l), every term >= 0;
    # E(x | l) - mean = sum_j p_j t q_l q_j (sig_l - sig_j)
    dlj = (q[:, None] * q[None, :]) * (sig[:, None] - sig[None, :])          # [L][L]
    dev = t[:, None] * (p[:, None, :] * dlj[None, :, :]).sum(axis=-1)        # [M][L]
    var = (p * s2).sum(axis=-1) + (p * dev * dev).sum(axis=-1)
    return dict(mean=mean, var=var, der=(hi + lo) * var.sum(), cond=var * tabs)


def _cohort_weights(r1k, gam1k, sig, logw):
    g = L_(gam1k)
    return _weights(np.asarray(r1k, dtype=L_) * g, g, sig, logw)[0]


def em_step(r1s, gam1s, a, lam, omegas, sigmas):
    """One EM step of the prior: with p_kml the responsibility of component l
    for r1_km and pi_km = sum_{l >= 1} p_kml,
      lam_new = mean_m sum_k a_k pi_km / sum_k a_k,
      omegas_new_l = sum_km a_k p_kml / sum_km a_k pi_km
    (prior_update_em: pi xi_tilde = p).  Returns (lam_new, omegas_new), longdouble."""
    sig, logw = _mix(lam, omegas, sigmas)
    aL = np.asarray(a, dtype=L_)
    K, M = np.shape(r1s)
    num = np.zeros(len(sig) - 1, dtype=L_)
    den = L_(0)
    for k in range(K):
        p = _cohort_weights(r1s[k], gam1s[k], sig, logw)[:, 1:]
        num = num + aL[k] * p.sum(axis=0)
        den = den + aL[k] * p.sum()
    return den / aL.sum() / M, num / den


def mle_sums(r1s, gam1s, a, sigma2, omega):
    """S_l = sum_km a_k f_kml / sum_j omega_j f_kmj, f_kml = N(r1_km; 0, sigma2_l +
    1/gam1_k), l = 0 .. L-1 (Lagrangian_der's sums; sigma2[0] is the spike's
    1e-16).  Ratios f_l / f_j per (k, m), so no global shift enters."""
    sig = np.asarray(sigma2, dtype=L_)
    om = np.asarray(omega, dtype=L_)
    aL = np.asarray(a, dtype=L_)
    S = np.zeros(len(sig), dtype=L_)
    for k in range(np.shape(r1s)[0]):
        p = _cohort_weights(r1s[k], gam1s[k], sig, np.log(om))   # omega_l f_l / sum_j omega_j f_j
        S = S + aL[k] * (p / om).sum(axis=0)
    return S


# ---------------------------------------------------------------------------
# distances (module docstring)
# ---------------------------------------------------------------------------
def dist_rel(x, ref):
    ref = np.asarray(ref, dtype=L_)
    return float(np.max(np.abs(np.asarray(x, dtype=L_) - ref) / np.abs(ref)))


def dist_xhat(x, post):
    """max_m |x_m - mean_m| / (|mean_m| + cond_m); 0 / 0 counts as 0."""
    err = np.abs(np.asarray(x, dtype=L_) - post["mean"])
    scale = np.abs(post["mean"]) + post["cond"]
    out = np.zeros(err.shape, dtype=L_)
    nz = scale > 0
    out[nz] = err[nz] / scale[nz]
    out[~nz & (err > 0)] = np.inf
    return float(out.max())


# ---------------------------------------------------------------------------
# exact data for the ordered reductions
# ---------------------------------------------------------------------------
EXACT_LIMIT = float(2 ** 52)


def exact_vectors(M, seed, bits=16):
    """Integer-valued f64 (x, x0) [M], |v| < 2**bits, and the four sums the
    metrics kernel forms, <x, x0>, |x|^2, |x - x0|^2, |x0|^2, as exact integers
    in f64.  The absolute values of each sum's terms add up to less than 2**52
    (asserted here, on the very data), so every partial sum in any order or
    grouping is an exactly representable integer."""
    rs = np.random.RandomState([int(seed) & 0x7FFFFFFF, int(M), int(bits)])
    m = (1 << bits) - 1
    x = rs.randint(-m, m + 1, size=M).astype(np.float64)
    x0 = rs.randint(-m, m + 1, size=M).astype(np.float64)
    d = x - x0
    terms = [x * x0, x * x, d * d, x0 * x0]
    for t in terms:
        assert np.array_equal(t, np.rint(t)) and np.abs(t).sum() < EXACT_LIMIT
    return x, x0, np.array([t.sum() for t in terms])


# ---------------------------------------------------------------------------
# partitions (LD block sizes)
# ---------------------------------------------------------------------------
_CYCLE = [1, 255, 256, 257, 1023, 1024, 1025, 2049]


def _mixed(n):
    return [_CYCLE[i % len(_CYCLE)] for i in range(n)]


PARTS = {
    "edges": [1025, 1, 767],
    "mixed8": _mixed(8),       # 8 blocks: the last count whose CG control is fused
    "mixed9": _mixed(9),       # the first on k_reduce_local + k_cg_ctl
    "mixed12": _mixed(12),     # the last count whose EM control is fused
    "mixed13": _mixed(13),     # the first on k_reduce_local + k_em_ctl
    "b17": _mixed(17),         # more blocks than k_reduce_local has waves
    "b1025": [1 + i % 3 for i in range(1025)],   # a second batch of 1,024 blocks
    "c64": [65536, 300],       # exactly 64 chunks: one lane round
    "c65": [65537, 300],       # 65 chunks: lane 0 takes a second one
    "one": [1],
}


# ---------------------------------------------------------------------------
# regimes
# ---------------------------------------------------------------------------
HEAD = np.array([0.0, 1e-8, 1.0, 5.0, 10.0, 20.0, 40.0, -40.0])
MLE_TAIL = 30.0     # cap of the planted |z| in the MLE cases (case())


def _geom(lo, hi, n):
    return np.array([hi]) if n == 1 else np.geomspace(lo, hi, n)


REGIMES = {
    # test_denoise_and_em_vs_oracle's
    "benign": dict(gam1=lambda rs, K: rs.uniform(0.5, 3.0, K),
                   sig=lambda rs, n: np.sort(rs.uniform(1.0, 50.0, n)), lams=(0.12,)),
    # a run's first iteration: gam1 = 1e-6 in every cohort
    "first_iter": dict(gam1=lambda rs, K: np.full(K, 1e-6),
                       sig=lambda rs, n: _geom(1e-4, 1e-2, n), lams=(0.1,)),
    "late": dict(gam1=lambda rs, K: np.geomspace(8e2, 1e4, K) if K > 1 else np.array([3e3]),
                 sig=lambda rs, n: _geom(1e-5, 1e-2, n), lams=(0.01,)),
    "late_big": dict(gam1=lambda rs, K: np.geomspace(1e5, 3e5, K) if K > 1 else np.array([2e5]),
                     sig=lambda rs, n: np.array([1e-5, 1e-2, 1e-4, 1e-3, 3e-5, 3e-3, 3e-4,
                                                 5e-3][:n]) if n > 1 else np.array([1e-2]),
                     lams=(1e-3,)),
    # argmax ties and the cancelling exponent
    "near_equal_slabs": dict(gam1=lambda rs, K: rs.uniform(5e2, 2e3, K),
                             sig=lambda rs, n: 1e-3 * (1.0 + np.array(
                                 [0.0, 1e-9, 1e-7, 1e-5, 3e-9, 3e-7, 1e-8, 1e-6][:n])),
                             lams=(0.05,)),
    "lam_edge": dict(gam1=lambda rs, K: rs.uniform(50.0, 500.0, K),
                     sig=lambda rs, n: _geom(1e-3, 1e-1, n), lams=(1.0 - 1e-12, 1e-12)),
}


def regime_cases():
    """(regime, index into its lams) for every named parameter set."""
    return [(name, i) for name, r in REGIMES.items() for i in range(len(r["lams"]))]


def draw(regime, K, nslab, M, seed=0, lam_index=0, tail=None):
    """Inputs of one case: dict(r1s [K][M], gam1s, a, lam, omegas, sigmas).
    Cohorts get distinct a_k, r1_k (and gam1_k where the regime allows), so a
    swapped or dropped cohort shows.  The first min(M, 8) markers of every
    cohort are HEAD x scale_k, scale_k = 1 / sqrt(gam1_k), the sd of r1_k's noise:
    HEAD is the marker's z-score r1_k sqrt(gam1_k) in every cohort; tail: cap of
    |HEAD| (the MLE cases, see case())."""
    R = REGIMES[regime]
    rs = np.random.RandomState([sum(map(ord, regime)), K, nslab, M, seed, lam_index])
    gam1s = np.asarray(R["gam1"](rs, K), dtype=np.float64)
    sigmas = np.asarray(R["sig"](rs, nslab), dtype=np.float64)
    lam = float(R["lams"][lam_index])
    a = rs.uniform(1.0, 2.0, K)
    a /= a.sum()
    omegas = rs.uniform(0.5, 1.0, nslab)
    omegas /= omegas.sum()
    # effects from the prior (at least a twentieth of them non-zero), noise 1/gam1_k
    slab = rs.randint(0, nslab, M)
    x = rs.normal(size=M) * np.sqrt(sigmas[slab]) * (rs.uniform(size=M) < min(max(lam, 0.05), 0.5))
    r1s = x[None, :] + rs.normal(size=(K, M)) / np.sqrt(gam1s)[:, None]
    scale = 1.0 / np.sqrt(gam1s)
    head = HEAD if tail is None else np.clip(HEAD, -tail, tail)
    n = min(M, len(head))
    r1s[:, :n] = head[None, :n] * scale[:, None]
    return dict(r1s=r1s, gam1s=gam1s, a=a, lam=lam, omegas=omegas, sigmas=sigmas)


def mle_inputs(c):
    """(sigma2, omega) of Lagrangian_der at the prior of case c: the spike first,
    with the reference's variance 1e-16."""
    return (np.concatenate([[1e-16], c["sigmas"]]),
            np.concatenate([[1.0 - c["lam"]], c["lam"] * c["omegas"]]))


# ---------------------------------------------------------------------------
# the f64 oracle against the references (the distances of the tolerance rule)
# ---------------------------------------------------------------------------
def _vo():
    from oracle import vamp_oracle
    return vamp_oracle


def den_distances(c):
    """The f64 oracle's distances from the reference on case c's inputs:
    (xhat1, derivative sums), finite asserted."""
    x = _vo().denoiser_meta(**c)
    der = _vo().der_denoiser_meta(**c).sum(axis=1)
    assert np.isfinite(x).all() and np.isfinite(der).all()
    post = posterior(**c)
    return dist_xhat(x, post), dist_rel(der, post["der"]), post


def em_distances(c):
    lam, om = _vo().prior_update_em(c["r1s"], c["gam1s"], c["a"], c["lam"], c["omegas"], c["sigmas"])
    assert np.isfinite(lam) and np.isfinite(om).all()
    ref = em_step(**c)
    return dist_rel(lam, ref[0]), dist_rel(om, ref[1]), ref


def mle_oracle_sums(c):
    """(exp_max, S) as Lagrangian_der forms them (its residual less the terms
    added to the sums), on the oracle."""
    sigma2, omega = mle_inputs(c)
    em = _vo().mle_exp_max(c["r1s"], c["gam1s"], sigma2)
    x = np.concatenate([omega, [0.0]])
    omega0 = np.ones(len(omega))              # (omega0 - 1) / omega = 0, gam = 0: y[:L] = S
    y = _vo().lagrangian_der(x, omega0, sigma2, c["r1s"], c["gam1s"], c["a"], em)
    return em, y[:len(omega)]


def mle_distance(c):
    em, S = mle_oracle_sums(c)
    assert np.isfinite(em) and np.isfinite(S).all(), "the reference's own formula is not finite"
    sigma2, omega = mle_inputs(c)
    ref = mle_sums(c["r1s"], c["gam1s"], c["a"], sigma2, omega)
    return dist_rel(S, ref), ref


# ---------------------------------------------------------------------------
# the gate's cases, shared by the CPU premise test and the GPU gate
# ---------------------------------------------------------------------------
DEN_KS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65]   # every L_DEN arm, both bounds; 2, 3 groups


def _den_cases():
    out = [("late", 0, K, 3) for K in DEN_KS]
    out += [("late", 0, K, n) for K in (2, 16, 33) for n in (1, 2, 3, 8)]
    out += [(r, i, K, 3) for r, i in regime_cases() for K in (1, 4, 33)]
    return list(dict.fromkeys(out))


DEN_CASES = _den_cases()                                   # (regime, lam index, K, slabs)
# (K, slabs) reaching each EM_DISPATCH arm, then 2 and 3 cohort groups
EM_KL = [(1, 1), (1, 3), (4, 2), (3, 8), (8, 2), (8, 8), (16, 2), (16, 3), (32, 2), (32, 8),
         (33, 2), (65, 3)]
EM_CASES = list(dict.fromkeys([("late", 0, K, n) for K, n in EM_KL] +
                              [(r, i, K, n) for r, i in regime_cases() for K, n in ((4, 2), (33, 2))]))
MLE_KS, MLE_LS = [1, 12, 32, 33, 65], [2, 4, 9]            # L counts the spike
MLE_CASES = list(dict.fromkeys([("late", 0, K, L - 1) for K in MLE_KS for L in MLE_LS] +
                               [(r, i, 12, 3) for r, i in regime_cases()]))


def case_id(c):
    return "%s%s-K%d-L%d" % (c[0], "" if len(REGIMES[c[0]]["lams"]) == 1 else c[1], c[2], c[3])


_CASES = {}


def case(c, M, mle=False):
    """The inputs of case c at M markers (drawn once per process and shared: do
    not write to them); mle: the planted tail capped at |z| = MLE_TAIL -- the
    reference's global exp_max is 0 here (the planted r1 = 0), so where gam1
    sigma << 1 a marker at |z| > 38.6 underflows every component and its own
    formula is 0 / 0."""
    key = (c, M, mle)
    if key not in _CASES:
        regime, li, K, nslab = c
        d = draw(regime, K, nslab, M, lam_index=li, tail=MLE_TAIL if mle else None)
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CASES[key] = d
    return _CASES[key]
