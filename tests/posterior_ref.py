"""References of the per-marker posterior outputs (posterior.hip: pip, lodds,
var, resp and their sums), in np.longdouble and the log domain, built on
tests/marker_ref.py's model pieces (_dot_ag, _mix, _weights, posterior); a plain
f64 NumPy restatement of the kernel's expressions; and the distances and
tolerances the tests measure with.  tests/test_posterior_ref.py proves the
references against 50-digit arithmetic on the CPU.

Notation (marker_ref's): t = sum_k r1_k a_k gam1_k (tabs = sum_k |r1_k a_k
gam1_k|), G = sum_k a_k gam1_k, q_l = 1 / (G sigma_l + 1), s2_l = sigma_l q_l, h =
t^2 / 2; against the spike, slab l has the log-weight

    D_l = log(lam omega_l / (1 - lam)) + h s2_l + log(q_l) / 2,

lodds = log sum_l exp(D_l), pip = sigmoid(lodds), resp_l = exp(D_l) / sum_j exp(D_j),
var = Var(x | r1) over all components, kappa3 = sum_l p_l (dev_l^3 + 3 dev_l s2_l)
the third central moment (d var / d t), dev_l = E(x | l) - E(x).

Distances: the error over the value's size plus the first-order effect of one
relative rounding in t (as marker_ref.dist_xhat).  A = max_l of the sum of the
absolute values of D_l's three terms, S = |lodds| + A + |t| (sum_l resp_l s2_l) tabs:

    lodds   S
    pip     pip (1 + (1 - pip) S)
    var     var + |kappa3| tabs
    resp_l  resp_l (1 + A + |t| |s2_l - sum_j resp_j s2_j| tabs) + 2**-970
    sums    relative;  the count is exact

(2**-970: a responsibility below f64's normal range is not representable).
Tolerance: marker_ref's rule, tol = 8 max(d, 2**-50) with d the f64
restatement's distance on the test's own inputs, capped at CAP = 1e-12.

Exact edges: lam == 0 gives pip = 0, lodds = -inf, var = 0; lam == 1 gives pip =
1, lodds = +inf, var = the slab mixture's variance; resp is the slabs' own
mixture either way (log omega_l in place of the odds' constant, also in A)."""
import numpy as np

from tests import marker_ref as mr

L_ = mr.L_
CAP = 1e-12
RESP_FLOOR = L_(2.0) ** -970
QUANTITIES = ("lodds", "pip", "var", "resp", "sum_pip", "sum_var")


def tolerance(d):
    return mr.tolerance(d, CAP)


def _moments(t, G, sig, logw):
    """Normalised weights p [M][L], mean, variance and third central moment of
    the mixture sum_l w_l N(0, sig_l) seen through t with precision G -- the
    non-negative-term forms of marker_ref.posterior (dev from the pairwise
    differences q_l q_j (sig_l - sig_j), never as a difference of means)."""
    p, q = mr._weights(t, G, sig, logw)
    s2 = sig * q
    dlj = (q[:, None] * q[None, :]) * (sig[:, None] - sig[None, :])
    dev = t[:, None] * (p[:, None, :] * dlj[None, :, :]).sum(axis=-1)
    mean = t * (p * s2).sum(axis=-1)
    var = (p * s2).sum(axis=-1) + (p * dev * dev).sum(axis=-1)
    k3 = (p * (dev ** 3 + 3 * dev * s2)).sum(axis=-1)
    return p, q, mean, var, k3


def reference(r1s, gam1s, a, lam, omegas, sigmas, thr=0.95):
    """Extended-precision reference of every output: dict(lodds, pip, omp (1 -
    pip), var, k3, resp [M][nslab], sum_pip, sum_var, count, and the distances'
    ingredients t, tabs, A [M], ms1 (sum_l resp_l s2_l), s2 [nslab])."""
    hi, lo = mr._ag(a, gam1s)
    G = (hi + lo).sum()
    t, tabs = mr._dot_ag(r1s, a, gam1s)
    om = np.asarray(omegas, dtype=L_)
    sg = np.asarray(sigmas, dtype=L_)
    lamL = L_(lam)
    h = t * t / 2
    # the slabs' own mixture: the responsibilities given inclusion
    resp, qs = mr._weights(t, G, sg, np.log(om))
    s2 = sg * qs
    ms1 = (resp * s2).sum(axis=-1)
    edge = lam == 0.0 or lam == 1.0
    cw = np.log(om) if edge else np.log(lamL * om) - np.log1p(-lamL)
    terms = np.abs(cw)[None, :] + np.abs(h[:, None] * s2[None, :]) + np.abs(np.log(qs) / 2)[None, :]
    A = terms.max(axis=-1)
    if edge:
        one, zero = np.ones_like(t), np.zeros_like(t)
        if lam == 0.0:
            lodds, pip, omp, var, k3 = -np.inf * one, zero, one, zero, zero
        else:
            _, _, _, var, k3 = _moments(t, G, sg, np.log(om))
            lodds, pip, omp = np.inf * one, one, zero
    else:
        D = cw[None, :] + h[:, None] * s2[None, :] + (np.log(qs) / 2)[None, :]
        mx = D.max(axis=-1)
        lodds = mx + np.log(np.exp(D - mx[:, None]).sum(axis=-1))
        sig, logw = mr._mix(lam, omegas, sigmas)
        p, _, _, var, k3 = _moments(t, G, sig, logw)
        pip, omp = p[:, 1:].sum(axis=-1), p[:, 0]
    return dict(lodds=lodds, pip=pip, omp=omp, var=var, k3=k3, resp=resp, sum_pip=pip.sum(),
                sum_var=var.sum(), count=int((pip >= L_(thr)).sum()), t=t, tabs=tabs, A=A,
                ms1=ms1, s2=s2)


def kernel_f64(r1s, gam1s, a, lam, omegas, sigmas, thr=0.95):
    """The kernel's expressions in plain f64 NumPy, operation for operation (the
    host constants of posterior_enqueue, then k_posterior's marker body)."""
    r1s = np.asarray(r1s, dtype=np.float64)
    ag = np.asarray(a, dtype=np.float64) * np.asarray(gam1s, dtype=np.float64)
    om = np.asarray(omegas, dtype=np.float64)
    sg = np.asarray(sigmas, dtype=np.float64)
    G, t = ag[0], r1s[0] * ag[0]
    for k in range(1, len(ag)):
        G = G + ag[k]
        t = t + r1s[k] * ag[k]
    edge = -1 if lam == 0.0 else 1 if lam == 1.0 else 0
    q = 1.0 / (G * sg + 1.0)
    s2 = sg * q
    hq = -np.log1p(G * sg) / 2
    with np.errstate(divide="ignore"):
        cw = np.log(om) if edge else np.log(lam * om) - np.log1p(-lam)
    h = t * t / 2
    D = (cw[None, :] + h[:, None] * s2[None, :]) + hq[None, :]
    mx = D.max(axis=-1)
    E = np.exp(D - mx[:, None])
    se = E[:, 0].copy()
    for l in range(1, len(sg)):
        se = se + E[:, l]
    resp = E / se[:, None]
    m1 = resp[:, 0] * s2[0]
    for l in range(1, len(sg)):
        m1 = m1 + resp[:, l] * s2[l]
    ms = t * m1
    vs = m1.copy()
    for l in range(len(sg)):
        d = t * s2[l] - ms
        vs = vs + resp[:, l] * (d * d)
    lo = mx + np.log(se)
    if edge:
        lo = np.full_like(lo, -np.inf if edge < 0 else np.inf)
    pos = lo >= 0
    with np.errstate(over="ignore"):
        e = np.exp(np.where(pos, -lo, lo))
    pip = np.where(pos, 1 / (1 + e), e / (1 + e))
    qip = np.where(pos, e / (1 + e), 1 / (1 + e))
    var = pip * vs + pip * qip * (ms * ms)
    return dict(lodds=lo, pip=pip, var=var, resp=resp, sum_pip=pip.sum(), sum_var=var.sum(),
                count=int((pip >= thr).sum()))


# ---------------------------------------------------------------------------
# distances
# ---------------------------------------------------------------------------
def _ratio(err, scale):
    """max err / scale; 0 / 0 counts as 0, a nonzero error on a zero scale as inf."""
    out = np.zeros(np.shape(err), dtype=L_)
    nz = scale > 0
    out[nz] = err[nz] / scale[nz]
    out[~nz & (err > 0)] = np.inf
    return float(out.max())


def _abs_err(x, ref):
    """|x - ref| with equal infinities counting as no error."""
    x = np.atleast_1d(np.asarray(x, dtype=L_))
    ref = np.atleast_1d(np.asarray(ref, dtype=L_))
    same = np.isinf(ref) & (x == ref)
    with np.errstate(invalid="ignore"):
        err = np.abs(x - ref)
    err[same] = 0
    err[np.isnan(err)] = np.inf
    return err


def _S(ref):
    fin = np.where(np.isinf(ref["lodds"]), L_(0), np.abs(ref["lodds"]))
    return fin + ref["A"] + np.abs(ref["t"]) * ref["ms1"] * ref["tabs"]


def dist_lodds(x, ref):
    return _ratio(_abs_err(x, ref["lodds"]), _S(ref))


def dist_pip(x, ref):
    return _ratio(_abs_err(x, ref["pip"]), ref["pip"] * (1 + ref["omp"] * _S(ref)))


def dist_var(x, ref):
    return _ratio(_abs_err(x, ref["var"]), ref["var"] + np.abs(ref["k3"]) * ref["tabs"])


def dist_resp(x, ref):
    """x: [M][nslab]."""
    r = ref["resp"]
    cond = np.abs(ref["t"])[:, None] * np.abs(ref["s2"][None, :] - ref["ms1"][:, None]) \
        * ref["tabs"][:, None]
    return _ratio(_abs_err(x, r), r * (1 + ref["A"][:, None] + cond) + RESP_FLOOR)


def dist_sum(x, ref):
    """Relative (sums of one sign); 0 against 0 counts as 0."""
    return _ratio(_abs_err(x, ref), np.atleast_1d(np.abs(np.asarray(ref, dtype=L_))))


def distances(got, ref):
    """Every quantity's distance of `got` (kernel_f64's or the device's dict) from
    the reference, by name (QUANTITIES)."""
    return dict(lodds=dist_lodds(got["lodds"], ref), pip=dist_pip(got["pip"], ref),
                var=dist_var(got["var"], ref), resp=dist_resp(got["resp"], ref),
                sum_pip=dist_sum(got["sum_pip"], ref["sum_pip"]),
                sum_var=dist_sum(got["sum_var"], ref["sum_var"]))


def count_is_decided(ref, thr, tol_pip):
    """No marker's reference pip lies within the pip tolerance of thr: the count is
    then the same for every result inside that tolerance."""
    scale = ref["pip"] * (1 + ref["omp"] * _S(ref))
    return bool((np.abs(ref["pip"] - L_(thr)) > tol_pip * scale).all())


_REFS = {}


def case_reference(cs, M, thr=0.95):
    """(inputs, reference, restatement, its distances) of marker_ref case cs at M
    markers, computed once per process and shared: do not write to them."""
    key = (cs, M, thr)
    if key not in _REFS:
        c = mr.case(cs, M)
        ref = reference(thr=thr, **c)
        f64 = kernel_f64(thr=thr, **c)
        _REFS[key] = (c, ref, f64, distances(f64, ref))
    return _REFS[key]
