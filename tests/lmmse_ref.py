"""References and cases of the LMMSE gate (tests/test_gpu_lmmse_step.py; the
premises are proved on the CPU by tests/test_lmmse_ref.py).

The step (sgv_lmmse), per cohort k, with R_s = (1 - s) R + s I and A = gamw R_s +
gam2 I:

    r2 = (xhat1 - alpha1 r1) / (1 - alpha1),   b = gamw r + gam2 r2,
    A x = b,   A S = u,   xhat2 = rho x + (1 - rho) xhat2_prev (damping),
    TrSigma2 = u.S,  alpha2 = gam2 TrSigma2 / M [damped: rho . + (1 - rho) alpha2_prev],
    gam1 = gam2 (1 - alpha2) / alpha2,  r1' = (xhat2 - alpha2 r2) / (1 - alpha2),
    XR = xhat2.r,  XRX = xhat2.R_s xhat2,  TrRSigma2 = u.R_s S,
    Z = max(N - 2 XR + XRX, 0),  gamw' = N / (Z + TrRSigma2).

Tier 1 (exact).  With cg_maxit = 0 the CG leaves X where set_vector put it, so
x = XHAT2 and S = SIG2U are inputs.  R holds multiples of 2**-5, s is 0 or 1/4,
every vector holds integers |v| <= 31, alpha1 = 1/2 (r2 = 2 xhat1 - r1 exactly):
R_s v is a multiple of 2**-7 and the four sums are sums of such multiples whose
absolute values stay below 2**52 units (asserted on the very data through
exact_ld.check_exact), so any order, grouping or FMA contraction gives the same
f64.  They are formed here from integers; the host scalars are then the
library's f64 expressions restated in its order (the library is compiled
without contraction), so everything is compared bit for bit.

Tier 2 (converged).  R has a unit diagonal and off-diagonal row sums < 0.95, so
kappa(A) is small and known from eigvalsh of the blocks.  The reference solves
every block in the eigenbasis of R (f64: only a preconditioner) and refines it
with np.longdouble residuals until they stop falling (test_lmmse_ref: below
2**-60 |b|), then forms every output in longdouble.

Distances and caps.  The CG stops at |b - A x| < rtol |b|, so |x - x*| <=
kappa rtol |x*| in the 2-norm; cap = 2 kappa rtol (the recurrence's residual
drifts from the true one: the factor 2).  Vectors: |v - ref|_2 / |ref|_2.  Each
scalar's distance is its error over its first-order sensitivity to a relative
2-norm error of size 1 in the solution vectors, so ONE cap serves all:

    TrSigma2 = u.S                      |d| <= |u| |S| e
    alpha2 = rho gam2 TrSigma2 / M ...  |d| <= rho gam2 |u| |S| e / M      =: da
    gam1 = gam2 (1 - alpha2) / alpha2   |d| <= gam2 da / alpha2**2
    XR = xhat2.r                        |d| <= |xhat2| |r| e
    XRX = xhat2.R_s xhat2               |d| <= 2 lmax(R_s) |xhat2|**2 e   (direct or carried)
    TrRSigma2 = u.R_s S                 |d| <= lmax(R_s) |u| |S| e
    Z = N - 2 XR + XRX                  |d| <= 2 d(XR) + d(XRX)
    gamw' = N / (Z + TrRSigma2)         |d| <= gamw'**2 (d(Z) + d(TrRSigma2)) / N
    r1' = (xhat2 - alpha2 r2)/(1 - alpha2)
                                        |d|_2 <= (|xhat2| e + da |xhat2 - r2| / (1 - alpha2)) / (1 - alpha2)

(rho = 1 where the call does not damp; xhat2_prev's own error is of the same
relative size, a convex combination keeps it).  Under the cap the bound of a
quantity is marker_ref.tolerance(d, cap), d the distance of the f64 oracle
(vamp_oracle.cg_track / cg_scipy with the blocked reducer) on the same inputs.
"""
import numpy as np

from oracle import vamp_oracle as vo
from tests import exact_ld as xl
from tests import marker_ref as mr

L_ = np.longdouble
NOUT = 8
O_TRSIGMA2, O_ALPHA2, O_GAM1, O_Z, O_TRRSIGMA2, O_GAMW, O_XR, O_XRX = range(NOUT)
OUT_NAMES = ["TRSIGMA2", "ALPHA2", "GAM1", "Z", "TRRSIGMA2", "GAMW", "XR", "XRX"]
MAXKG = 8

# cohort layouts: name -> ld_of
COHORTS = {"K1": [0], "K2": [0, 0], "K3": [0, 1, 0], "K9": [0] * 9}


def expected_passes(ld_of, warm_pass, learn, rs_rec):
    """LD passes of a cg_maxit = 0 call: per cohort group and LD matrix in it one
    warm-start pass (where columns were set from outside) and, learning gamw
    without the carried products, one more."""
    n = 0
    for g0 in range(0, len(ld_of), MAXKG):
        n += len(set(ld_of[g0:g0 + MAXKG]))
    return n * (int(bool(warm_pass)) + int(bool(learn and not rs_rec)))


# ---------------------------------------------------------------------------
# tier 1: exact arithmetic
# ---------------------------------------------------------------------------
BITS = 5
VMAX_BITS = 5              # |v| <= 31
RIDGES = (0.0, 0.25)
RHO1, ALPHA1 = 0.5, 0.5
T1_SHAPES = ["edges", "mixed9", "one", "c65"]
T1_BAND_BW = 6
_GW = [0.5, 1.0, 2.0]
_T1 = {}


def t1_blocks(shape, ld):
    """LD matrix ld of a tier 1 shape: c65 from band blocks only, the rest dense."""
    key = ("blocks", shape, ld)
    if key not in _T1:
        sizes = mr.PARTS[shape]
        if shape == "c65":
            _T1[key] = [xl.Band(n, BITS, 40 + ld, T1_BAND_BW) for n in sizes]
        else:
            _T1[key] = [xl.exact_block(n, BITS, 30 + 5 * ld + b) for b, n in enumerate(sizes)]
    return _T1[key]


def _ints(seed, M):
    return xl.exact_rhs(1, M, VMAX_BITS, seed)[0]


def _exact_sum(a, b, unit):
    """sum a_i b_i as a Python integer count of `unit`s (a, b multiples of
    units whose product is `unit`), returned as the exact f64."""
    t = a * b / unit
    assert np.array_equal(t, np.rint(t)) and np.abs(t).sum() < xl.LIMIT
    return float(int(t.astype(np.int64).sum())) * unit   # integer sum, < 2**52 units: exact


def t1_case(shape, cfg, s):
    """Inputs and exact sums of one tier 1 case (built once, read-only).  The
    last cohort of a layout with more than one has r aligned with XHAT2 and a
    small N, so its Z is clamped; the others' Z is positive."""
    key = (shape, cfg, s)
    if key in _T1:
        return _T1[key]
    ld_of = COHORTS[cfg]
    K, sizes = len(ld_of), mr.PARTS[shape]
    M = sum(sizes)
    c = dict(shape=shape, cfg=cfg, s=s, ld_of=ld_of, K=K, M=M, sizes=sizes,
             xhat1=_ints(900, M), r=[], r1=[], x2=[], s2u=[], u=[], gamw=[], gam2=[],
             a2prev=[], N=[], clamp=[], sums=[], r2=[])
    for k in range(K):
        x2, r, r1 = _ints(100 + k, M), _ints(300 + k, M), _ints(400 + k, M)
        gw, g2, a2p = _GW[k % 3], _GW[(k // 3 + k) % 3], (1 + k) / 16.0
        for draw in range(16):   # a single marker can give alpha2 = 0 or 1: draw again
            s2u = _ints(200 + k + 1000 * draw, M)
            a2 = g2 * float(np.dot(s2u, np.random.RandomState(500 + k).randint(0, 2, M) * 2.0 - 1)) / M
            if all(a not in (0.0, 1.0) for a in (a2, RHO1 * a2 + (1 - RHO1) * a2p)):
                break
        clamp = K > 1 and k == K - 1
        if clamp:
            r = 31.0 * np.where(x2 < 0, -1.0, 1.0)
        u = np.random.RandomState(500 + k).randint(0, 2, M).astype(np.int8) * 2 - 1
        uf = u.astype(np.float64)
        blocks = t1_blocks(shape, ld_of[k])
        V, W = np.stack([x2, s2u]), np.stack([x2, uf])
        # the pass's own sums and the two dots over it: exact in any order
        xl.check_exact(blocks, V, [1.0 - s] * 2, [s] * 2, BITS, w=W)
        RV = xl.matmul(blocks, V)
        rs = (1.0 - s) * RV + s * V                       # multiples of 2**-7, exact
        unit = 2.0 ** -(BITS + 2)
        sums = dict(TrS=_exact_sum(uf, s2u, 1.0), XR=_exact_sum(x2, r, 1.0),
                    XRX=_exact_sum(x2, rs[0], unit), TrRS=_exact_sum(uf, rs[1], unit))
        t = 2.0 * sums["XR"] - sums["XRX"]
        N = float(1 + k) if clamp else float(int(np.ceil(abs(t))) + 100 + 7 * k)
        z = N - 2.0 * sums["XR"] + sums["XRX"]
        assert (z < 0) == clamp and z != 0.0, (shape, cfg, s, k, z)
        r2 = (c["xhat1"] - ALPHA1 * r1) / (1 - ALPHA1)
        assert np.array_equal(r2, 2.0 * c["xhat1"] - r1)
        assert np.any(gw * r + g2 * r2 != 0.0)
        for name, v in (("r", r), ("r1", r1), ("x2", x2), ("s2u", s2u), ("u", u), ("gamw", gw),
                        ("gam2", g2), ("a2prev", a2p), ("N", N), ("clamp", clamp),
                        ("sums", sums), ("r2", r2)):
            c[name].append(v)
    assert len({(a, b) for a, b in zip(c["gamw"], c["gam2"])}) == K
    _T1[key] = c
    return c


def host_scalars(sums, gamw, gam2, a2prev, N, Mtot, damp, learn, rho=RHO1):
    """The output row of one cohort from its four sums: the library's f64
    expressions in its order (solver.hip: lmmse_group, gamw_outputs)."""
    TrS = np.float64(sums["TrS"])
    with np.errstate(divide="ignore", invalid="ignore"):
        a2 = gam2 * TrS / float(Mtot)
        if damp:
            a2 = rho * a2 + (1 - rho) * a2prev
        g1 = gam2 * (1 - a2) / a2
        out = np.zeros(NOUT)
        out[[O_TRSIGMA2, O_ALPHA2, O_GAM1, O_XR, O_GAMW]] = TrS, a2, g1, sums["XR"], gamw
        if learn:
            z = N - 2 * np.float64(sums["XR"]) + np.float64(sums["XRX"])
            if z < 0:
                z = 0.0
            out[[O_Z, O_XRX, O_TRRSIGMA2]] = z, sums["XRX"], sums["TrRS"]
            out[O_GAMW] = 1 / (z / N + np.float64(sums["TrRS"]) / N)
    return out


def t1_expected(c, damp, learn, sums=None, x2=None):
    """(out [K][8], r1' [K][M]) of a tier 1 case; sums / x2: per-cohort overrides
    (the state-from-outside variants)."""
    out, r1n = [], []
    for k in range(c["K"]):
        sm = c["sums"][k] if sums is None else sums[k]
        xk = c["x2"][k] if x2 is None else x2[k]
        o = host_scalars(sm, c["gamw"][k], c["gam2"][k], c["a2prev"][k], c["N"][k], c["M"], damp,
                         learn)
        a2 = o[O_ALPHA2]
        with np.errstate(divide="ignore", invalid="ignore"):
            r1n.append((xk - a2 * c["r2"][k]) / (1 - a2))
        out.append(o)
    return np.stack(out), np.stack(r1n)


# ---------------------------------------------------------------------------
# tier 2: the systems
# ---------------------------------------------------------------------------
T2_SHAPES = {"edges": (mr.PARTS["edges"], ()), "mixed9": (mr.PARTS["mixed9"], ()),
             "band": ([700, 1300], (1,))}      # (sizes, the blocks stored from CSR as bands)
T2_S = 0.1
T2_RTOL = 1e-13
T2_MAXIT = 500
T2_RHO = 0.3               # not 1/2: rho and 1 - rho are told apart
T2_LD_OF = [0, 1, 0]
_SYS = {}


def _offdiag(ld, b, n):
    return 0.2 + 0.25 * (((b + 3 * ld) * 7) % 17) / 17.0 + 0.01 * np.cos(np.arange(max(n - 1, 0)) + ld)


class System:
    """Two LD matrices over one partition: blocks as _cg_system's (unit diagonal,
    off-diagonal row sums < 0.95), their eigen-decompositions, and R_s products
    in f64 (the oracle's operator) and longdouble (the reference's)."""

    def __init__(self, shape):
        import scipy.sparse

        self.shape = shape
        self.sizes, band = T2_SHAPES[shape]
        self.M = sum(self.sizes)
        self.bounds = np.cumsum([0] + list(self.sizes))
        self.s = T2_S
        self.mats, self.upper, self.eig, self._ld = [], [], [], {}
        for ld in range(2):
            rs = np.random.RandomState([len(self.sizes), ld])
            mats, ups, eigs = [], [], []
            for b, n in enumerate(self.sizes):
                if b in band:     # a narrow band, stored from its upper triangle
                    d1 = 0.35 + 0.01 * np.cos(np.arange(n - 1) + ld)
                    U = scipy.sparse.diags([np.ones(n), d1, np.full(n - 2, -0.1 + 0.02 * ld)],
                                           [0, 1, 2], format="csr")
                    R = (U + scipy.sparse.triu(U, 1).T).toarray()
                    ups.append(U)
                else:             # the same band under a small dense symmetric part
                    Nn = rs.uniform(-1, 1, (n, n)) * (0.02 / n)
                    R = (Nn + Nn.T) / 2
                    i = np.arange(n)
                    R[i, i] = 1.0
                    R[i[:-1], i[1:]] += _offdiag(ld, b, n)
                    R[i[1:], i[:-1]] += _offdiag(ld, b, n)
                    ups.append(None)
                assert (np.abs(R).sum(axis=1) - 1.0).max() < 0.95
                assert np.array_equal(R, R.T)
                mats.append(R)
                eigs.append(np.linalg.eigh(R))
            self.mats.append(mats)
            self.upper.append(ups)
            self.eig.append(eigs)

    def upload(self, eng, lds=(0, 1)):
        for ld in lds:
            for b, R in enumerate(self.mats[ld]):
                if self.upper[ld][b] is not None:
                    eng.set_ld_block_csr(ld, b, self.upper[ld][b])
                else:
                    eng.set_ld_block(ld, b, R)

    def lam_range(self, ld):
        """(min, max) eigenvalue of R_s."""
        lo = min(w[0] for w, _ in self.eig[ld])
        hi = max(w[-1] for w, _ in self.eig[ld])
        return (1 - self.s) * lo + self.s, (1 - self.s) * hi + self.s

    def kappa(self, ld, gw, g2):
        lo, hi = self.lam_range(ld)
        return (gw * hi + g2) / (gw * lo + g2)

    def mv(self, ld, v, mats=None):
        """R_s v in f64, as vamp_oracle.BlockLD.matvec_Rs forms it."""
        out = np.empty_like(v)
        for (s0, s1), B in zip(zip(self.bounds[:-1], self.bounds[1:]), mats or self.mats[ld]):
            out[s0:s1] = B @ v[s0:s1]
        return out if self.s == 0.0 else (1 - self.s) * out + self.s * v

    def mv_ld(self, ld, v, mats=None):
        """R_s v in longdouble, rows summed pairwise (np.sum along the row)."""
        v = np.asarray(v, dtype=L_)
        out = np.empty(self.M, dtype=L_)
        for b, ((s0, s1), B) in enumerate(zip(zip(self.bounds[:-1], self.bounds[1:]),
                                              mats or self.mats[ld])):
            key = (ld, b) if mats is None else None
            BL = self._ld.get(key)
            if BL is None:
                BL = B.astype(L_)
                if key is not None:
                    self._ld[key] = BL
            vb = v[s0:s1]
            for i0 in range(0, s1 - s0, 256):
                i1 = min(i0 + 256, s1 - s0)
                out[s0 + i0:s0 + i1] = (BL[i0:i1] * vb[None, :]).sum(axis=1)
        s = L_(self.s)
        return (1 - s) * out + s * v

    def solve(self, ld, gw, g2, b, mats=None):
        """x with (gw R_s + g2 I) x = b: the eigenbasis solve (f64) refined with
        longdouble residuals until they stop falling.  Returns (x, |b - A x| /
        |b|), longdouble.  mats: a perturbed copy of the blocks (the planted
        errors); the preconditioner stays the unperturbed one."""
        b = np.asarray(b, dtype=L_)
        gwL, g2L = L_(gw), L_(g2)

        def pre(res):
            out = np.empty(self.M)
            r64 = res.astype(np.float64)
            for (s0, s1), (w, V) in zip(zip(self.bounds[:-1], self.bounds[1:]), self.eig[ld]):
                out[s0:s1] = V @ ((V.T @ r64[s0:s1]) / (gw * ((1 - self.s) * w + self.s) + g2))
            return out.astype(L_)

        bn = np.sqrt((b * b).sum())
        if bn == 0:
            return np.zeros(self.M, dtype=L_), L_(0)
        x = pre(b)
        best, best_x = None, None
        for _ in range(12):
            res = b - (gwL * self.mv_ld(ld, x, mats) + g2L * x)
            rn = np.sqrt((res * res).sum()) / bn
            if best is not None and rn >= best:
                break
            best, best_x = rn, x
            x = x + pre(res)
        return best_x, best


def system(shape):
    if shape not in _SYS:
        _SYS[shape] = System(shape)
    return _SYS[shape]


# ---------------------------------------------------------------------------
# tier 2: inputs, the longdouble reference step and the f64 oracle step
# ---------------------------------------------------------------------------
def t2_inputs(shape, ncall=3):
    """Everything a sequence of calls is given, for the three cohorts of
    T2_LD_OF (a layout with fewer takes the first ones): r, xhat1, N and per call
    r1, alpha1, probes.  The marker of the smallest block carries a large r."""
    S = system(shape)
    M, K = S.M, len(T2_LD_OF)
    rs = np.random.RandomState([M, 77])
    r = rs.normal(size=(K, M))
    r[:, S.bounds[int(np.argmin(S.sizes))]] *= 40.0
    d = dict(r=r, xhat1=rs.normal(size=M), N=[4.0 * M * (1 + k / 4.0) for k in range(K)],
             gamw=[1.0, 2.0, 0.7], gam2=[0.8, 0.5, 1.5], a2prev=[0.25, 0.4, 0.1],
             r1=[rs.normal(size=(K, M)) for _ in range(ncall)],
             alpha1=[rs.uniform(0.3, 0.6, K) for _ in range(ncall)],
             u=[(rs.randint(0, 2, (K, M)) * 2 - 1).astype(np.int8) for _ in range(ncall)])
    return d


def new_state(M):
    """A cohort's carried state: xhat2, Sigma2_u and their R_s products."""
    z = np.zeros(M)
    return dict(x2=z, s2u=z.copy(), rx2=z.copy(), rs2=z.copy())


def ref_step(S, ld, inp, st, damp, learn, rho, mats=None):
    """One cohort's step in longdouble.  inp: r, xhat1, r1, u, alpha1, gamw, gam2,
    a2prev, N.  st: dict(x2) -- only xhat2_prev enters a converged step.  Returns
    dict(out [8], x2, s2u, r1, scale [8], r1_scale, res) and the new state."""
    A = lambda v: np.asarray(v, dtype=L_)
    r, xh, r1, u = A(inp["r"]), A(inp["xhat1"]), A(inp["r1"]), A(inp["u"])
    al, gw, g2, N = L_(inp["alpha1"]), L_(inp["gamw"]), L_(inp["gam2"]), L_(inp["N"])
    rhoL = L_(rho)
    r2 = (xh - al * r1) / (1 - al)
    x, res1 = S.solve(ld, inp["gamw"], inp["gam2"], gw * r + g2 * r2, mats)
    s2u, res2 = S.solve(ld, inp["gamw"], inp["gam2"], u, mats)
    x2 = rhoL * x + (1 - rhoL) * A(st["x2"]) if damp else x
    TrS = (u * s2u).sum()
    a2 = g2 * TrS / L_(S.M)
    if damp:
        a2 = rhoL * a2 + (1 - rhoL) * L_(inp["a2prev"])
    g1 = g2 * (1 - a2) / a2
    r1n = (x2 - a2 * r2) / (1 - a2)
    XR = (x2 * r).sum()
    out = np.zeros(NOUT, dtype=L_)
    out[[O_TRSIGMA2, O_ALPHA2, O_GAM1, O_XR, O_GAMW]] = TrS, a2, g1, XR, gw
    nrm = lambda v: float(np.sqrt((v * v).sum()))
    nu, ns, nx, nr = nrm(u), nrm(s2u), nrm(x2), nrm(r)
    lmax = S.lam_range(ld)[1]
    rh = rho if damp else 1.0
    da = rh * float(g2) * nu * ns / S.M
    scale = np.zeros(NOUT)
    scale[O_TRSIGMA2], scale[O_ALPHA2] = nu * ns, da
    scale[O_GAM1] = float(g2) * da / float(a2) ** 2
    scale[O_XR] = nx * nr
    if learn:
        XRX = (x2 * S.mv_ld(ld, x2, mats)).sum()
        TrRS = (u * S.mv_ld(ld, s2u, mats)).sum()
        z = N - 2 * XR + XRX
        assert z > 0
        out[[O_Z, O_XRX, O_TRRSIGMA2]] = z, XRX, TrRS
        out[O_GAMW] = 1 / (z / N + TrRS / N)
        scale[O_XRX], scale[O_TRRSIGMA2] = 2 * lmax * nx * nx, lmax * nu * ns
        scale[O_Z] = 2 * scale[O_XR] + scale[O_XRX]
        scale[O_GAMW] = float(out[O_GAMW]) ** 2 * (scale[O_Z] + scale[O_TRRSIGMA2]) / float(N)
    r1_scale = (nx + da * nrm(x2 - r2) / float(1 - a2)) / float(1 - a2)
    return dict(out=out, x2=x2, s2u=s2u, r1=r1n, scale=scale, r1_scale=r1_scale,
                res=max(float(res1), float(res2)), kappa=S.kappa(ld, inp["gamw"], inp["gam2"])), \
        dict(x2=x2.astype(np.float64))


def oracle_step(S, ld, inp, st, damp, learn, rho, rs_rec, maxit=T2_MAXIT, rtol=T2_RTOL, mats=None):
    """One cohort's step in f64 with vamp_oracle's CG (cg_track carrying R_s x, or
    cg_scipy with direct products) and the blocked reducer, as vamp_oracle.infer
    strings them together.  Returns (dict(out, x2, s2u, r1, cg), new state)."""
    red = vo.Reducer("blocked", S.bounds)
    mv = lambda p: S.mv(ld, p, mats)
    r, xh, r1 = inp["r"], inp["xhat1"], inp["r1"]
    al, gw, g2, N = inp["alpha1"], inp["gamw"], inp["gam2"], inp["N"]
    uf = inp["u"].astype(np.float64)
    r2 = (xh - al * r1) / (1 - al)
    mu2 = gw * r + g2 * r2
    Aop = lambda p: gw * mv(p) + g2 * p
    if rs_rec:
        x2, rx2, i1, n1, _ = vo.cg_track(mv, gw, g2, mu2, st["x2"], st["rx2"], maxit, red, rtol)
        s2u, rs2, i2, n2, _ = vo.cg_track(mv, gw, g2, uf, st["s2u"], st["rs2"], maxit, red, rtol)
        if damp:
            rx2 = rho * rx2 + (1 - rho) * st["rx2"]
    else:
        x2, i1, n1, _ = vo.cg_scipy(Aop, mu2, st["x2"], maxit, red, rtol)
        s2u, i2, n2, _ = vo.cg_scipy(Aop, uf, st["s2u"], maxit, red, rtol)
    if damp:
        x2 = rho * x2 + (1 - rho) * st["x2"]
    if not rs_rec:
        rx2, rs2 = mv(x2), mv(s2u)
    TrS = red.dot(uf, s2u)
    a2 = g2 * TrS / S.M
    if damp:
        a2 = rho * a2 + (1 - rho) * inp["a2prev"]
    out = np.zeros(NOUT)
    out[[O_TRSIGMA2, O_ALPHA2, O_GAM1, O_XR, O_GAMW]] = TrS, a2, g2 * (1 - a2) / a2, red.dot(x2, r), gw
    if learn:
        xRx, TrRS = red.dot(x2, rx2), red.dot(uf, rs2)
        z = max(N - 2 * out[O_XR] + xRx, 0.0)
        out[[O_Z, O_XRX, O_TRRSIGMA2, O_GAMW]] = z, xRx, TrRS, 1 / (z / N + TrRS / N)
    return dict(out=out, x2=x2, s2u=s2u, r1=(x2 - a2 * r2) / (1 - a2), cg=[n1, i1, n2, i2]), \
        dict(x2=x2, s2u=s2u, rx2=rx2, rs2=rs2)


def distances(got, ref):
    """{quantity: distance} of a step result (dict(out, x2, s2u, r1)) from the
    reference's (module docstring); a quantity whose scale is 0 is left out."""
    nrm = lambda v: np.sqrt((v * v).sum())
    d = {}
    for name, key in (("xhat2", "x2"), ("sig2u", "s2u")):
        n = nrm(ref[key])
        e = nrm(np.asarray(got[key], dtype=L_) - ref[key])
        d[name] = float(e / n) if n > 0 else (0.0 if e == 0 else np.inf)
    d["r1"] = float(nrm(np.asarray(got["r1"], dtype=L_) - ref["r1"]) / ref["r1_scale"])
    for i, name in enumerate(OUT_NAMES):
        if ref["scale"][i] > 0:
            d[name] = float(abs(L_(got["out"][i]) - ref["out"][i]) / ref["scale"][i])
    return d


def cap(ref, rtol=T2_RTOL):
    return 2.0 * ref["kappa"] * rtol


def bounds_of(d_oracle, ref):
    """{quantity: bound}: marker_ref.tolerance of the oracle's distance under the cap."""
    c = cap(ref)
    return {q: mr.tolerance(d, c) for q, d in d_oracle.items()}


def check(got, ref, d_oracle, what, log=None):
    """Print (and record) every figure, then assert each distance under its bound."""
    d, b = distances(got, ref), bounds_of(d_oracle, ref)
    bad = []
    for q in d:
        line = "%s %s: device %.3e  oracle %.3e  bound %.3e  (cap %.3e, kappa %.2f)" % (
            what, q, d[q], d_oracle[q], b[q], cap(ref), ref["kappa"])
        print(line)
        if log is not None:
            log.append(line)
        if not d[q] <= b[q]:
            bad.append(q)
    assert not bad, (what, {q: (d[q], b[q]) for q in bad})


# ---------------------------------------------------------------------------
# sequences of calls: inputs -> per call, per cohort reference and oracle
# ---------------------------------------------------------------------------
SEQ_DAMP = [False, True, True]
_SEQ = {}


def _f64(v):
    return float(np.float64(v))


def sequence(shape, events=None, name="main", ncall=3, rs_modes=None, zero_cohort=None):
    """The reference and the oracle over `ncall` consecutive calls of the three
    cohorts (learn_gamw on; call 0 cold and undamped, the later ones damped).

    Inputs of call n > 0: alpha2_prev is the reference's alpha2 of call n - 1;
    in the last call gamw and gam2 are the reference's new gamw and gam1 of the
    call before (clipped to [0.5, 4] and [0.3, 5]), all rounded to f64 -- so the
    device, the oracle and the reference get the same numbers.
    events: {n: [(what, k, v)]} applied before call n: what "XHAT2" / "SIG2U"
    replaces that part of cohort k's state by the vector v.
    rs_modes: per call, the carried-product setting of the oracle run "toggle";
    zero_cohort: (n, k): in call n cohort k has r = 0 and r1 = 0 and xhat1 = 0 for all.
    Returns dict(inp[n][k], ref[n][k], ora[mode][n][k], dist[mode][n][k]) with
    mode in ("rs", "direct", and "toggle" if rs_modes)."""
    key = (shape, name)
    if key in _SEQ:
        return _SEQ[key]
    S = system(shape)
    D = t2_inputs(shape, ncall)
    K = len(T2_LD_OF)
    events = events or {}
    modes = {"rs": [True] * ncall, "direct": [False] * ncall}
    if rs_modes:
        modes["toggle"] = list(rs_modes)
    rst = [dict(x2=np.zeros(S.M)) for _ in range(K)]
    ost = {m: [new_state(S.M) for _ in range(K)] for m in modes}
    out = dict(inp=[], ref=[], ora={m: [] for m in modes}, dist={m: [] for m in modes},
               damp=SEQ_DAMP[:ncall], shape=shape)
    gamw, gam2, a2prev = list(D["gamw"]), list(D["gam2"]), list(D["a2prev"])
    for n in range(ncall):
        for what, k, v in events.get(n, []):
            v = np.array(v, dtype=np.float64)
            if what == "XHAT2":
                rst[k] = dict(x2=v)
            for m in modes:
                st = dict(ost[m][k])
                if what == "XHAT2":   # R_s v is re-derived
                    st["x2"], st["rx2"] = v, S.mv(T2_LD_OF[k], v)
                else:
                    st["s2u"], st["rs2"] = v, S.mv(T2_LD_OF[k], v)
                ost[m][k] = st
        inps, refs = [], []
        zc = zero_cohort is not None and zero_cohort[0] == n
        for k in range(K):
            z = zc and zero_cohort[1] == k
            inp = dict(r=np.zeros(S.M) if z else D["r"][k],
                       xhat1=np.zeros(S.M) if zc else D["xhat1"],
                       r1=np.zeros(S.M) if z else D["r1"][n][k], u=D["u"][n][k],
                       alpha1=_f64(D["alpha1"][n][k]), gamw=gamw[k], gam2=gam2[k],
                       a2prev=a2prev[k], N=D["N"][k])
            inps.append(inp)
            if z:      # cold and undamped: xhat2 = 0 exactly, nothing else to refer to
                assert n == 0
                ref, rst[k] = None, dict(x2=np.zeros(S.M))
            else:
                ref, rst[k] = ref_step(S, T2_LD_OF[k], inp, rst[k], SEQ_DAMP[n], True, T2_RHO)
            refs.append(ref)
        out["inp"].append(inps)
        out["ref"].append(refs)
        for m, rsm in modes.items():
            os_, ds = [], []
            for k in range(K):
                o, ost[m][k] = oracle_step(S, T2_LD_OF[k], inps[k], ost[m][k], SEQ_DAMP[n], True,
                                           T2_RHO, rsm[n])
                os_.append(o)
                ds.append(None if refs[k] is None else distances(o, refs[k]))
            out["ora"][m].append(os_)
            out["dist"][m].append(ds)
        for k in range(K):
            if refs[k] is None:
                continue
            a2prev[k] = _f64(refs[k]["out"][O_ALPHA2])
            if n == ncall - 2:
                gamw[k] = _f64(min(max(refs[k]["out"][O_GAMW], 0.5), 4.0))
                gam2[k] = _f64(min(max(refs[k]["out"][O_GAM1], 0.3), 5.0))
    _SEQ[key] = out
    return out


# ---------------------------------------------------------------------------
# tier 3: state set from outside, on the tier 2 system
# ---------------------------------------------------------------------------
T3_SHAPE = "edges"
T3_NAMES = ["x2zero", "s2uzero", "x2set", "toggle", "zero_rhs"]


def t3_vector(shape):
    """The non-zero vector XHAT2 is set to in "x2set"."""
    M = system(shape).M
    return 0.3 * np.random.RandomState([M, 78]).normal(size=M)


def t3_sequence(name, shape=T3_SHAPE):
    """The named sequences: before the third call cohort 0's XHAT2 (SIG2U) is set
    to zeros, or XHAT2 to t3_vector; the carried products toggled on, off, on;
    a zero right-hand side for cohort 0 in a first call, then an ordinary one."""
    M = system(shape).M
    if name == "x2zero":
        return sequence(shape, {2: [("XHAT2", 0, np.zeros(M))]}, name)
    if name == "s2uzero":
        return sequence(shape, {2: [("SIG2U", 0, np.zeros(M))]}, name)
    if name == "x2set":
        return sequence(shape, {2: [("XHAT2", 0, t3_vector(shape))]}, name)
    if name == "toggle":
        return sequence(shape, None, name, rs_modes=[True, False, True])
    if name == "zero_rhs":
        return sequence(shape, None, name, ncall=2, zero_cohort=(0, 0))
    raise KeyError(name)
