"""CPU premises of the LMMSE gate (tests/lmmse_ref.py): tier 1's data is exact,
the dense reference's residual is below 2**-60 |b|, the f64 oracle alone passes
every bound, and an error of 1e-12 planted in one entry of R or in one scalar
is caught by the rule.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

from tests import lmmse_ref as lr
from tests import marker_ref as mr


@pytest.mark.parametrize("shape", lr.T1_SHAPES)
def test_tier1_data_is_exact(shape):
    """t1_case asserts, on the very data, the grids and the 2**52 bound of every
    pass sum and dot; here also: a clamped and an unclamped Z in every layout
    with more than one cohort, distinct scalars, finite expected outputs that
    the learn / damp switches change only where the step says."""
    for cfg, ld_of in lr.COHORTS.items():
        for s in lr.RIDGES:
            c = lr.t1_case(shape, cfg, s)
            assert c["clamp"] == [len(ld_of) > 1 and k == len(ld_of) - 1 for k in range(len(ld_of))]
            assert len(set(c["N"])) == c["K"]
            for k in range(c["K"]):
                for v in (c["x2"][k], c["s2u"][k], c["r"][k], c["r1"][k], c["xhat1"]):
                    assert np.array_equal(v, np.rint(v)) and np.abs(v).max() <= 31
                assert set(np.unique(c["u"][k])) <= {-1, 1}
            outs = {(d, l): lr.t1_expected(c, d, l) for d in (False, True) for l in (False, True)}
            for (d, l), (o, r1n) in outs.items():
                assert np.isfinite(o).all() and np.isfinite(r1n).all(), (cfg, s, d, l)
                np.testing.assert_array_equal(o[:, lr.O_TRSIGMA2], outs[(False, False)][0][:, lr.O_TRSIGMA2])
                if not l:
                    assert not o[:, [lr.O_Z, lr.O_TRRSIGMA2, lr.O_XRX]].any()
                    np.testing.assert_array_equal(o[:, lr.O_GAMW], c["gamw"])
                else:
                    assert [(z == 0.0) for z in o[:, lr.O_Z]] == c["clamp"]
            # damping moves alpha2 (alpha2_prev is not the undamped value)
            assert (outs[(True, True)][0][:, lr.O_ALPHA2] != outs[(False, True)][0][:, lr.O_ALPHA2]).all()


def test_passes_of_a_zero_iteration_call():
    assert lr.expected_passes([0], True, True, True) == 1
    assert lr.expected_passes([0, 1, 0], True, True, False) == 4
    assert lr.expected_passes([0] * 9, True, False, False) == 2
    assert lr.expected_passes([0] * 9, False, True, False) == 2


@pytest.mark.parametrize("shape", list(lr.T2_SHAPES))
def test_reference_residual_and_oracle_inside_every_bound(shape):
    """On the gate's own systems: the refined solutions' longdouble residual is
    below 2**-60 |b|; every distance of the oracle, in both CG forms and every
    call, is below the cap 2 kappa rtol (so inside marker_ref.tolerance of
    itself); the CG needs iterations and converges."""
    S = lr.system(shape)
    seq = lr.sequence(shape)
    for n, refs in enumerate(seq["ref"]):
        for k, ref in enumerate(refs):
            print("%s call %d cohort %d: residual 2**%.1f  kappa %.2f  cap %.3e" % (
                shape, n, k, np.log2(max(ref["res"], 1e-30)), ref["kappa"], lr.cap(ref)))
            assert ref["res"] < 2.0 ** -60
            assert 1.0 < ref["kappa"] < 100.0
            lo, hi = S.lam_range(lr.T2_LD_OF[k])
            assert 0.05 < lo and hi < 1.95          # Gershgorin, row sums < 0.95
            for m in ("rs", "direct"):
                o, d = seq["ora"][m][n][k], seq["dist"][m][n][k]
                b = lr.bounds_of(d, ref)
                print("   %s cg %s  %s" % (m, o["cg"], "  ".join("%s %.2e" % kv for kv in d.items())))
                assert o["cg"][1] == 0 and o["cg"][3] == 0 and min(o["cg"][0], o["cg"][2]) >= 10
                for q in d:
                    assert d[q] <= b[q] and d[q] <= lr.cap(ref), (shape, n, k, m, q, d[q], b[q])


@pytest.mark.parametrize("name", lr.T3_NAMES)
def test_oracle_inside_every_bound_with_state_set_from_outside(name):
    seq = lr.t3_sequence(name)
    for m in seq["ora"]:
        for n, refs in enumerate(seq["ref"]):
            for k, ref in enumerate(refs):
                if ref is None:
                    o = seq["ora"][m][n][k]
                    assert not o["x2"].any() and o["out"][lr.O_XR] == 0.0
                    assert o["out"][lr.O_Z] == seq["inp"][n][k]["N"]
                    continue
                d = seq["dist"][m][n][k]
                assert ref["res"] < 2.0 ** -60
                for q in d:
                    assert d[q] <= lr.cap(ref), (name, m, n, k, q, d[q])


def test_planted_errors_are_detected():
    """1e-12 in the one entry of the block of 1 of R, and a relative 1e-12 in
    gamw, gam2 or alpha1: at least one quantity leaves its bound, in both CG
    forms; the unperturbed oracle stays inside all of them."""
    shape, k = "edges", 0
    S = lr.system(shape)
    seq = lr.sequence(shape)
    inp, ref, ld = seq["inp"][0][k], seq["ref"][0][k], lr.T2_LD_OF[k]
    b1 = int(np.argmin(S.sizes))
    assert S.sizes[b1] == 1
    mats = [B.copy() for B in S.mats[ld]]
    mats[b1][0, 0] += 1e-12
    plants = {"R entry": dict(mats=mats)}
    for q in ("gamw", "gam2", "alpha1"):
        plants[q] = dict(inp=dict(inp, **{q: inp[q] * (1 + 1e-12)}))
    for m, rs_rec in (("rs", True), ("direct", False)):
        bound = lr.bounds_of(seq["dist"][m][0][k], ref)
        for what, p in plants.items():
            o, _ = lr.oracle_step(S, ld, p.get("inp", inp), lr.new_state(S.M), False, True, lr.T2_RHO,
                                  rs_rec, mats=p.get("mats"))
            d = lr.distances(o, ref)
            out = {q: (d[q], bound[q]) for q in d if d[q] > bound[q]}
            print(m, what, "caught by", {q: "%.2e > %.2e" % v for q, v in out.items()})
            assert out, (m, what, d, bound)


def test_tolerance_rule_is_marker_refs():
    assert lr.bounds_of({"q": 0.0}, dict(kappa=5.0)) == {"q": 8 * 2.0 ** -50}
    assert lr.bounds_of({"q": 1.0}, dict(kappa=5.0)) == {"q": 2 * 5.0 * lr.T2_RTOL}
    assert mr.tolerance(1e-14, 1e-12) == 8e-14
