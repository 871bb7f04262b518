"""The premise of the exact-arithmetic gate (tests/exact_ld.py), proved on the
CPU with no GPU involved: on the gate's own shapes the bound check holds, and
the f64 numpy reference is the exact result -- it does not move under random
permutations of the summation order nor when summed in np.longdouble."""
import numpy as np
import pytest

from tests import exact_ld as xl


def _blocks(kind, regime):
    bits = regime["bits"]
    if kind == "tri":
        return [xl.exact_block(n, bits, 11) for n in xl.TRI_SIZES]
    if kind == "nonsym":
        return [xl.exact_block(n, bits, 12, symmetric=False) for n in xl.DENSE_SIZES]
    if kind == "hist_band":
        return [xl.Band(n, bits, 14, bw) for n, bw in zip(xl.HIST_SIZES, xl.HIST_BWS)]
    if kind == "coupled":
        return [xl.Band(xl.COUPLED["M"], bits, 15, xl.COUPLED["bw"])]
    return [xl.Band(n, bits, 13, kind) for n in xl.walk_sizes(kind)]


KINDS = ["tri", "nonsym", "hist_band", "coupled"] + xl.WALK_BWS


@pytest.mark.parametrize("kind", KINDS)
def test_bound_holds_on_every_shape_list(kind):
    """check_exact passes in both regimes at 16 columns (the widest pass; fewer
    columns are a prefix of the same right-hand sides)."""
    for regime in (xl.NARROW, xl.WIDE):
        blocks = _blocks(kind, regime)
        M = sum(xl.block_size(B) for B in blocks)
        V = xl.exact_rhs(16, M, regime["vmax"].bit_length(), 1)
        if regime is xl.NARROW:
            c1, c2 = xl.narrow_coeffs(16)
            w = xl.exact_weights(16, M, regime["wmax"], 2)
            RA = xl.check_exact(blocks, V, c1, c2, regime["bits"], w=w, ys=(xl.YS1, xl.YS0))
            xl.check_exact(None, V, c1, c2, regime["bits"], w=V, ys=(xl.YS1, xl.YS0), RA=RA)
        else:
            c1, c2 = xl.wide_coeffs(16)
            xl.check_exact(blocks, V, c1, c2, regime["bits"])


def test_walk_sizes_reach_the_partition_edges():
    """Per ring size: blocks of exactly W, W + 1 and 2 W panels, and (where the
    smallest band block, R + 1 panels, allows) of fewer than W."""
    assert [xl.ring_slots(bw) for bw in xl.WALK_BWS] == [2, 3, 4, 5]
    for bw in xl.WALK_BWS:
        R = xl.ring_slots(bw)
        W = max(4, 2 * (R - 1))
        P = [-(-n // 256) for n in xl.walk_sizes(bw)]
        assert P == list(range(R + 1, 2 * W + 3))
        assert {W, W + 1, 2 * W} <= set(P)
        assert min(P) < W or R + 1 == W
        assert all(n > 256 * R for n in xl.walk_sizes(bw))   # stored as a band


def test_wide_bit_rows_need_more_than_f32():
    """Typical wide-bit results need more than 24 significant bits (a float
    intermediate anywhere breaks equality) while every stored R fits f32."""
    bits = xl.WIDE["bits"]
    blocks = [xl.exact_block(n, bits, 11) for n in (129, 513, 1281)]
    M = sum(B.shape[0] for B in blocks)
    V = xl.exact_rhs(8, M, 17, 1)
    c1, c2 = xl.wide_coeffs(8)
    out, _, _ = xl.reference(xl.matmul(blocks, V), V, c1, c2)
    assert np.median(xl.significant_bits(out, bits)) > 24
    for B in blocks:
        np.testing.assert_array_equal(B.astype(np.float32).astype(np.float64), B)


def _small(regime):
    bits = regime["bits"]
    return [xl.exact_block(257, bits, 11), xl.exact_block(130, bits, 12, symmetric=False),
            xl.Band(700, bits, 13, 300), xl.exact_block(1, bits, 11)]


@pytest.mark.parametrize("regime", [xl.NARROW, xl.WIDE], ids=["narrow", "wide"])
def test_reference_is_order_and_precision_invariant(regime):
    """The f64 reference equals, bit for bit, the same sums taken in random
    orders (R's columns and V's rows permuted together, one term at a time
    grouped into random chunks) and in np.longdouble."""
    blocks = _small(regime)
    bits = regime["bits"]
    M = sum(xl.block_size(B) for B in blocks)
    V = xl.exact_rhs(5, M, regime["vmax"].bit_length(), 3)
    if regime is xl.NARROW:
        c1, c2 = xl.narrow_coeffs(5)
        w = xl.exact_weights(5, M, regime["wmax"], 4)
        ys = (xl.YS1, xl.YS0)
    else:
        c1, c2 = xl.wide_coeffs(5)
        w, ys = None, None
    xl.check_exact(blocks, V, c1, c2, bits, w=w, ys=ys)
    RV = xl.matmul(blocks, V)
    out, yout, dots = xl.reference(RV, V, c1, c2, w=w, ys=ys)
    rs = np.random.RandomState(5)
    o = 0
    for B in blocks:
        n = xl.block_size(B)
        D = B.scipy_csr().toarray() if isinstance(B, xl.Band) else B
        Vb = V[:, o:o + n]
        for _ in range(3):
            p = rs.permutation(n)
            # sequential sums over a permuted order, then two-level chunked sums
            seq = np.zeros((V.shape[0], n))
            for j in p:
                seq += Vb[:, j:j + 1] * D[:, j][None, :]
            np.testing.assert_array_equal(seq, RV[:, o:o + n])
            cut = np.sort(rs.choice(np.arange(1, n), size=min(7, n - 1), replace=False)) if n > 1 \
                else np.array([], dtype=int)
            parts = [Vb[:, q] @ D[:, q].T for q in np.split(p, cut)]
            np.testing.assert_array_equal(sum(parts[::-1]), RV[:, o:o + n])
        ld = Vb.astype(np.longdouble) @ D.T.astype(np.longdouble)
        np.testing.assert_array_equal(ld.astype(np.float64), RV[:, o:o + n])
        assert np.array_equal(ld, RV[:, o:o + n].astype(np.longdouble))
        o += n
    L = np.longdouble
    out_l = c1.astype(L)[:, None] * RV.astype(L) + c2.astype(L)[:, None] * V.astype(L)
    assert np.array_equal(out_l, out.astype(L))
    if w is not None:
        p = rs.permutation(M)
        np.testing.assert_array_equal((w[:, p] * out[:, p]).sum(axis=1), dots)
        assert np.array_equal((w.astype(L) * out_l).sum(axis=1), dots.astype(L))
        assert np.array_equal(L(ys[0]) * RV.astype(L) + L(ys[1]) * V.astype(L), yout.astype(L))


def test_band_matches_dense():
    """Band.matmul (from the upper triangle) is the dense product of the same block."""
    B = xl.Band(700, 5, 13, 300)
    V = xl.exact_rhs(3, 700, 5, 9)
    D = B.scipy_csr().toarray()
    np.testing.assert_array_equal(D, D.T)
    np.testing.assert_array_equal(B.matmul(V), V @ D.T)
    np.testing.assert_array_equal(B.matmul(np.abs(V), absolute=True), np.abs(V) @ np.abs(D).T)
