"""Exact genotype panels for the factor LD form (tests/test_gpu_geno_factor.py,
tests/test_geno_factor_host.py): panels whose G is exactly representable, so
G (G^T p) of integer p has ONE value whatever the order of any sum.

N in {64, 256, 1024} (1 / sqrt(N) dyadic).  Every marker has n_obs in {N, N / 2}
observed samples, the rest carry code 1 (missing), and is one of two kinds:
  kind A  n_obs / 2 at x = 0, n_obs / 2 at x = 2: mean 1, sd 1, sqrt(N) G = +-1;
  kind B  n_obs / 8 at x = 0, n_obs / 8 at x = 2, 3 n_obs / 4 at x = 1: mean 1,
          sd 1/2, sqrt(N) G in {0, +-2}.
The sample positions are permuted per row with a seeded generator.  With
integer right-hand sides |p| <= 1023, N q = (sqrt(N) G)(sqrt(N) G)^T p is an
integer below 2**53 by a wide margin (exact_reference asserts it), so q = N q /
N is exact and so is every partial sum on the way, in any order.
"""
import numpy as np

from tests import bed_ref

EXACT_NS = [64, 256, 1024]
RHS_BITS = 10    # |p| <= 1023 (exact_ld.exact_rhs)


def exact_codes(n, N, seed):
    """(n, N) codes by the rules above; kinds and n_obs cycle over the markers."""
    assert N in EXACT_NS
    rs = np.random.RandomState([int(seed), int(n), int(N)])
    codes = np.ones((n, N), dtype=np.int64)            # missing everywhere
    for i in range(n):
        nobs = N if (i // 2) % 2 == 0 else N // 2
        if i % 2 == 0:      # kind A
            row = [3] * (nobs // 2) + [0] * (nobs // 2)
        else:               # kind B
            row = [3] * (nobs // 8) + [0] * (nobs // 8) + [2] * (3 * nobs // 4)
        pos = rs.permutation(N)[:nobs]
        codes[i, pos] = row
    return codes


def scaled_G(codes):
    """sqrt(N) G as int64, asserted to be exactly {-2, -1, 0, 1, 2} and every
    marker usable."""
    codes = np.asarray(codes)
    N = codes.shape[1]
    assert not bed_ref.unusable(codes).any()
    g = bed_ref.G(codes) * np.sqrt(float(N))
    gi = np.rint(g).astype(np.int64)
    assert np.array_equal(g, gi.astype(np.float64))
    assert set(np.unique(gi).tolist()) <= {-2, -1, 0, 1, 2}
    return gi


def exact_reference(blocks, V):
    """[ncol][M] f64: the block-diagonal product R V = G (G^T V) from int64
    arithmetic, exact (V: integer-valued f64 [ncol][M]), and [ncol][M] the sums of
    the absolute values of all its terms, |G| (|G|^T |V|) (exact_ld.check_exact's
    RA: what bounds every partial sum in any order)."""
    Vi = np.rint(V).astype(np.int64)
    assert np.array_equal(Vi.astype(np.float64), V)
    out, RA, o, big = np.empty_like(V), np.empty_like(V), 0, 0
    for codes in blocks:
        n, N = codes.shape
        gi = scaled_G(codes)
        nq = gi @ (gi.T @ Vi[:, o:o + n].T)             # (n, ncol) int64 = N q
        na = np.abs(gi) @ (np.abs(gi).T @ np.abs(Vi[:, o:o + n]).T)
        big = max(big, int(na.max()))
        out[:, o:o + n] = (nq.astype(np.float64) / float(N)).T
        RA[:, o:o + n] = (na.astype(np.float64) / float(N)).T
        o += n
    assert o == V.shape[1] and big < 2 ** 40      # far from 2**53: int64 and f64 both exact
    return out, RA
