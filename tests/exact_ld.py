"""Exact-arithmetic LD data: inputs whose products and partial sums are exactly
representable in f64 in ANY order, so one integer reference pins every form of
the LD pass bit for bit.

R holds dyadic rationals r / 2**bits, the right-hand sides and dot weights are
integers, the coefficients multiples of 1/4.  Every product R_ij v_j is then a
multiple of 2**-bits, every partial sum of them too, and c1 (R v)_i + c2 v_i a
multiple of 2**-(bits + 2).  A sum of multiples of a unit u whose absolute
values add up to less than 2**53 u is exact however it is ordered, grouped or
contracted into FMAs; check_exact asserts that bound (with a bit to spare:
2**52) on the very inputs a test uses, for out, yout and the dots.

Two regimes:
  narrow   R 5 bits, |v| <= 31, w in [-3, 3], c1, c2 in {k/4, |k| <= 8},
           ys1 = 0.75, ys0 = 0.25: out, yout and dots together;
  wide-bit R 17 bits, v 17 bits, c1 in {1, 0.75}, c2 in {0, 0.25}, no dots: out
           only; the row sums need more than 24 significant bits, so a float
           intermediate anywhere breaks equality, while every stored R (<= 18
           significant bits) is exact in f32 storage.
"""
import numpy as np

NARROW = dict(bits=5, vmax=31, wmax=3)
WIDE = dict(bits=17, vmax=(1 << 17) - 1)
YS1, YS0 = 0.75, 0.25
LIMIT = float(2 ** 52)


def _seed(*key):
    return np.random.RandomState([int(k) & 0x7FFFFFFF for k in key])


def exact_block(n, bits, seed, bw=None, symmetric=True):
    """n x n f64 array of entries r / 2**bits, r an integer in [-2**bits,
    2**bits]; exactly symmetric unless symmetric=False; zero where |i - j| > bw
    when bw is given."""
    rs = _seed(seed, n, bits)
    if symmetric:   # X + X^T of half-range integers: symmetric by construction
        h = 1 << (bits - 1)
        A = rs.randint(-h, h + 1, size=(n, n), dtype=np.int32)
        A = A + A.T
    else:
        A = rs.randint(-(1 << bits), (1 << bits) + 1, size=(n, n), dtype=np.int32)
    if bw is not None:
        i = np.arange(n)
        A[np.abs(i[:, None] - i[None, :]) > bw] = 0
    return A.astype(np.float64) / float(1 << bits)


class Band:
    """Exactly symmetric band block kept as its upper diagonals, never densified:
    U[i, d] = R[i, i + d] (0 past the last column), entries r / 2**bits."""

    def __init__(self, n, bits, seed, bw):
        self.n, self.bw, self.bits = int(n), int(min(bw, n - 1)), bits
        self.shape = (self.n, self.n)
        rs = _seed(seed, n, bits, bw)
        U = rs.randint(-(1 << bits), (1 << bits) + 1, size=(self.n, self.bw + 1))
        U = U.astype(np.float64) / float(1 << bits)
        i = np.arange(self.n)[:, None]
        U[i + np.arange(self.bw + 1)[None, :] >= self.n] = 0.0
        self.U = U
        # the CSR arrays of the upper triangle (Engine.set_ld_block_csr)
        lens = np.minimum(self.bw + 1, self.n - np.arange(self.n))
        self.indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        keep = np.arange(self.bw + 1)[None, :] < lens[:, None]
        self.indices = (i + np.arange(self.bw + 1)[None, :])[keep].astype(np.int64)
        self.data = U[keep]

    def matmul(self, V, absolute=False):
        """(R V^T)^T for V [ncol][n] from the upper triangle: U V + U^T V - diag V
        (scipy CSR products; under check_exact's bound any order is exact).
        absolute: |R|."""
        import scipy.sparse

        data = np.abs(self.data) if absolute else self.data
        up = scipy.sparse.csr_matrix((data, self.indices, self.indptr), shape=self.shape)
        diag = np.abs(self.U[:, 0]) if absolute else self.U[:, 0]
        return (up @ V.T + up.T @ V.T).T - diag * V

    def scipy_csr(self):
        """The whole symmetric block as scipy CSR."""
        import scipy.sparse

        up = scipy.sparse.csr_matrix((self.data, self.indices, self.indptr), shape=self.shape)
        return (up + scipy.sparse.triu(up, 1).T).tocsr()


def block_size(B):
    return B.shape[0]


def block_matmul(B, V, absolute=False):
    if isinstance(B, Band):
        return B.matmul(V, absolute)
    return V @ (np.abs(B) if absolute else B).T


def matmul(blocks, V, absolute=False):
    """[ncol][M] block-diagonal product R V (or |R| V) in f64 numpy."""
    out, o = np.empty_like(V), 0
    for B in blocks:
        n = block_size(B)
        out[:, o:o + n] = block_matmul(B, V[:, o:o + n], absolute)
        o += n
    assert o == V.shape[1]
    return out


def exact_rhs(ncol, M, bits, seed):
    """Integer-valued f64 right-hand sides [ncol][M], |v| <= 2**bits - 1."""
    m = (1 << bits) - 1
    return _seed(seed, ncol, M, bits).randint(-m, m + 1, size=(ncol, M)).astype(np.float64)


def exact_weights(ncol, M, wmax, seed):
    """Integer dot weights [ncol][M] in [-wmax, wmax]."""
    return _seed(seed, ncol, M, wmax, 77).randint(-wmax, wmax + 1, size=(ncol, M)).astype(np.float64)


def narrow_coeffs(ncol):
    """Per-column c1, c2 (multiples of 1/4, |k| <= 8), all pairs different, with
    a zero c1, a negative c1, a negative c2 and a c2 = 0 column among the first
    three (so every column count >= 3 holds them)."""
    k1 = np.array([3, -5, 0, 8, 1, -2, 7, 4, -8, 6, 2, -1, 5, -3, -7, -4], dtype=np.float64)
    k2 = np.array([0, 2, -3, 1, -6, 0, 5, -1, 4, 8, -8, 3, -2, 7, 6, -4], dtype=np.float64)
    return k1[:ncol] / 4.0, k2[:ncol] / 4.0


def wide_coeffs(ncol):
    c1 = np.where(np.arange(ncol) % 2 == 0, 1.0, 0.75)
    c2 = np.where(np.arange(ncol) % 3 == 0, 0.0, 0.25)
    return c1, c2


def check_blocks(blocks, bits):
    """Every stored entry is r / 2**bits with an integer |r| <= 2**bits."""
    scale = float(1 << bits)
    for B in blocks:
        a = (B.U if isinstance(B, Band) else B) * scale
        assert np.array_equal(a, np.rint(a)) and np.max(np.abs(a), initial=0.0) <= scale


def abs_bound(blocks, V):
    """[1][M]: sum_j |R_ij| max_c |V_cj|, an upper bound of every column's
    sum_j |R_ij| |V_cj| from one product instead of one per column."""
    return matmul(blocks, np.abs(V).max(axis=0, keepdims=True), absolute=True)


def check_exact(blocks, V, c1, c2, bits, w=None, ys=None, RA=None):
    """Assert the premise on these very inputs: R and the coefficients sit on
    their grids, and in units of 2**-(bits + 2) the absolute values of all terms
    of any out, yout (ys = (ys1, ys0)) or dot (w given; the sum runs over ALL
    markers, as the ordered reduction does) add up to less than 2**52.  RA:
    abs_bound(blocks, V') of right-hand sides V' that hold V's columns, for a
    caller that formed it (and ran check_blocks) once for many calls; blocks
    may then be None."""
    if RA is None:
        check_blocks(blocks, bits)
        RA = abs_bound(blocks, V)
    c1, c2 = np.asarray(c1, dtype=np.float64), np.asarray(c2, dtype=np.float64)
    for v in (V, 4.0 * c1, 4.0 * c2) + (() if w is None else (w,)) + \
            (() if ys is None else (4.0 * np.asarray(ys),)):
        assert np.array_equal(v, np.rint(v))
    unit = 4.0 * float(1 << bits)
    bound = (np.abs(c1)[:, None] * RA + np.abs(c2)[:, None] * np.abs(V)) * unit
    assert bound.max() < LIMIT, bound.max()
    if ys is not None:
        yb = (abs(ys[0]) * RA + abs(ys[1]) * np.abs(V)) * unit
        assert yb.max() < LIMIT, yb.max()
    if w is not None:
        db = (np.abs(w) * bound).sum(axis=1)
        assert db.max() < LIMIT, db.max()
    return RA


def reference(RV, V, c1, c2, w=None, ys=None):
    """(out, yout, dots) from the exact product RV = matmul(blocks, V)."""
    c1, c2 = np.asarray(c1, dtype=np.float64), np.asarray(c2, dtype=np.float64)
    out = c1[:, None] * RV + c2[:, None] * V
    yout = None if ys is None else ys[0] * RV + ys[1] * V
    dots = None if w is None else (w * out).sum(axis=1)
    return out, yout, dots


def significant_bits(x, bits):
    """Bits between the highest and the lowest set bit of x in units of
    2**-(bits + 2) (0 for 0): what an exact representation of x needs."""
    q = np.abs(np.rint(np.asarray(x, dtype=np.float64) * float(1 << (bits + 2)))).astype(np.int64)
    hi = np.frexp(q.astype(np.float64))[1]                 # q < 2**53: exact
    low = np.frexp((q & -q).astype(np.float64))[1] - 1     # the lowest set bit's index
    return np.where(q != 0, hi - low, 0)


# ---- shapes shared by the CPU premise test and the GPU gate -----------------
# triangle / dense / f32 geometry: 4353 = 17 panels + 1 (a second 512-column
# strip per parity), 8449 = 33 panels + 1 (the wide form's 8 + 1 strip split)
TRI_SIZES = [1, 2, 127, 128, 129, 255, 256, 257, 511, 512, 513, 767, 1023, 1024, 1025, 1281,
             2047, 2049, 4097, 4353, 8449]
DENSE_SIZES = TRI_SIZES[:-1]   # the full square of 8449 is left out
WALK_BWS = [200, 300, 600, 1000]   # R = 2, 3, 4, 5 ring slots


def ring_slots(bw):
    return (256 + bw + 255) // 256


def walk_sizes(bw):
    """Band block sizes n = 256 (P - 1) + r for P = R + 1 .. 2 W + 2 panels, r
    cycling through 1, 129, 256 (W = max(4, 2 (R - 1)) panels per walk)."""
    R = ring_slots(bw)
    W = max(4, 2 * (R - 1))
    return [256 * (P - 1) + (1, 129, 256)[i % 3] for i, P in enumerate(range(R + 1, 2 * W + 3))]


# history independence: one partition, held as an f64 triangle, an f64 band
# (block b's bandwidth HIST_BWS[b]: 2-5 ring slots) and an f32 triangle
HIST_SIZES = [1281, 769, 4353, 1025, 2049]
HIST_BWS = [200, 200, 600, 300, 1000]
COUPLED = dict(M=21001, bw=700, piece=5120)
