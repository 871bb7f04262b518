"""NumPy restatement of the genotype LD definition (include/sgvamp_hip.h,
"genotype LD source"), for the tests: decode, exact integer counts, mean, sd, G,
R = G G^T, r = G y, g = X_std^T beta.  Independent of ldio.BedLD.block (sample
by sample indexing here, a bit-field reshape there) and of the device code.

Also the tests' panels: draw_codes() draws A1 counts at allele frequencies in
[0.05, 0.5] with a missing rate, until every marker has LD.
"""
import numpy as np

A1 = {0: 2.0, 2: 1.0, 3: 0.0}   # code -> A1 count (code 1: missing)


def decode(rows, N):
    """(n, N) codes of packed rows: sample s is bits 2 (s % 4) of byte s // 4."""
    rows = np.asarray(rows, dtype=np.uint8)
    out = np.empty((rows.shape[0], N), dtype=np.int64)
    for s in range(N):
        out[:, s] = (rows[:, s // 4].astype(np.int64) >> (2 * (s % 4))) & 3
    return out


def pack(codes, row_bytes=None, pad_bits=0):
    """Packed rows of (n, N) codes; row_bytes >= ceil(N / 4) (default: that);
    pad_bits: the 2-bit code written into every position past sample N."""
    codes = np.asarray(codes, dtype=np.int64)
    n, N = codes.shape
    nb = (N + 3) // 4 if row_bytes is None else int(row_bytes)
    full = np.full((n, nb * 4), pad_bits, dtype=np.int64)
    full[:, :N] = codes
    rows = np.zeros((n, nb), dtype=np.int64)
    for q in range(4):
        rows |= full[:, q::4] << (2 * q)
    return rows.astype(np.uint8)


def counts(codes):
    """(n, 4) int64: samples per code."""
    codes = np.asarray(codes)
    return np.stack([(codes == k).sum(axis=1) for k in range(4)], axis=1).astype(np.int64)


def moments(codes):
    """Exact integers n_obs, S1, S2 per marker."""
    c = counts(codes)
    nobs = c[:, 0] + c[:, 2] + c[:, 3]
    return nobs, 2 * c[:, 0] + c[:, 2], 4 * c[:, 0] + c[:, 2]


def unusable(codes):
    nobs, s1, s2 = moments(codes)
    return (nobs == 0) | (nobs * s2 - s1 * s1 == 0)


def mean_sd(codes):
    nobs, s1, s2 = moments(codes)
    mean = s1.astype(np.float64) / nobs.astype(np.float64)
    sd = np.sqrt((nobs * s2 - s1 * s1).astype(np.float64)
                 / (nobs.astype(np.float64) * nobs.astype(np.float64)))
    return mean, sd


def X_std(codes):
    """(n, N): (x - mean) / sd, 0 where missing."""
    codes = np.asarray(codes)
    mean, sd = mean_sd(codes)
    x = np.zeros(codes.shape)
    for k, v in A1.items():
        x[codes == k] = v
    X = (x - mean[:, None]) / sd[:, None]
    X[codes == 1] = 0.0
    return X


def G(codes):
    codes = np.asarray(codes)
    return X_std(codes) / np.sqrt(float(codes.shape[1]))


def R(codes):
    g = G(codes)
    return g @ g.T


def r(codes, y):
    return G(codes) @ np.asarray(y, dtype=np.float64)


def g(codes, beta):
    return X_std(codes).T @ np.asarray(beta, dtype=np.float64)


def _draw(rs, n, N, miss):
    p = rs.uniform(0.05, 0.5, size=n)
    x = rs.binomial(2, p[:, None], size=(n, N))
    codes = np.array([3, 2, 0])[x]           # A1 count 0, 1, 2 -> code 3, 2, 0
    if miss > 0:
        codes = np.where(rs.uniform(size=(n, N)) < miss, 1, codes)
    return codes.astype(np.int64)


def draw_codes(n, N, miss=0.0, seed=0, tries=8):
    """(n, N) codes in which every marker has LD: redrawn from RandomState(seed),
    whole, up to `tries` times; where that cannot succeed (N = 5 leaves about one
    marker in six monomorphic) the usable markers of an oversampled draw, in
    their order."""
    rs = np.random.RandomState(seed)
    for _ in range(tries):
        codes = _draw(rs, n, N, miss)
        if not unusable(codes).any():
            return codes
    keep = np.zeros((0, N), dtype=np.int64)
    while keep.shape[0] < n:
        codes = _draw(rs, 2 * n, N, miss)
        keep = np.concatenate([keep, codes[~unusable(codes)]])
    return keep[:n]


def bim_fam(M, N, prefix="rs"):
    bim = [("1", "%s%d" % (prefix, i), "0", str(i + 1), "A", "G") for i in range(M)]
    fam = [("f%d" % s, "i%d" % s, "0", "0", "0", "-9") for s in range(N)]
    return bim, fam
