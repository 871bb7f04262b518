"""NumPy restatement of scoring (include/sgvamp_hip.h, "scoring"), for the tests:
the per-marker tables of the three modes, S = X^T B with X[i][n] = tab_i[code_in],
the derived error bound, and the host statistics.  Built on tests/bed_ref.py's
decode, counts and X_std; independent of score.py and of the device code."""
import numpy as np

from tests import bed_ref

U = 2.0 ** -53


def x_target(codes):
    """(n, N): bed_ref.X_std on the markers that have variance in THIS panel, 0 on
    the monomorphic and unobserved ones (TARGET mode)."""
    codes = np.asarray(codes)
    ok = ~bed_ref.unusable(codes)
    X = np.zeros(codes.shape)
    if ok.any():
        X[ok] = bed_ref.X_std(codes[ok])
    return X


def tab_raw(codes):
    """(n, 4): A1 dosage 2 / 1 / 0 by code, missing -> S1 / n_obs (0 if unobserved)."""
    nobs, s1, _ = bed_ref.moments(codes)
    t = np.zeros((np.asarray(codes).shape[0], 4))
    t[:, 0], t[:, 2] = 2.0, 1.0
    has = nobs > 0
    t[has, 1] = s1[has].astype(np.float64) / nobs[has].astype(np.float64)
    return t


def x_of(codes, tab):
    """(n, N): X[i][s] = tab[i][codes[i][s]]."""
    return np.take_along_axis(np.asarray(tab), np.asarray(codes), axis=1)


def x_raw(codes):
    return x_of(codes, tab_raw(codes))


def scores(X, beta, dtype=np.longdouble):
    """(ncol, N): S[c][n] = sum_i X[i][n] beta[c][i], accumulated in dtype."""
    return (np.asarray(X, dtype=dtype).T @ np.asarray(beta, dtype=dtype).T).T


def bound(X, beta):
    """(ncol, N): 2 (M + 16) 2^-53 (|X|^T |beta|): the sequential-sum bound of an M-
    term dot product, a factor 2 for the table entries' own rounding."""
    M = np.asarray(X).shape[0]
    return 2.0 * (M + 16) * U * np.asarray(scores(np.abs(X), np.abs(beta)), dtype=np.float64)


def pearson(x, y):
    """Pearson correlation in f64 over the entries where y is finite, and how many
    those are; nan with fewer than two of them or a constant side."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    m = np.isfinite(y)
    n = int(m.sum())
    if n < 2:
        return float("nan"), n
    dx, dy = x[m] - x[m].mean(), y[m] - y[m].mean()
    den = np.sqrt((dx * dx).sum() * (dy * dy).sum())
    return (float((dx * dy).sum() / den) if den > 0 else float("nan")), n
