"""Scoring a target panel with saved effects (csrc/score.hip, sgv_score_begin /
_chunk / _end): S[n][c] = sum_i tab_i[code_in] B[i][c] on the f64 matrix cores.

Extents the kernel cuts the work by, and the shapes that cross them:
  samples  16 (an MFMA's rows: one word of a .bed row), 64 (a wave's four
           groups), 256 (a workgroup): N = 5, 16, 17, 63, 250, 256, 257, 1027;
  markers  4 (an MFMA's K), 128 (an LDS tile), 1,024 (a slab partial): M = 1, 3, 4,
           5, 1023, 1024, 1025, 2500;
  columns  16 (a column group): 1, 2, 5, 15, 16, 17, 33, 64.

1. exact: integer tables and effects, equal to ONE int64 reference bit for bit,
   also with longer rows whose padding holds each of the four codes, and in RAW
   mode on panels without missing genotypes.
2. chunk independence, 3. column independence: bitwise.
4. general panels against np.longdouble references within the derived bound
   2 (M + 16) 2^-53 (|X|^T |beta|), monomorphic and unobserved markers included.
5. the one-column path sgv_geno_g within the same bound.
6. refusals, and that scoring leaves an LD block, its passes and the LD timers
   alone.
"""
import functools

import numpy as np
import pytest

import hip_backend as hb
from engine import Engine

from tests import bed_ref
from tests import score_ref as sr

pytestmark = pytest.mark.gpu

NS = [5, 16, 17, 63, 250, 256, 257, 1027]
MS = [1, 3, 4, 5, 1023, 1024, 1025, 2500]
NCOLS = [1, 2, 5, 15, 16, 17, 33, 64]
# every N with M in {5, 1025}, every M with N in {17, 257}; the column counts cycle
# (offset per family so each family meets all eight)
EXACT_CASES = sorted({(N, M, NCOLS[(a + b) % 8]) for a, N in enumerate(NS) for b, M in enumerate(MS)
                      if M in (5, 1025) or N in (17, 257)})
ARG, STATE = "(-2)", "(-4)"


@pytest.fixture(scope="module")
def eng():
    e = Engine([64], K=1)
    yield e
    e.close()


def stream(e, rows, N, beta, mode=hb.SCORE_TARGET, tab=None, chunk=None):
    """One whole scoring stream over rows in chunks of `chunk` markers (None: one
    chunk): (ncol, N) scores and the (M, 4) counts."""
    beta = np.atleast_2d(beta)
    M = rows.shape[0]
    step = M if chunk is None else chunk
    e.score_begin(N, beta.shape[0])
    cnt = []
    for i in range(0, M, step):
        j = min(M, i + step)
        cnt.append(e.score_chunk(rows[i:j], beta[:, i:j], mode=mode,
                                 tab=None if tab is None else tab[i:j]))
    return e.score_end(), np.concatenate(cnt)


# ---- 1. exact ---------------------------------------------------------------------
@pytest.mark.parametrize("N,M,ncol", EXACT_CASES)
def test_exact(eng, N, M, ncol):
    rs = np.random.RandomState([N, M, ncol])
    codes = rs.randint(0, 4, size=(M, N)).astype(np.int64)
    tab = rs.randint(-2, 3, size=(M, 4)).astype(np.int64)
    beta = rs.randint(-8, 9, size=(ncol, M)).astype(np.int64)
    ref = (sr.x_of(codes, tab).T @ beta.T).T                     # int64, exact
    assert np.abs(ref).max() < 2 ** 40
    tabf, betaf = tab.astype(np.float64), beta.astype(np.float64)
    S, cnt = stream(eng, bed_ref.pack(codes), N, betaf, hb.SCORE_TABLE, tabf)
    assert np.array_equal(S, ref.astype(np.float64))
    np.testing.assert_array_equal(cnt, bed_ref.counts(codes))
    nb = (N + 3) // 4 + 5
    for pad in range(4):
        S, cnt = stream(eng, bed_ref.pack(codes, row_bytes=nb, pad_bits=pad), N, betaf,
                        hb.SCORE_TABLE, tabf)
        assert np.array_equal(S, ref.astype(np.float64)), pad
        np.testing.assert_array_equal(cnt, bed_ref.counts(codes))
    # RAW on a panel without missing genotypes: dosages 2 / 1 / 0 are exact
    craw = np.array([0, 2, 3])[rs.randint(0, 3, size=(M, N))].astype(np.int64)
    xr = sr.x_raw(craw)
    refr = (np.rint(xr).astype(np.int64).T @ beta.T).T
    assert np.array_equal(xr, np.rint(xr))
    S, _ = stream(eng, bed_ref.pack(craw, row_bytes=nb, pad_bits=1), N, betaf, hb.SCORE_RAW)
    assert np.array_equal(S, refr.astype(np.float64))


# ---- 4. general panels (their data also serves 2, 3 and 5) -------------------------
@functools.lru_cache(maxsize=None)
def general(M, N, miss, ncol, seed=11):
    """A raw draw (markers without variance are kept; some are forced), its packed
    rows, normal effects, and the longdouble references of both modes."""
    rs = np.random.RandomState([seed, M, N, int(miss * 100), ncol])
    codes = bed_ref._draw(rs, M, N, miss)
    if M >= 8:
        codes[M // 3] = 3                        # monomorphic
        codes[M // 2] = 1                        # unobserved
        codes[M - 2] = np.where(np.arange(N) % 2 == 0, 0, 1)   # one value among the observed
    beta = rs.normal(size=(ncol, M)) / np.sqrt(M)
    Xt, Xr = sr.x_target(codes), sr.x_raw(codes)
    out = dict(codes=codes, rows=bed_ref.pack(codes), beta=beta, Xt=Xt, Xr=Xr,
               St=sr.scores(Xt, beta), Sr=sr.scores(Xr, beta),
               Bt=sr.bound(Xt, beta), Br=sr.bound(Xr, beta))
    for v in out.values():
        v.setflags(write=False)
    return out


def within(S, ref, bnd):
    err = np.abs(S.astype(np.longdouble) - ref).astype(np.float64)
    worst = float(np.max(err / np.maximum(bnd, np.finfo(float).tiny)))
    print("max err / bound = %.3g" % worst)
    return bool(np.all(err <= bnd))


@pytest.mark.parametrize("miss", [0.0, 0.03])
@pytest.mark.parametrize("N", [5, 130, 500, 1027])
def test_general(eng, N, miss):
    M = 1501
    d = general(M, N, miss, 3)
    bad = bed_ref.unusable(d["codes"])
    assert bad.sum() >= 3                        # they score 0 and are in the counts
    S, cnt = stream(eng, d["rows"], N, d["beta"], hb.SCORE_TARGET)
    np.testing.assert_array_equal(cnt, bed_ref.counts(d["codes"]))
    assert within(S, d["St"], d["Bt"])
    only_bad = np.where(bad[None, :], d["beta"], 0.0)
    Z, _ = stream(eng, d["rows"], N, only_bad, hb.SCORE_TARGET)
    assert np.array_equal(Z, np.zeros_like(Z))
    S, cnt = stream(eng, d["rows"], N, d["beta"], hb.SCORE_RAW)
    np.testing.assert_array_equal(cnt, bed_ref.counts(d["codes"]))
    assert within(S, d["Sr"], d["Br"])


# ---- 2. chunk independence ---------------------------------------------------------
@pytest.mark.parametrize("M", [2500, 5000])
def test_chunk_independence(eng, M):
    N = 130
    d = general(M, N, 0.03, 17)
    for mode, ref, bnd in ((hb.SCORE_TARGET, d["St"], d["Bt"]), (hb.SCORE_RAW, d["Sr"], d["Br"])):
        one, _ = stream(eng, d["rows"], N, d["beta"], mode)
        assert within(one, ref, bnd)
        for chunk in (1024, 2048):
            S, _ = stream(eng, d["rows"], N, d["beta"], mode, chunk=chunk)
            assert np.array_equal(S, one), (mode, chunk)


# ---- 3. column independence --------------------------------------------------------
def test_column_independence(eng):
    M, N = 1501, 500
    d = general(M, N, 0.03, 40)
    beta = d["beta"]
    full, _ = stream(eng, d["rows"], N, beta)
    assert within(full, d["St"], d["Bt"])
    g16, _ = stream(eng, d["rows"], N, beta[:16])
    g5, _ = stream(eng, d["rows"], N, beta[:5])
    assert np.array_equal(g16, full[:16]) and np.array_equal(g5, full[:5])
    for c in (0, 4, 15, 16, 31, 32, 39):
        alone, _ = stream(eng, d["rows"], N, beta[c:c + 1])
        assert np.array_equal(alone[0], full[c]), c
    # a column's place in its group does not matter either
    moved, _ = stream(eng, d["rows"], N, beta[[39, 3, 20]])
    assert np.array_equal(moved, full[[39, 3, 20]])


# ---- 5. the one-column path --------------------------------------------------------
@pytest.mark.parametrize("N", [130, 1027])
def test_against_geno_g(eng, N):
    M = 700
    codes = bed_ref.draw_codes(M, N, 0.03, seed=5)
    rows = bed_ref.pack(codes)
    beta = np.random.RandomState(6).normal(size=M) / np.sqrt(M)
    X = sr.x_target(codes)
    e2 = Engine([M], K=1)
    try:
        e2.geno_set_block(0, rows, N)
        g = e2.geno_g(beta, N)[0]
        S, _ = stream(e2, rows, N, beta)         # beside the staged block
        np.testing.assert_array_equal(e2.geno_g(beta, N)[0], g)   # which it left alone
    finally:
        e2.close()
    bnd = sr.bound(X, beta[None, :])[0]
    assert np.all(np.abs(S[0] - g) <= bnd)
    assert within(S, sr.scores(X, beta[None, :]), bnd[None, :])


# ---- 6. state ----------------------------------------------------------------------
def refused(code, fn, *args):
    with pytest.raises(hb.HipError) as ei:
        fn(*args)
    assert code in str(ei.value), str(ei.value)


def test_refusals_leave_the_stream_alone():
    M, N, ncol = 1524, 130, 3
    d = general(M, N, 0.03, ncol)
    rows, beta = d["rows"], np.ascontiguousarray(d["beta"])
    e = Engine([64], K=1)
    try:
        ctx = e.ctx
        u8 = lambda a: a.ctypes.data_as(hb._c_u8_p)
        cnt = np.empty((M, 4), dtype=np.int64)
        cp = cnt.ctypes.data_as(hb._c_i64_p)
        nb = rows.shape[1]
        refused(STATE, ctx.sgv_score_chunk, u8(rows), nb, 4, hb.SCORE_RAW, None, hb.dptr(beta), M, cp)
        refused(STATE, ctx.sgv_score_end, hb.dptr(np.empty((ncol, N))))
        for bad in ((0, 1), (N, 0), (N, hb.SCORE_MAXCOL + 1), (-3, 2)):
            refused(ARG, ctx.sgv_score_begin, *bad)
        want, _ = stream(e, rows, N, beta, hb.SCORE_RAW)

        def refusals():
            b0 = np.ascontiguousarray(beta[:, :4])
            tab = np.zeros((4, 4))
            refused(ARG, ctx.sgv_score_begin, N, 0)
            refused(ARG, ctx.sgv_score_chunk, u8(rows), nb - 1, 4, hb.SCORE_RAW, None, hb.dptr(b0), 4, cp)
            refused(ARG, ctx.sgv_score_chunk, u8(rows), nb, 0, hb.SCORE_RAW, None, hb.dptr(b0), 4, cp)
            refused(ARG, ctx.sgv_score_chunk, u8(rows), nb, 4, 3, None, hb.dptr(b0), 4, cp)
            refused(ARG, ctx.sgv_score_chunk, u8(rows), nb, 4, hb.SCORE_TABLE, None, hb.dptr(b0), 4, cp)
            refused(ARG, ctx.sgv_score_chunk, u8(rows), nb, 4, hb.SCORE_RAW, None, hb.dptr(b0), 3, cp)
            refused(ARG, ctx.sgv_score_chunk, None, nb, 4, hb.SCORE_RAW, None, hb.dptr(b0), 4, cp)
            refused(ARG, ctx.sgv_score_chunk, u8(rows), nb, 4, hb.SCORE_RAW, None, None, 4, cp)
            refused(ARG, ctx.sgv_score_chunk, u8(rows), nb, 4, hb.SCORE_RAW, None, hb.dptr(b0), 4, None)
            for v in (np.nan, np.inf, -np.inf):
                tab[2, 1] = v
                refused(ARG, ctx.sgv_score_chunk, u8(rows), nb, 4, hb.SCORE_TABLE, hb.dptr(tab),
                        hb.dptr(b0), 4, cp)
            refused(ARG, ctx.sgv_score_end, None)

        e.score_begin(N, ncol)
        refusals()
        e.score_chunk(rows[:1024], beta[:, :1024], mode=hb.SCORE_RAW)
        refusals()
        e.score_chunk(rows[1024:], beta[:, 1024:], mode=hb.SCORE_RAW)     # 500: the ragged last chunk
        refusals()
        # a chunk after the ragged one: detected here, and the stream still ends right
        with pytest.raises(hb.HipError) as ei:
            e.score_chunk(rows[:4], beta[:, :4], mode=hb.SCORE_RAW)
        assert ARG in str(ei.value) and "1024" in str(ei.value)
        got = e.score_end()
        assert np.array_equal(got, want)
        refused(STATE, ctx.sgv_score_end, hb.dptr(got))                   # the stream has ended
    finally:
        e.close()


def test_scoring_leaves_ld_alone():
    n, N, M = 300, 257, 1100
    rs = np.random.RandomState(3)
    A = rs.normal(size=(2 * n, n)) / np.sqrt(2 * n)
    R = A.T @ A
    V = rs.normal(size=(2, n))
    d = general(M, N, 0.03, 17)
    e = Engine([n], K=1)
    try:
        e.set_ld_block(0, 0, R)
        y0 = e.ld_matvec(0, V)
        t0 = e.timers()
        S, _ = stream(e, d["rows"], N, d["beta"], chunk=1024)
        t1 = e.timers()
        for k in ("ld_launches", "ld_bytes", "rhs_bytes", "dense_bytes", "aux_bytes", "ld_flops",
                  "wide_flops", "wide_launches", "ld_ms", "wide_ms"):
            assert t1[k] == t0[k], k
        assert np.array_equal(e.ld_matvec(0, V), y0)
        assert within(S, d["St"], d["Bt"])
        st = e.score_timers()
        assert st["chunks"] == 2 and st["flops"] == 2.0 * N * M * 17 and st["kernel_ms"] > 0
    finally:
        e.close()
