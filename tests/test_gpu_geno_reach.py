"""Distance-windowed LD from .bed genotypes on the device (geno.hip: k_bed_band,
k_bed_corner with their row policies): a reach per row instead of one window, and
the triangular taper that keeps the windowed block positive semi-definite.

The definition (include/sgvamp_hip.h, "distance-windowed genotype LD"): for j >= i
entry (i, j) is kept iff j <= hi[i], hi[i] = max{j : pos[j] - pos[i] <= D};
everything else is exactly 0.0; with the taper a kept entry is acc * (1.0 - (pos[j]
- pos[i]) / D), formed in that order in f64.  Kept entries are sgv_geno_ld's sums,
so every comparison here is bitwise except those against the NumPy restatement
tests/bed_ref.R (maxrel < 1e-12, tests/test_gpu_geno_ld.py's bar for this
contraction), the products of cut against uncut bands (1e-12, tests/
test_gpu_parity.py's bar for coupled pieces) and the smallest eigenvalue (1e-9:
Weyl's bound n * max |dR| for n = 700 and entries within 1e-12).

Shapes: blocks of 130, 257 and 700 markers cross the 64-row tile and the 256-row
panel edges; the clustered positions (ties, gaps up to 400) give a reach from 0 to
124 at D = 4,000 and past 256 -- a panel and several tiles -- at D = 40,000; N in
{5, 130}: less than one 16-sample word, N % 4 = 2.  The cut case is 2,500 markers,
D = 4,000 (width 132), pieces [1024, 1476]."""
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse

import hip_backend as hb
from engine import Engine
from ldio import BedLD, read_bed, write_bed
from sgvamp import band_cuts

from tests import bed_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


def maxrel(a, b):
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def clustered(n):
    return np.cumsum(np.random.RandomState(3).choice([0, 1, 5, 50, 400], n,
                                                     p=[.1, .3, .3, .2, .1])).astype(np.float64)


def reach_of(pos, D):
    """hi by the predicate itself, one row at a time: forward from i while it holds
    (the positions are sorted, and rounding keeps the f64 difference monotone)."""
    p, n = [float(x) for x in pos], len(pos)
    hi = np.empty(n, dtype=np.int32)
    for i in range(n):
        j = i
        while j + 1 < n and p[j + 1] - p[i] <= D:
            j += 1
        hi[i] = j
    return hi


def kept(hi):
    i = np.arange(len(hi))
    up = (i[None, :] >= i[:, None]) & (i[None, :] <= np.asarray(hi)[:, None])
    return up | up.T


def weight(pos, D):
    """w[i][j] = 1.0 - (pos[max(i, j)] - pos[min(i, j)]) / D: one subtraction, one
    division, one subtraction, as the kernel forms it."""
    w = 1.0 - (pos[None, :] - pos[:, None]) / D
    return np.triu(w) + np.triu(w, 1).T


def band_format(n, bw):
    ext = -(-(256 + bw) // 256) * 256
    return 2 if ext < n else 1


def reach_csr(R, hi, full=False):
    """Upper triangle of R within the reach (full: both triangles) as CSR, every
    kept position stored explicitly."""
    n = R.shape[0]
    lo = np.array([int(np.argmax(np.asarray(hi) >= j)) for j in range(n)])   # first row reaching j
    cols = [np.arange(lo[i] if full else i, hi[i] + 1) for i in range(n)]
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])])
    return scipy.sparse.csr_matrix((np.concatenate([R[i, c] for i, c in enumerate(cols)]),
                                    np.concatenate(cols), indptr), shape=(n, n))


def stage(eng, blocks):
    N = blocks[0].shape[1]
    return [eng.geno_set_block(b, bed_ref.pack(c), N) for b, c in enumerate(blocks)]


# ---- uniform reach: the marker window's kernel, bit for bit -----------------------
USIZES = [130, 257, 700]
UOFFS = np.concatenate([[0], np.cumsum(USIZES)])


@functools.lru_cache(maxsize=None)
def upanel(N):
    codes = bed_ref.draw_codes(sum(USIZES), N, miss=0.03, seed=4000 + N)
    blocks = [codes[UOFFS[b]:UOFFS[b + 1]] for b in range(len(USIZES))]
    for a in blocks:
        a.setflags(write=False)
    return blocks


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("N", [5, 130])
@pytest.mark.parametrize("W", [1, 64, 300])
def test_uniform_reach_is_the_marker_window(W, N, bits):
    blocks = upanel(N)
    a, b = Engine(USIZES, K=1), Engine(USIZES, K=1)
    try:
        for eng in (a, b):
            eng.set_ld_precision(bits)
            stage(eng, blocks)
        for k, n in enumerate(USIZES):
            a.geno_ld_band(0, k, W)
            b.geno_ld_band_reach(0, k, np.minimum(np.arange(n) + W, n - 1))
        for k, n in enumerate(USIZES):
            assert b.ld_block_format(0, k) == a.ld_block_format(0, k) == band_format(n, min(W, n - 1))
            assert b.ld_block_precision(0, k) == bits
            np.testing.assert_array_equal(b.get_ld_block(0, k), a.get_ld_block(0, k))
        assert b.stored_bytes(0) == a.stored_bytes(0)
    finally:
        a.close()
        b.close()


# ---- ragged reach ----------------------------------------------------------------
RSIZES = [257, 700]
ROFFS = [0, 257, 957]


@functools.lru_cache(maxsize=None)
def rpanel(N, miss):
    """The case's codes per block, the reference R and the dense-triangle build
    (geno_ld) of each, computed once."""
    codes = bed_ref.draw_codes(sum(RSIZES), N, miss=miss, seed=5000 + N)
    blocks = [codes[ROFFS[b]:ROFFS[b + 1]] for b in range(2)]
    Rref = [bed_ref.R(c) for c in blocks]
    eng = Engine(RSIZES, K=1)
    try:
        stage(eng, blocks)
        for b in range(2):
            eng.geno_ld(0, b)
        T = [eng.get_ld_block(0, b) for b in range(2)]
    finally:
        eng.close()
    for x in blocks + Rref + T:
        x.setflags(write=False)
    return blocks, Rref, T


@functools.lru_cache(maxsize=None)
def rreach(D):
    pos = [clustered(n) for n in RSIZES]
    hi = [reach_of(p, D) for p in pos]
    return pos, hi


def build_reach(blocks, his, bits=64, pos=None, D=0.0):
    eng = Engine([c.shape[0] for c in blocks], K=1)
    eng.set_ld_precision(bits)
    stage(eng, blocks)
    for b, hi in enumerate(his):
        eng.geno_ld_band_reach(0, b, hi, None if pos is None else pos[b], D)
    return eng


@pytest.mark.parametrize("D", [4000.0, 40000.0])
@pytest.mark.parametrize("miss", [0.0, 0.03])
@pytest.mark.parametrize("N", [5, 130])
def test_ragged_reach_equals_masked_triangle_bitwise(N, miss, D):
    blocks, Rref, T = rpanel(N, miss)
    pos, his = rreach(D)
    widths = [int(np.max(h - np.arange(len(h)))) for h in his]
    assert all(int(np.min(h - np.arange(len(h)))) == 0 for h in his)
    assert (widths[1] > 256) == (D == 40000.0)       # past a panel and several tiles, or within
    eng = build_reach(blocks, his)
    ref = Engine(RSIZES, K=1)
    try:
        got = []
        for b, n in enumerate(RSIZES):
            keep = kept(his[b])
            assert eng.ld_block_format(0, b) == band_format(n, widths[b])
            assert eng.ld_block_precision(0, b) == 64
            R = eng.get_ld_block(0, b)
            np.testing.assert_array_equal(R, np.where(keep, T[b], 0.0))
            assert not R[~keep].any()                              # exactly 0 outside
            np.testing.assert_array_equal(R, R.T)
            err = maxrel(R, np.where(keep, Rref[b], 0.0))
            print("n=%d N=%d miss=%g D=%g width %d: maxrel %.3e" % (n, N, miss, D, widths[b], err))
            assert err < TOL, (n, err)
            got.append(R)
        # indistinguishable from the same matrix uploaded as CSR
        for b in range(2):
            ref.set_ld_block_csr(0, b, reach_csr(got[b], his[b]))
        assert [ref.ld_block_format(0, b) for b in range(2)] == \
            [eng.ld_block_format(0, b) for b in range(2)]
        assert eng.stored_bytes(0) == ref.stored_bytes(0)
        for b in range(2):
            np.testing.assert_array_equal(ref.get_ld_block(0, b), got[b])
        for ncol in (1, 4, 16):
            V = np.random.RandomState(ncol).normal(size=(ncol, sum(RSIZES)))
            np.testing.assert_array_equal(eng.ld_matvec(0, V), ref.ld_matvec(0, V))
    finally:
        eng.close()
        ref.close()


@pytest.mark.parametrize("bits", [64, 32])
def test_csr_route_f32_and_the_two_extremes(bits):
    """f32 against the CSR route at D = 4,000 (a packed band at n = 700); hi = i: the diagonal alone in the
    narrowest band (extent 256); hi = n - 1: the packed triangle, geno_ld's block."""
    N, miss = 130, 0.03
    blocks, _, T = rpanel(N, miss)
    _, his = rreach(4000.0)
    for kind in ("ragged", "diagonal", "triangle"):
        hs = his if kind == "ragged" else \
            [np.arange(n) if kind == "diagonal" else np.full(n, n - 1) for n in RSIZES]
        eng = build_reach(blocks, hs, bits)
        ref = Engine(RSIZES, K=1)
        try:
            ref.set_ld_precision(bits)
            got = [eng.get_ld_block(0, b) for b in range(2)]
            for b in range(2):
                want = np.where(kept(hs[b]), T[b], 0.0)
                np.testing.assert_array_equal(got[b], f32(want) if bits == 32 else want)
                ref.set_ld_block_csr(0, b, reach_csr(got[b], hs[b]))
            fmts = [eng.ld_block_format(0, b) for b in range(2)]
            assert fmts == [ref.ld_block_format(0, b) for b in range(2)]
            assert fmts == {"ragged": [1, 2], "diagonal": [2, 2], "triangle": [1, 1]}[kind]
            assert [eng.ld_block_precision(0, b) for b in range(2)] == [bits, bits]
            assert eng.stored_bytes(0) == ref.stored_bytes(0)
            if kind == "diagonal":   # extent 256: per panel its rows x min(256, columns left)
                assert eng.stored_bytes(0) == (bits // 8) * sum(
                    min(256, n - r0) ** 2 for n in RSIZES for r0 in range(0, n, 256))
            for b in range(2):
                np.testing.assert_array_equal(ref.get_ld_block(0, b), got[b])
            V = np.random.RandomState(4).normal(size=(4, sum(RSIZES)))
            np.testing.assert_array_equal(eng.ld_matvec(0, V), ref.ld_matvec(0, V))
        finally:
            eng.close()
            ref.close()


def test_narrower_reach_over_a_stored_band():
    """A second build of the same stored extent with a narrower reach leaves nothing
    of the first behind (the entry point zeroes the block)."""
    blocks, _, T = rpanel(130, 0.03)
    wide = [np.minimum(np.arange(n) + 200, n - 1) for n in RSIZES]
    _, his = rreach(4000.0)
    eng = build_reach(blocks, wide)
    try:
        for b in range(2):
            eng.geno_ld_band_reach(0, b, his[b])
            np.testing.assert_array_equal(eng.get_ld_block(0, b), np.where(kept(his[b]), T[b], 0.0))
    finally:
        eng.close()


@pytest.mark.parametrize("taper", [False, True])
def test_reach_past_a_panel_in_a_packed_band(taper):
    """n = 1,500 at D = 40,000: the reach passes 256 and the block is still a band
    (extent < n), so kept entries lie in the panels' columns past the diagonal
    block, up to the stored extent."""
    n, N, D = 1500, 130, 40000.0
    codes = bed_ref.draw_codes(n, N, miss=0.03, seed=5500)
    pos = clustered(n)
    hi = reach_of(pos, D)
    bw = int(np.max(hi - np.arange(n)))
    assert bw > 256 and band_format(n, bw) == 2
    tri = Engine([n], K=1)
    eng = build_reach([codes], [hi], 64, [pos] if taper else None, D)
    try:
        stage(tri, [codes])
        tri.geno_ld(0, 0)
        want = np.where(kept(hi), tri.get_ld_block(0, 0) * (weight(pos, D) if taper else 1.0), 0.0)
        assert eng.ld_block_format(0, 0) == 2
        np.testing.assert_array_equal(eng.get_ld_block(0, 0), want)
    finally:
        tri.close()
        eng.close()


# ---- taper -----------------------------------------------------------------------
@pytest.mark.parametrize("D", [4000.0, 40000.0])
@pytest.mark.parametrize("N,miss", [(5, 0.0), (130, 0.03)])
def test_taper_is_the_masked_triangle_times_the_weight_bitwise(N, miss, D):
    blocks, Rref, T = rpanel(N, miss)
    pos, his = rreach(D)
    e64 = build_reach(blocks, his, 64, pos, D)
    e32 = build_reach(blocks, his, 32, pos, D)
    try:
        for b, n in enumerate(RSIZES):
            keep, w = kept(his[b]), weight(pos[b], D)
            assert (w[keep] >= 0).all() and (np.diag(w) == 1.0).all()
            want = np.where(keep, T[b] * w, 0.0)
            R = e64.get_ld_block(0, b)
            np.testing.assert_array_equal(R, want)
            np.testing.assert_array_equal(R, R.T)
            np.testing.assert_array_equal(np.diag(R), np.diag(T[b]))      # R_ii = n_obs_i / N
            assert maxrel(R, np.where(keep, Rref[b] * w, 0.0)) < TOL
            assert e32.ld_block_precision(0, b) == 32
            assert not np.array_equal(R, f32(R))
            np.testing.assert_array_equal(e32.get_ld_block(0, b), f32(R))
            assert e32.ld_block_format(0, b) == e64.ld_block_format(0, b)
    finally:
        e64.close()
        e32.close()


def test_taper_marker_window_and_the_explicit_zero():
    """A tapered marker window (pos = the index, D = W + 1) on evenly spaced
    positions, and a distance window whose farthest kept entry is at d = D exactly:
    stored as 0.0, inside the band."""
    blocks, _, T = rpanel(130, 0.03)
    W = 70
    his = [np.minimum(np.arange(n) + W, n - 1) for n in RSIZES]
    pos = [np.arange(float(n)) for n in RSIZES]
    eng = build_reach(blocks, his, 64, pos, W + 1.0)
    try:
        for b in range(2):
            np.testing.assert_array_equal(
                eng.get_ld_block(0, b), np.where(kept(his[b]), T[b] * weight(pos[b], W + 1.0), 0.0))
            eng.geno_ld_band_reach(0, b, his[b], pos[b], float(W))       # d = D at the edge
            R = eng.get_ld_block(0, b)
            assert not np.diag(R, W).any() and np.diag(R, W - 1).all()
            np.testing.assert_array_equal(
                R, np.where(kept(his[b]), T[b] * weight(pos[b], float(W)), 0.0))
    finally:
        eng.close()


def test_taper_is_positive_definite_where_the_hard_window_is_not():
    """draw_codes(700, 130, miss=0.03, seed=7), the clustered positions, D = 4,000:
    the smallest eigenvalue of the fetched tapered block is within 1e-9 (Weyl: 700
    entries a row, each within 1e-12) of the NumPy restatement's, so > 0.1 (+0.118
    recorded), where the hard window of the same inputs is < -0.5 (-0.543)."""
    codes = bed_ref.draw_codes(700, 130, miss=0.03, seed=7)
    pos, D = clustered(700), 4000.0
    hi = reach_of(pos, D)
    assert int(np.max(hi - np.arange(700))) == 124
    keep, w, Rref = kept(hi), weight(pos, D), bed_ref.R(codes)
    got = {}
    for taper in (False, True):
        eng = build_reach([codes], [hi], 64, [pos] if taper else None, D)
        try:
            got[taper] = eng.get_ld_block(0, 0)
        finally:
            eng.close()
    lam = {t: float(np.linalg.eigvalsh(got[t])[0]) for t in got}
    ref = float(np.linalg.eigvalsh(np.where(keep, Rref * w, 0.0))[0])
    print("lambda_min: hard %.6f, tapered %+.6f (NumPy %+.6f)" % (lam[False], lam[True], ref))
    assert abs(lam[True] - ref) < 1e-9
    assert lam[True] > 0.1
    assert lam[False] < -0.5


# ---- band pieces and their couplings -----------------------------------------------
CUT_N, CUT_NS, CUT_KB, CUT_PIECES, CUT_BW = 2500, 500, 4.0, [1024, 1476], 132


@functools.lru_cache(maxsize=None)
def cut_codes():
    codes = bed_ref.draw_codes(CUT_N, CUT_NS, miss=0.03, seed=31)   # tests/test_gpu_geno_band.py's
    codes.setflags(write=False)
    return codes


def cut_bim(chrom=None, pos=None):
    pos = clustered(CUT_N) if pos is None else pos
    return [("1" if chrom is None else chrom[i], "rs%d" % i, "0", str(int(pos[i])), "A", "G")
            for i in range(CUT_N)]


@pytest.fixture(scope="module")
def cut_prefix(tmp_path_factory):
    return write_bed(str(tmp_path_factory.mktemp("cut") / "p"), cut_codes(), cut_bim(),
                     bed_ref.bim_fam(CUT_N, CUT_NS)[1])


def coupling_by_unit_vectors(eng, rows, cols):
    """out[a][c] = (R e_{cols[c]})[rows[a]]: products with 1.0 and zeros, exact."""
    out = np.empty((len(rows), len(cols)))
    for c0 in range(0, len(cols), 16):
        cc = cols[c0:c0 + 16]
        V = np.zeros((len(cc), CUT_N))
        V[np.arange(len(cc)), cc] = 1.0
        out[:, c0:c0 + len(cc)] = eng.ld_matvec(0, V)[:, rows].T
    return out


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("taper", [None, "triangle"])
def test_pieces_and_coupling_are_the_uncut_band(cut_prefix, taper, bits):
    L = BedLD(read_bed(cut_prefix), [CUT_N], window_kb=CUT_KB, taper=taper)
    assert L.band_width(0) == CUT_BW
    cuts = band_cuts([L], [CUT_N], piece=1024)
    assert cuts == [CUT_PIECES]
    P, cps = L.pieces(cuts)
    whole, cut = Engine([CUT_N], K=1), Engine(CUT_PIECES, K=1)
    try:
        for eng, src in ((whole, L), (cut, P)):
            eng.set_ld_precision(bits)
            for b in range(len(src.block_sizes)):
                src.upload(eng, 0, b)
        cps[0].upload(cut, 0, 0)
        assert whole.ld_block_format(0, 0) == 2
        assert [cut.ld_block_format(0, b) for b in range(2)] == [2, 2]
        R = whole.get_ld_block(0, 0)
        pos, hi = clustered(CUT_N), L.reach(0)
        np.testing.assert_array_equal(hi, reach_of(pos, 4000.0))
        want = np.where(kept(hi), bed_ref.R(cut_codes()) * (weight(pos, 4000.0) if taper else 1.0), 0.0)
        if bits == 32:
            np.testing.assert_array_equal(R, f32(R))
        assert maxrel(R, want) < (TOL if bits == 64 else TOL + 2.0 ** -24)
        assert not R[~kept(hi)].any()
        np.testing.assert_array_equal(cut.get_ld_block(0, 0), R[:1024, :1024])
        np.testing.assert_array_equal(cut.get_ld_block(0, 1), R[1024:, 1024:])
        # C, both ways round: the head's unit vectors give C's columns in the tail's
        # rows, the tail's unit vectors give C's rows in the head's
        bw = CUT_BW
        tail, head = np.arange(1024 - bw, 1024), np.arange(1024, 1024 + bw)
        C = R[1024 - bw:1024, 1024:1024 + bw]
        inside = np.arange(bw)[None, :] < np.clip(hi[tail] - 1023, 0, bw)[:, None]
        assert not C[~inside].any() and np.count_nonzero(C) > 1000   # a ragged corner, not a sliver
        np.testing.assert_array_equal(coupling_by_unit_vectors(cut, tail, head), C)
        np.testing.assert_array_equal(coupling_by_unit_vectors(cut, head, tail), C.T)
        # and nothing but C couples the pieces
        V = np.zeros((2, CUT_N))
        V[0, :1024 - bw], V[1, 1024 + bw:] = 1.0, 1.0
        Y = cut.ld_matvec(0, V)
        assert not Y[0, 1024:].any() and not Y[1, :1024].any()
        assert not R[:1024 - bw, 1024:].any() and not R[:1024, 1024 + bw:].any()
        # tests/test_gpu_parity.py's bar for coupled pieces against the whole band
        for ncol in (1, 4, 16):
            V = np.random.RandomState(ncol).normal(size=(ncol, CUT_N))
            Yc, Yw = cut.ld_matvec(0, V), whole.ld_matvec(0, V)
            for j in range(ncol):
                assert maxrel(Yc[j], Yw[j]) < 1e-12, (ncol, j, maxrel(Yc[j], Yw[j]))
                assert maxrel(Yc[j], R @ V[j]) < 1e-12, (ncol, j)
    finally:
        whole.close()
        cut.close()


# ---- refusals ------------------------------------------------------------------
def test_refusals(tmp_path):
    N = 130
    blocks, _, T = rpanel(N, 0.03)
    n0, n1 = RSIZES
    bad = np.array(blocks[1])
    bad[17] = 3                      # homozygous A2 everywhere
    up = np.arange(n0, dtype=np.int32)
    pos = np.arange(float(n0))
    eng = Engine(RSIZES, K=1)
    try:
        eng.geno_set_block(0, bed_ref.pack(blocks[0]), N)
        eng.geno_set_block(1, bed_ref.pack(bad), N)
        ok = np.minimum(up + 3, n0 - 1)
        eng.geno_ld_band_reach(0, 0, ok)
        with pytest.raises(hb.HipError, match=r"\(-4\).*1 marker\(s\) without LD"):
            eng.geno_ld_band_reach(0, 1, np.arange(n1))
        assert [eng.ld_block_format(0, b) for b in range(2)] == [1, -1]
        eng.geno_set_block(1, bed_ref.pack(blocks[1]), N)
        eng.geno_ld_band_reach(0, 1, np.minimum(np.arange(n1) + 3, n1 - 1))
        before = eng.get_ld_block(0, 0)
        for at, val, where in ((5, 4, 5), (n0 - 1, n0, n0 - 1), (5, 10, 6)):   # < i, > n - 1, decreasing
            hi = ok.copy()
            hi[at] = val
            with pytest.raises(hb.HipError, match=r"\(-2\).*reach hi\[%d\]" % where):
                eng.geno_ld_band_reach(0, 0, hi)
        for p, span, msg in ((pos, 0.0, "span"), (pos, float("nan"), "span"),
                             (pos, float("inf"), "span"), (pos, -1.0, "span"),
                             (np.where(up == 9, np.nan, pos), 5.0, "not finite"),
                             (np.where(up == 9, np.inf, pos), 5.0, "not finite"),
                             (np.where(up == 9, 7.5, pos), 5.0, "positions decrease"),
                             (pos, 2.5, "weight would be negative")):
            with pytest.raises(hb.HipError, match=r"\(-2\).*" + msg):
                eng.geno_ld_band_reach(0, 0, ok, p, span)
        with pytest.raises(ValueError, match="the block has 257 markers"):
            eng.geno_ld_band_reach(0, 0, ok[:-1])
        eng.set_ld_packing(False)
        with pytest.raises(hb.HipError, match=r"\(-4\).*packing is off"):
            eng.geno_ld_band_reach(0, 0, ok)
        eng.set_ld_packing(True)
        np.testing.assert_array_equal(eng.get_ld_block(0, 0), before)   # untouched by every refusal
        # the coupling: keep outside [0, nc], decreasing, a negative weight, no such piece
        rows = bed_ref.pack(np.concatenate([blocks[0][-4:], blocks[1][:4]]))
        p8 = np.arange(8.0)
        eng.geno_coupling_reach(0, 0, 4, 4, rows, N, [0, 1, 2, 3])
        V = np.zeros((1, n0 + n1))
        V[0, n0:n0 + 4] = 1.0
        before = eng.ld_matvec(0, V)
        assert before[0, n0 - 4:n0].any()
        for keep, p, span, msg in (([0, 1, 2, 5], None, 0.0, r"keep\[3\] = 5"),
                                   ([-1, 1, 2, 3], None, 0.0, r"keep\[0\] = -1"),
                                   ([0, 2, 1, 3], None, 0.0, r"keep\[2\] = 1"),
                                   ([0, 1, 2, 3], p8, 0.0, "span"),
                                   ([0, 1, 2, 3], p8[::-1].copy(), 9.0, "positions decrease"),
                                   ([0, 1, 2, 4], p8, 3.5, "weight would be negative")):
            with pytest.raises(hb.HipError, match=r"\(-2\).*" + msg):
                eng.geno_coupling_reach(0, 0, 4, 4, rows, N, keep, p, span)
        with pytest.raises(hb.HipError, match=r"\(-2\)"):
            eng.geno_coupling_reach(0, 1, 4, 4, rows, N, [0, 1, 2, 3])   # no piece 2
        badrows = bed_ref.pack(np.concatenate([blocks[0][-4:], bad[15:19]]))
        with pytest.raises(hb.HipError, match=r"\(-4\).*1 marker\(s\) without LD"):
            eng.geno_coupling_reach(0, 0, 4, 4, badrows, N, [0, 1, 2, 3])
        np.testing.assert_array_equal(eng.ld_matvec(0, V), before)      # the coupling as it was
        eng.geno_coupling_reach(0, 0, 4, 4, rows, N, [0, 0, 0, 0])        # all zero: no coupling
        assert not eng.ld_matvec(0, V)[0, :n0].any()
        eng.geno_clear()
        with pytest.raises(hb.HipError, match=r"\(-4\).*no genotypes"):
            eng.geno_ld_band_reach(0, 0, ok)
    finally:
        eng.close()
    # through BedLD: the marker is named, in a block and in a halo, and nothing is stored
    codes = np.concatenate([blocks[0], bad])
    bim = [("1", "rs%d" % i, "0", str(100 * i), "A", "G") for i in range(n0 + n1)]
    prefix = write_bed(str(tmp_path / "p"), codes, bim, bed_ref.bim_fam(1, N)[1])
    L = BedLD(read_bed(prefix), RSIZES, window_kb=1.0, taper="triangle")
    eng = Engine(RSIZES, K=1)
    try:
        L.upload(eng, 0, 0)
        with pytest.raises(ValueError, match=r"1 marker\(s\) of LD block 1 have no LD.*rs274"):
            L.upload(eng, 0, 1)
        assert [eng.ld_block_format(0, b) for b in range(2)] == [1, -1]
        eng.set_ld_packing(False)
        with pytest.raises(ValueError, match="needs LD packing on"):
            L.upload(eng, 0, 0, packed=False)
    finally:
        eng.close()
    one = BedLD(read_bed(prefix), [n0 + n1], window_kb=1.0, taper="triangle")
    P, cps = one.pieces([[267, 690]])          # rs274 is the 8th row of the head's halo
    assert (cps[0].nr, cps[0].nc) == (10, 10)
    eng = Engine([267, 690], K=1)
    try:
        P.upload(eng, 0, 0)
        with pytest.raises(ValueError, match=r"1 marker\(s\) of the coupling between LD band "
                                             r"pieces 0 and 1 have no LD.*rs274"):
            cps[0].upload(eng, 0, 0)
        assert [eng.ld_block_format(0, b) for b in range(2)] == [1, -1]
    finally:
        eng.close()


# ---- one rank against two ranks --------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("precision,taper", [("f64", "triangle"), ("f32", "triangle"),
                                             ("f64", "none"), ("f32", "none")])
def test_one_rank_vs_two_ranks_bitwise(precision, taper):
    """tests/test_gpu_multirank.py's harness (ranks on one device, host exchange):
    the 2,500-marker panel at 4 kb in pieces [1024, 1476], one piece per rank, the
    coupling spanning the two: the stored pieces and the 5-iteration xhat / r1
    files equal one rank's, bit for bit (tools/geno_reach_ranks_gpu.py)."""
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2",
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), SGV_EXCHANGE="host",
                   SGV_BAND_PIECE="1024")
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(ROOT, "tools", "geno_reach_ranks_gpu.py"), precision,
             taper], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(out)
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, out[-4000:])
    assert "bitwise equal -> OK" in outs[0], outs[0][-3000:]


# ---- command line ----------------------------------------------------------------
CHR_SIZES = [2100, 400]     # the first chromosome spans two band pieces of 1,024


@pytest.fixture(scope="module")
def chr_prefix(tmp_path_factory):
    """The cut panel on two chromosomes, the positions restarting at the second."""
    pos = np.concatenate([clustered(n) for n in CHR_SIZES])
    chrom = ["1"] * CHR_SIZES[0] + ["2"] * CHR_SIZES[1]
    return write_bed(str(tmp_path_factory.mktemp("chr") / "p"), cut_codes(), cut_bim(chrom, pos),
                     bed_ref.bim_fam(CUT_N, CUT_NS)[1])


@functools.lru_cache(maxsize=None)
def cli_inputs():
    """tests/test_gpu_geno_band.py's r and beta recipe on its panel."""
    codes = cut_codes()
    rs = np.random.RandomState(5)
    beta = np.zeros(CUT_N)
    beta[rs.choice(CUT_N, 100, replace=False)] = rs.normal(0, np.sqrt(0.8 / 100), 100)
    y = bed_ref.g(codes, beta) + rs.normal(0, np.sqrt(0.2), CUT_NS)
    return bed_ref.r(codes, y), beta


CLI = {   # flags on the .bed, the BedLD of the same, --s, the partition without / with the piece
    "kb": (["--ld-block-size", str(CUT_N), "--ld-window-kb", "4"],
           dict(window_kb=4.0), "0.3", [CUT_N], CUT_PIECES),
    "taper": (["--ld-block-size", str(CUT_N), "--ld-window", "200", "--ld-taper", "triangle"],
              dict(window=200, taper="triangle"), "0", [CUT_N], CUT_PIECES),
    "chr": (["--ld-chr-blocks", "--ld-window-kb", "4", "--ld-taper", "triangle"],
            dict(window_kb=4.0, taper="triangle"), "0", CHR_SIZES, [1024, 1076, 400]),
}


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("piece", [None, 1024])
@pytest.mark.parametrize("case", sorted(CLI))
def test_cli_equals_npz_of_the_band(tmp_path, cut_prefix, chr_prefix, monkeypatch, case, piece,
                                    precision):
    """main.py with the new flags on the .bed (K = 2 cohorts sharing it, 5
    iterations) against main.py on an .npz CSR of the uncut band fetched with
    get_ld_block, every kept position explicit, under the same band piece: every
    output file byte-identical.  The tapered marker window solves at --s 0, where
    the hard window of this panel (smallest eigenvalue -0.298) gives nothing: the
    CPU oracle's corr(xhat, beta) is 0.489 tapered against 0.078 hard."""
    import main
    import sgvamp

    if piece is not None:
        monkeypatch.setattr(sgvamp, "BAND_PIECE", piece)
    flags, kw, s, sizes, pieces = CLI[case]
    prefix = chr_prefix if case == "chr" else cut_prefix
    r, beta = cli_inputs()
    np.save(tmp_path / "r.npy", r.reshape(-1, 1))
    np.save(tmp_path / "beta.npy", beta.reshape(-1, 1))
    seen = []

    def run(ld, out, extra):
        (tmp_path / out).mkdir()
        main.main(["--ld-files", "%s,%s" % (ld, ld), "--r-files",
                   "%s,%s" % (tmp_path / "r.npy", tmp_path / "r.npy"),
                   "--true-signal-file", str(tmp_path / "beta.npy"), "--out-dir",
                   str(tmp_path / out), "--out-name", "run", "--N", "%d,%d" % (CUT_NS, CUT_NS),
                   "--M", "%d,%d" % (CUT_N, CUT_N), "--K", "2", "--iterations", "5", "--seed", "11",
                   "--prior-probs", "0.9,0.1", "--s", s, "--ld-precision", precision] + extra)
        return {fn: open(tmp_path / out / fn, "rb").read()
                for fn in sorted(os.listdir(tmp_path / out))}

    real = Engine.__init__

    def spy(self, block_sizes, *a, **kw):
        seen.append(list(block_sizes))
        real(self, block_sizes, *a, **kw)

    monkeypatch.setattr(Engine, "__init__", spy)
    a = run(prefix + ".bed", "bed", flags)
    monkeypatch.setattr(Engine, "__init__", real)
    assert seen == [pieces if piece else sizes]
    L = BedLD(read_bed(prefix), sizes, **kw)
    eng = Engine(sizes, K=1)
    try:
        eng.set_ld_precision(32 if precision == "f32" else 64)
        for b in range(len(sizes)):
            L.upload(eng, 0, b)
        mats = [reach_csr(eng.get_ld_block(0, b), L.reach(b), full=True)
                for b in range(len(sizes))]
    finally:
        eng.close()
    A = scipy.sparse.block_diag(mats, format="csr")
    assert A.nnz == sum(2 * int(np.sum(L.reach(b) - np.arange(n))) + n for b, n in enumerate(sizes))
    scipy.sparse.save_npz(tmp_path / "R.npz", A)
    b = run(str(tmp_path / "R.npz"), "npz", [])
    assert a.keys() == b.keys()
    assert sum(fn.endswith(".bin") for fn in a) == 5 * 3 and "run_metrics.csv" in a
    for fn in a:
        assert a[fn] == b[fn], fn
    x = np.frombuffer(a["run_xhat_it_4.bin"])
    assert np.isfinite(x).all() and x.any()
    if case == "taper":
        corr = float(np.corrcoef(x, beta)[0, 1])
        print("tapered W = 200, --s 0, %s: corr(xhat, beta) = %.3f" % (precision, corr))
        assert corr >= 0.4
