"""Windowed LD from .bed genotypes on the device (geno.hip: k_bed_band, k_bed_corner
with their window policies): packed bands and the couplings of band pieces, formed
from the bits.

The definition (include/sgvamp_hip.h, "windowed genotype LD"): R[i][j] = (G G^T)[i][j]
where |i - j| <= W, exactly 0 elsewhere.  The band is required to equal the
dense-triangle build (sgv_geno_ld) masked to the window ENTRY FOR ENTRY, so most
checks here are bitwise; against the NumPy restatement tests/bed_ref.R the bar is
maxrel < 1e-12, tests/test_gpu_geno_ld.py's for this contraction.

Shapes: blocks of 130, 257, 700 and 1,500 markers cross the 64-row tile and the
256-row panel edges; windows 1, 63, 64, 255, 256, 300 and n - 1 cross the tile
edge, the panel edge and every stored extent (512, 768 and the packed triangle);
N in {5, 130, 1027}: less than one 16-sample word, N % 4 = 2, N % 16 = 3.  The
cut case is 2,500 markers, W = 200, pieces [1024, 1476]."""
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
SIZES = [130, 257, 700, 1500]
OFFS = np.concatenate([[0], np.cumsum(SIZES)])
WINDOWS = [1, 63, 64, 255, 256, 300, "n-1"]
NS = [5, 130, 1027]
MISS = [0.0, 0.03]
TOL = 1e-12


def maxrel(a, b):
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def win(W, n):
    return n - 1 if W == "n-1" else W


def masked(R, W):
    i = np.arange(R.shape[0])
    return np.where(np.abs(i[:, None] - i[None, :]) <= W, R, 0.0)


def band_format(n, W):
    """sgv_set_ld_block_csr's rule: 2 (packed band) or 1 (packed triangle)."""
    ext = -(-(256 + min(W, n - 1)) // 256) * 256
    return 2 if ext < n else 1


def band_csr(R, W, full=False):
    """Upper triangle of R within the window (full: both triangles) as CSR, every
    in-band position stored explicitly (an exact-zero correlation cannot narrow
    the band)."""
    n = R.shape[0]
    cols = [np.arange(max(i - W, 0) if full else i, min(i + W, n - 1) + 1) for i in range(n)]
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])])
    indices = np.concatenate(cols)
    data = np.concatenate([R[i, c] for i, c in enumerate(cols)])
    return scipy.sparse.csr_matrix((data, indices, indptr), shape=(n, n))


def stage(eng, blocks):
    N = blocks[0].shape[1]
    return [eng.geno_set_block(b, bed_ref.pack(c), N) for b, c in enumerate(blocks)]


@functools.lru_cache(maxsize=None)
def panel(N, miss):
    """The case's codes per block and their reference R, computed once."""
    codes = bed_ref.draw_codes(sum(SIZES), N, miss=miss, seed=2000 + N)
    assert not bed_ref.unusable(codes).any()
    blocks = [codes[OFFS[b]:OFFS[b + 1]] for b in range(len(SIZES))]
    R = [bed_ref.R(c) for c in blocks]
    for a in blocks + R:
        a.setflags(write=False)
    return blocks, R


@functools.lru_cache(maxsize=None)
def triangle(N, miss, bits=64):
    """The blocks as the existing dense-triangle build (geno_ld) stores them."""
    blocks, _ = panel(N, miss)
    eng = Engine(SIZES, K=1)
    try:
        eng.set_ld_precision(bits)
        stage(eng, blocks)
        for b in range(len(SIZES)):
            eng.geno_ld(0, b)
        T = [eng.get_ld_block(0, b) for b in range(len(SIZES))]
    finally:
        eng.close()
    for t in T:
        t.setflags(write=False)
    return T


def build_bands(N, miss, W, bits=64):
    """An engine whose blocks are the windowed bands (caller closes it)."""
    blocks, _ = panel(N, miss)
    eng = Engine(SIZES, K=1)
    eng.set_ld_precision(bits)
    stage(eng, blocks)
    for b, n in enumerate(SIZES):
        eng.geno_ld_band(0, b, win(W, n))
    return eng


@pytest.mark.parametrize("miss", MISS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("W", WINDOWS)
def test_band_equals_masked_triangle_bitwise(W, N, miss):
    blocks, Rref = panel(N, miss)
    T = triangle(N, miss)
    eng = build_bands(N, miss, W)
    try:
        for b, n in enumerate(SIZES):
            w = win(W, n)
            assert eng.ld_block_format(0, b) == band_format(n, w)
            assert eng.ld_block_precision(0, b) == 64
            R = eng.get_ld_block(0, b)
            np.testing.assert_array_equal(R, masked(T[b], w))
            i = np.arange(n)
            assert not R[np.abs(i[:, None] - i[None, :]) > w].any()   # exactly 0 outside
            np.testing.assert_array_equal(R, R.T)
            err = maxrel(R, masked(Rref[b], w))
            print("n=%d W=%s N=%d miss=%g: maxrel %.3e" % (n, W, N, miss, err))
            assert err < TOL, (n, err)
            nobs = bed_ref.moments(blocks[b])[0]
            assert np.max(np.abs(np.diag(R) - nobs / N)) < 1e-12
    finally:
        eng.close()


def test_narrower_window_over_a_stored_band():
    """A second build with a narrower window and the same stored extent (W = 300,
    then 257: both 768 columns) leaves nothing of the first behind."""
    blocks, _ = panel(130, 0.03)
    T = triangle(130, 0.03)
    eng = Engine(SIZES, K=1)
    try:
        stage(eng, blocks)
        for b in range(len(SIZES)):
            eng.geno_ld_band(0, b, 300)
        for b in range(len(SIZES)):
            eng.geno_ld_band(0, b, 257)
        for b in range(len(SIZES)):
            np.testing.assert_array_equal(eng.get_ld_block(0, b), masked(T[b], 257))
    finally:
        eng.close()


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("W", WINDOWS)
def test_layout_equals_csr_route(W, bits):
    """The block is indistinguishable from the same matrix uploaded as CSR: format,
    stored bytes, contents and the products of 1, 4 and 16 columns, bit for bit.
    Format 2 at n = 700 (W <= 256) and 1,500, format 1 at n = 130 and 257."""
    N, miss = 130, 0.03
    eng = build_bands(N, miss, W, bits)
    ref = Engine(SIZES, K=1)
    try:
        ref.set_ld_precision(bits)
        got = [eng.get_ld_block(0, b) for b in range(len(SIZES))]
        for b, n in enumerate(SIZES):
            ref.set_ld_block_csr(0, b, band_csr(got[b], win(W, n)))
        fmts = [eng.ld_block_format(0, b) for b in range(len(SIZES))]
        assert fmts == [ref.ld_block_format(0, b) for b in range(len(SIZES))]
        assert fmts == [band_format(n, win(W, n)) for n in SIZES]
        assert fmts[:2] == [1, 1] and fmts[3] == (2 if W != "n-1" else 1)
        assert [eng.ld_block_precision(0, b) for b in range(len(SIZES))] == [bits] * len(SIZES)
        assert eng.stored_bytes(0) == ref.stored_bytes(0)
        for b in range(len(SIZES)):
            np.testing.assert_array_equal(ref.get_ld_block(0, b), got[b])
        for ncol in (1, 4, 16):
            V = np.random.RandomState(ncol).normal(size=(ncol, sum(SIZES)))
            np.testing.assert_array_equal(eng.ld_matvec(0, V), ref.ld_matvec(0, V))
    finally:
        eng.close()
        ref.close()


@pytest.mark.parametrize("N,miss", [(130, 0.03), (1027, 0.0)])
@pytest.mark.parametrize("W", [1, 64, 255, 300, "n-1"])
def test_f32_band_rounds_on_store(W, N, miss):
    """The f32 engine's stored band is float32(round) of the f64 engine's, bit for bit."""
    got = {}
    for bits in (64, 32):
        eng = build_bands(N, miss, W, bits)
        try:
            assert [eng.ld_block_precision(0, b) for b in range(len(SIZES))] == [bits] * len(SIZES)
            got[bits] = [eng.get_ld_block(0, b) for b in range(len(SIZES))]
        finally:
            eng.close()
    for b in range(len(SIZES)):
        assert not np.array_equal(got[64][b], f32(got[64][b]))
        np.testing.assert_array_equal(got[32][b], f32(got[64][b]))


# ---- band pieces and their couplings -----------------------------------------
CUT_N, CUT_W, CUT_NS, CUT_PIECES = 2500, 200, 500, [1024, 1476]
# Truncating this panel's R (rank <= 500) to the window leaves eigenvalues down to
# -0.298 (numpy.linalg.eigvalsh of the masked bed_ref.R): R_s = (1 - s) R + s I is
# positive definite from s > 0.298 / 1.298 = 0.23, so the solves below use 0.3
CUT_S = "0.3"


@functools.lru_cache(maxsize=None)
def cut_codes():
    codes = bed_ref.draw_codes(CUT_N, CUT_NS, miss=0.03, seed=31)
    codes.setflags(write=False)
    return codes


@pytest.fixture(scope="module")
def cut_prefix(tmp_path_factory):
    codes = cut_codes()
    return write_bed(str(tmp_path_factory.mktemp("cut") / "p"), codes,
                     *bed_ref.bim_fam(CUT_N, CUT_NS))


def coupling_by_unit_vectors(eng, rows, cols, M=CUT_N):
    """out[a][c] = (R e_{cols[c]})[rows[a]]: products with 1.0 and zeros, exact."""
    out = np.empty((len(rows), len(cols)))
    for c0 in range(0, len(cols), 16):
        cc = cols[c0:c0 + 16]
        V = np.zeros((len(cc), M))
        V[np.arange(len(cc)), cc] = 1.0
        out[:, c0:c0 + len(cc)] = eng.ld_matvec(0, V)[:, rows].T
    return out


@pytest.mark.parametrize("bits", [64, 32])
def test_pieces_and_coupling_are_the_uncut_band(cut_prefix, bits):
    L = BedLD(read_bed(cut_prefix), [CUT_N], window=CUT_W)
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
        if bits == 32:
            np.testing.assert_array_equal(R, f32(R))
        assert maxrel(R, masked(bed_ref.R(cut_codes()), CUT_W)) < (TOL if bits == 64 else TOL + 2.0 ** -24)
        np.testing.assert_array_equal(cut.get_ld_block(0, 0), R[:1024, :1024])
        np.testing.assert_array_equal(cut.get_ld_block(0, 1), R[1024:, 1024:])
        # C, both ways round: the head's unit vectors give C's columns in the tail's
        # rows, the tail's unit vectors give C's rows in the head's
        tail, head = np.arange(824, 1024), np.arange(1024, 1224)
        C = R[824:1024, 1024:1224]
        assert np.count_nonzero(C) > 200 * 199 // 2 - 200          # the whole corner, not a part
        np.testing.assert_array_equal(coupling_by_unit_vectors(cut, tail, head), C)
        np.testing.assert_array_equal(coupling_by_unit_vectors(cut, head, tail), C.T)
        # and nothing but C couples the pieces
        V = np.zeros((2, CUT_N))
        V[0, :824], V[1, 1224:] = 1.0, 1.0
        Y = cut.ld_matvec(0, V)
        assert not Y[0, 1024:].any() and not Y[1, :1024].any()
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


# ---- the corner: a marker window is a count of kept columns per row ----------------
CORNER_PIECES, CORNER_NR, CORNER_NC = [200, 150], 130, 70


@functools.lru_cache(maxsize=None)
def corner_case(N):
    """The 350 markers' codes and their uncut f64 geno_ld block, computed once."""
    M = sum(CORNER_PIECES)
    codes = bed_ref.draw_codes(M, N, miss=0.03, seed=4100 + N)
    assert not bed_ref.unusable(codes).any()
    eng = Engine([M], K=1)
    try:
        eng.geno_set_block(0, bed_ref.pack(codes), N)
        eng.geno_ld(0, 0)
        T = eng.get_ld_block(0, 0)
    finally:
        eng.close()
    codes.setflags(write=False)
    T.setflags(write=False)
    return codes, T


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("N", [5, 130])
def test_window_corner_is_the_keep_corner(N, bits):
    """geno_coupling(W) == geno_coupling_reach(keep[a] = clip(W - nr + a + 1, 0, nc)),
    bit for bit, at nr = 130, nc = 70 (three row tiles, two column tiles, nr != nc):
    W = 1 keeps one entry (rows above it keep 0), W = 150 keeps all nc columns from
    row 49 on.  Both are the uncut block's corner where c + nr - a <= W (rounded
    once through f32 for 32 bits) and exactly 0.0 elsewhere."""
    nr, nc, (n0, n1) = CORNER_NR, CORNER_NC, CORNER_PIECES
    codes, T = corner_case(N)
    corner = T[n0 - nr:n0, n0:n0 + nc]
    if bits == 32:
        corner = f32(corner)
    rows = bed_ref.pack(codes[n0 - nr:n0 + nc])
    tail, head = np.arange(n0 - nr, n0), np.arange(n0, n0 + nc)
    a, c = np.arange(nr)[:, None], np.arange(nc)[None, :]
    A, B = Engine(CORNER_PIECES, K=1), Engine(CORNER_PIECES, K=1)
    try:
        for eng in (A, B):
            eng.set_ld_precision(bits)
            stage(eng, [codes[:n0], codes[n0:]])
            for b in range(2):
                eng.geno_ld(0, b)
        for W in (1, 64, 150):
            keep = np.clip(W - nr + np.arange(nr) + 1, 0, nc)
            A.geno_coupling(0, 0, nr, nc, rows, N, W)
            B.geno_coupling_reach(0, 0, nr, nc, rows, N, keep)
            CA = coupling_by_unit_vectors(A, tail, head, n0 + n1)
            CB = coupling_by_unit_vectors(B, tail, head, n0 + n1)
            inside = c + nr - a <= W
            assert inside.sum() == keep.sum()
            assert (keep[-2], keep[-1], keep[48], keep[49]) == \
                {1: (0, 1, 0, 0), 64: (63, 64, 0, 0), 150: (nc, nc, nc - 1, nc)}[W]
            np.testing.assert_array_equal(CA, CB)
            for C in (CA, CB):
                np.testing.assert_array_equal(C, np.where(inside, corner, 0.0))
                assert not C[~inside].any()
    finally:
        A.close()
        B.close()


# ---- refusals ------------------------------------------------------------------
def test_refusals(tmp_path):
    N = 130
    blocks, _ = panel(N, 0.03)
    bad = np.array(blocks[1])
    bad[17] = 3                      # homozygous A2 everywhere
    eng = Engine(SIZES[:2], K=1)
    try:
        eng.geno_set_block(0, bed_ref.pack(blocks[0]), N)
        eng.geno_set_block(1, bed_ref.pack(bad), N)
        for w in (0, -5):
            with pytest.raises(hb.HipError, match=r"\(-2\).*window"):
                eng.geno_ld_band(0, 0, w)
        with pytest.raises(hb.HipError, match=r"\(-4\).*1 marker\(s\) without LD"):
            eng.geno_ld_band(0, 1, 10)
        assert [eng.ld_block_format(0, b) for b in range(2)] == [-1, -1]
        eng.set_ld_packing(False)
        with pytest.raises(hb.HipError, match=r"\(-4\).*packing is off"):
            eng.geno_ld_band(0, 0, 10)
        assert eng.ld_block_format(0, 0) == -1
        eng.set_ld_packing(True)
        eng.geno_ld_band(0, 0, 10)
        assert [eng.ld_block_format(0, b) for b in range(2)] == [1, -1]
        with pytest.raises(hb.HipError, match=r"\(-2\).*window"):
            eng.geno_coupling(0, 0, 4, 4, bed_ref.pack(blocks[0][:8]), N, 0)
        with pytest.raises(hb.HipError, match=r"\(-2\)"):
            eng.geno_coupling(0, 1, 4, 4, bed_ref.pack(blocks[0][:8]), N, 5)   # no piece 2
        eng.geno_clear()
        with pytest.raises(hb.HipError, match=r"\(-4\).*no genotypes"):
            eng.geno_ld_band(0, 0, 10)
    finally:
        eng.close()
    # through BedLD: the marker is named, in a block and in a halo, and nothing is stored
    codes = np.concatenate([blocks[0], bad])
    prefix = write_bed(str(tmp_path / "p"), codes, *bed_ref.bim_fam(codes.shape[0], N))
    L = BedLD(read_bed(prefix), SIZES[:2], window=10)
    eng = Engine(SIZES[:2], K=1)
    try:
        L.upload(eng, 0, 0)
        with pytest.raises(ValueError, match=r"1 marker\(s\) of LD block 1 have no LD.*rs147"):
            L.upload(eng, 0, 1)
        assert [eng.ld_block_format(0, b) for b in range(2)] == [1, -1]
        eng.set_ld_packing(False)
        with pytest.raises(ValueError, match="needs LD packing on"):
            L.upload(eng, 0, 0, packed=False)
    finally:
        eng.close()
    one = BedLD(read_bed(prefix), [sum(SIZES[:2])], window=10)
    P, cps = one.pieces([[140, 247]])         # rs147 is the 8th row of the head's halo
    eng = Engine([140, 247], K=1)
    try:
        P.upload(eng, 0, 0)
        with pytest.raises(ValueError, match=r"1 marker\(s\) of the coupling between LD band "
                                             r"pieces 0 and 1 have no LD.*rs147"):
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


def test_one_rank_vs_two_ranks_bitwise():
    """tests/test_gpu_multirank.py's harness (ranks on one device, host exchange):
    the 2,500-marker panel at W = 200 in pieces [1024, 1476], one piece per rank,
    the coupling spanning the two: the stored pieces and the 5-iteration xhat / r1
    files equal one rank's, bit for bit (tools/geno_band_ranks_gpu.py)."""
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2",
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), SGV_EXCHANGE="host",
                   SGV_BAND_PIECE="1024")
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(ROOT, "tools", "geno_band_ranks_gpu.py")], env=env,
            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
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
@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("piece", [None, 1024])
def test_cli_window_equals_npz_of_the_band(tmp_path, cut_prefix, monkeypatch, piece, precision):
    """main.py --ld-window 200 on the .bed (K = 2 cohorts sharing it, one block of
    2,500, 5 iterations) against main.py on an .npz CSR of the uncut band fetched
    with get_ld_block, every in-band position explicit, under the same band piece:
    every output file byte-identical."""
    import main
    import sgvamp

    if piece is not None:
        monkeypatch.setattr(sgvamp, "BAND_PIECE", piece)
    codes = cut_codes()
    rs = np.random.RandomState(5)
    beta = np.zeros(CUT_N)
    beta[rs.choice(CUT_N, 100, replace=False)] = rs.normal(0, np.sqrt(0.8 / 100), 100)
    y = bed_ref.g(codes, beta) + rs.normal(0, np.sqrt(0.2), CUT_NS)
    np.save(tmp_path / "r.npy", bed_ref.r(codes, y).reshape(-1, 1))
    np.save(tmp_path / "beta.npy", beta.reshape(-1, 1))

    seen = []

    def run(ld, out, extra):
        (tmp_path / out).mkdir()
        main.main(["--ld-files", "%s,%s" % (ld, ld), "--r-files",
                   "%s,%s" % (tmp_path / "r.npy", tmp_path / "r.npy"),
                   "--true-signal-file", str(tmp_path / "beta.npy"), "--out-dir",
                   str(tmp_path / out), "--out-name", "run", "--N", "%d,%d" % (CUT_NS, CUT_NS),
                   "--M", "%d,%d" % (CUT_N, CUT_N), "--K", "2", "--iterations", "5", "--seed", "11",
                   "--prior-probs", "0.9,0.1", "--s", CUT_S, "--ld-precision", precision] + extra)
        return {fn: open(tmp_path / out / fn, "rb").read()
                for fn in sorted(os.listdir(tmp_path / out))}

    real = Engine.__init__

    def spy(self, block_sizes, *a, **kw):
        seen.append(list(block_sizes))
        real(self, block_sizes, *a, **kw)

    monkeypatch.setattr(Engine, "__init__", spy)
    a = run(cut_prefix + ".bed", "bed", ["--ld-block-size", str(CUT_N), "--ld-window", str(CUT_W)])
    monkeypatch.setattr(Engine, "__init__", real)
    assert seen == [CUT_PIECES if piece else [CUT_N]]
    L = BedLD(read_bed(cut_prefix), [CUT_N], window=CUT_W)
    eng = Engine([CUT_N], K=1)
    try:
        eng.set_ld_precision(32 if precision == "f32" else 64)
        L.upload(eng, 0, 0)
        R = eng.get_ld_block(0, 0)
    finally:
        eng.close()
    A = band_csr(R, CUT_W, full=True)
    assert A.nnz == CUT_N + 2 * sum(min(CUT_W, CUT_N - 1 - i) for i in range(CUT_N))
    scipy.sparse.save_npz(tmp_path / "R.npz", A)
    b = run(str(tmp_path / "R.npz"), "npz", [])
    assert a.keys() == b.keys()
    assert sum(fn.endswith(".bin") for fn in a) == 5 * 3 and "run_metrics.csv" in a
    for fn in a:
        assert a[fn] == b[fn], fn
    x = np.frombuffer(a["run_xhat_it_4.bin"])
    assert np.isfinite(x).all() and x.any()
