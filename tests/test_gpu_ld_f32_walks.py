"""Float instances of the band walks (band_walk.h, band_walk_f32.hip) on an f32-stored windowed
LD matrix (sgv_set_ld_precision 32).

What ships (profiles/ld_f32_walk/ldpass_band_ab.jsonl): on one
MI355X the float walks took 1.26-1.33x the time of the 512-column strips at
3, 4, 5 and 8 columns (M = 1e6, bw = 1,000 and 500), so by the ship rule neither
column group moved: an f32 band matrix runs every column count on the strips,
bit for bit as before, and the walks are the opt-in arm SGV_AB=1 SGV_F32_WALK=1
(3-8 columns, whatever set_mfma_min says).  DEFAULT_WALK_NCOLS, the column
counts an f32 matrix walks by default, is therefore empty; the tests hold the
float instances under the switch (the bitwise pin at WALK_NCOLS, scipy and the
invariance at every walked count, ALL_WALK_NCOLS; each gate checks through
sgv_timers t[5] that its engine did walk), and the default at "nothing moved".

Only the fragment loads differ from the f64 walks: the 8-B form (SGV_F32_FORM=1)
loads the same sub-tiles in the same order and widens them exactly, so it is
pinned bit for bit against the f64 walks on the widened blocks W(B) =
B.astype(float32).astype(float64); the 16-B form (the arm's default) adds a
row's terms in another fixed order and is held to the project's 1e-12 bar
against scipy on W(B).

Shapes: band-only engines holding xl.walk_sizes(bw) for bw in xl.WALK_BWS (R =
2..5 ring slots; blocks shorter than a walk, of exactly W, W + 1 and 2 W + 2
panels, ragged, half and whole last panels).

Measured on an MI355X: worst column against scipy 1.9e-15 (bw = 1,000); end to
end against the oracle on the widened matrix 1.9e-13 (K = 4, EM) and 1.0e-11
(K = 2, MLE), all counts equal.  The whole file takes 14 s.
"""
import contextlib
import os

import numpy as np
import pytest

from engine import Engine
from oracle import vamp_oracle as vo
from sgvamp import VAMP, BlockLD
from tests import exact_ld as xl
from tests.test_gpu_pass_exact import (ALL, assert_form, call, data, epilogue_gate, expect, kinds,
                                       nan_cols, nan_gate, two_matrix_engine, upload, OUT_FILL,
                                       YOUT_FILL)
from tests.test_gpu_pass_exact import environ as pass_environ

pytestmark = pytest.mark.gpu

DEFAULT_WALK_NCOLS = []              # what ships: no f32 pass walks by default
WALK_NCOLS = [3, 4, 5, 6, 8]         # the column counts of the opt-in arm's bitwise pin
ALL_WALK_NCOLS = list(range(3, 9))   # every column count the arm walks: scipy, invariance
SHIPPED_FORM = "2"                   # the arm's load form
STRIP_NCOLS = [1, 2, 9, 16]          # f32 passes the arm leaves on the strips
SWITCH = "SGV_F32_WALK"
WALK = {SWITCH: "1"}                 # the arm: an f32 band matrix on the walks
NOWALK = {"SGV_BAND_WALK": "0"}
FORM1 = dict(WALK, SGV_F32_FORM="1")


@contextlib.contextmanager
def environ(env):
    """test_gpu_pass_exact's environ, which also clears the f32 walks' switch."""
    old = os.environ.pop(SWITCH, None)
    try:
        with pass_environ(env):
            yield
    finally:
        os.environ.pop(SWITCH, None)
        if old is not None:
            os.environ[SWITCH] = old


def assert_walks(eng, ld, M, ncol=4):
    """An ncol-column pass of LD matrix ld takes the walks: its partial traffic
    (sgv_timers t[5]) is not what the same pass moves on the strips
    (SGV_BAND_WALK=0, read per pass) -- the evidence, independent of the report,
    that the form Engine.ld_pass_form reports beside it is the one that ran.
    Called under SGV_AB=1."""
    def aux():
        eng.timers(reset=True)
        eng.ld_matvec(ld, np.zeros((ncol, M)))
        return eng.timers()["aux_bytes"]

    assert os.environ.get("SGV_AB") == "1" and "SGV_BAND_WALK" not in os.environ
    assert eng.ld_pass_form(ld, ncol).kind == "walk", (ld, ncol, eng.ld_pass_form(ld, ncol))
    walked = aux()
    os.environ["SGV_BAND_WALK"] = "0"
    try:
        assert eng.ld_pass_form(ld, ncol).kind in ("strip4", "pair"), eng.ld_pass_form(ld, ncol)
        strips = aux()
    finally:
        del os.environ["SGV_BAND_WALK"]
    assert walked != strips, (ld, ncol, walked, strips)
    assert eng.ld_pass_form(ld, ncol).kind == "walk"
    assert aux() == walked


def maxrel(a, b):
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


def W(x):
    """x rounded to the nearest f32 and widened back: what an f32 block stores."""
    return x.astype(np.float32).astype(np.float64)


class GBand:
    """Exactly symmetric band block with general f64 entries (~ N(0, 1 / bw), so
    rounding to f32 really happens), kept as the CSR of its upper triangle."""

    def __init__(self, n, bw, seed):
        bw = int(min(bw, n - 1))
        lens = np.minimum(bw + 1, n - np.arange(n))
        self.shape = (n, n)
        self.indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        within = np.arange(int(lens.sum())) - np.repeat(self.indptr[:-1], lens)
        self.indices = (np.repeat(np.arange(n), lens) + within).astype(np.int64)
        self.data = np.random.RandomState([seed, n, bw]).standard_normal(int(lens.sum())) / np.sqrt(bw)

    def widened(self):
        g = object.__new__(GBand)
        g.shape, g.indptr, g.indices, g.data = self.shape, self.indptr, self.indices, W(self.data)
        return g

    def matmul(self, V):
        """(R V^T)^T for V [ncol][n] in f64 (scipy CSR products)."""
        import scipy.sparse

        up = scipy.sparse.csr_matrix((self.data, self.indices, self.indptr), shape=self.shape)
        return (up @ V.T + up.T @ V.T).T - up.diagonal() * V


_blocks, _rhs, _runs = {}, {}, {}


def gblocks(bw):
    if bw not in _blocks:
        _blocks[bw] = [GBand(n, bw, 17) for n in xl.walk_sizes(bw)]
    return _blocks[bw]


def rhs(M, ncol):
    if M not in _rhs:
        _rhs[M] = np.random.RandomState(M % 9973).normal(size=(16, M))
    return _rhs[M][:ncol]


def run(blocks, ncols, bits=32, env=None, widen=False, mfma_min=None, key=None):
    """{ncol: ([Y, Y again], aux_bytes of the second pass, the form reported
    before the first)} on a fresh band-only
    engine holding `blocks` (widen: their widened copies) at `bits`; cached
    under key."""
    if key is not None and key in _runs:
        return _runs[key]
    sizes = [B.shape[0] for B in blocks]
    out = {}
    with environ(env):
        eng = Engine(sizes, K=1)
        eng.set_ld_precision(bits)
        if mfma_min is not None:
            eng.set_mfma_min(mfma_min)
        for b, B in enumerate(blocks):
            eng.set_ld_block_csr(0, b, B.widened() if widen else B)
            assert eng.ld_block_format(0, b) == 2 and eng.ld_block_precision(0, b) == bits
        for ncol in ncols:
            V = rhs(sum(sizes), ncol)
            form = eng.ld_pass_form(0, ncol)
            Y = [np.array(eng.ld_matvec(0, V))]
            eng.timers(reset=True)
            Y.append(np.array(eng.ld_matvec(0, V)))
            out[ncol] = (Y, eng.timers()["aux_bytes"], form)
        eng.close()
    if key is not None:
        _runs[key] = out
    return out


def walked_f32(bw):
    """The arm at its default form, every column count (cached)."""
    return run(gblocks(bw), ALL_WALK_NCOLS + STRIP_NCOLS, env=WALK, key=("f32 walks", bw))


# 1 -------------------------------------------------------------------------
@pytest.mark.parametrize("bw", [300, 1000])
def test_f32_walk_selection(bw):
    """The partial traffic of one pass (sgv_timers t[5]) names the kernel.  Under
    SGV_F32_WALK=1, at 3, 4, 5 and 8 columns, the f32 engine's equals the f64
    engine's (the walks' head and carry buffers, f64 for both) and not the
    strips'; with SGV_BAND_WALK=0 as well it is the strips'.  Its 1-2- and
    9-16-column passes did not move (bitwise the SGV_BAND_WALK=0 products), and
    set_mfma_min(0) changes neither the products nor the traffic.  Without the
    switch (what ships) no f32 pass moved: every column count has the strips'
    traffic and, bit for bit, the SGV_BAND_WALK=0 products."""
    B = gblocks(bw)
    nc = [3, 4, 5, 8]
    f32 = walked_f32(bw)
    f32_strips = run(B, nc + STRIP_NCOLS, env=dict(WALK, **NOWALK))
    f64 = run(B, nc, bits=64)
    f64_strips = run(B, nc, bits=64, env=NOWALK)
    f32_valu = run(B, nc, env=WALK, mfma_min=0)
    shipped = run(B, nc + STRIP_NCOLS)
    for n in nc:
        print("bw=%d ncol=%d aux bytes: f32 walks %.0f f64 %.0f strips %.0f shipped f32 %.0f" % (
            bw, n, f32[n][1], f64[n][1], f64_strips[n][1], shipped[n][1]))
        # the reported forms (bw = 300 and 1,000: the band's strips are ragged)
        assert (f32[n][2].kind, f32[n][2].load_form) == ("walk", int(SHIPPED_FORM)), f32[n][2]
        assert (f64[n][2].kind, f64[n][2].load_form) == ("walk", 1), f64[n][2]
        assert (f32_valu[n][2].kind, f32_valu[n][2].load_form) == ("walk", int(SHIPPED_FORM))
        assert f32_strips[n][2].kind == f64_strips[n][2].kind == shipped[n][2].kind == "strip4", n
        assert (f32_strips[n][2].fin_form, f64_strips[n][2].fin_form) == (1, 1), n
        # and the traffic that bears them out
        assert f32[n][1] == f64[n][1], n
        assert f32[n][1] != f64_strips[n][1], n
        assert f32_strips[n][1] == f64_strips[n][1], n
        assert f32_valu[n][1] == f32[n][1], n
        np.testing.assert_array_equal(f32_valu[n][0][0], f32[n][0][0])
        assert not np.array_equal(f32[n][0][0], f32_strips[n][0][0])
    for n in STRIP_NCOLS:
        for r in (f32, f32_strips, shipped):
            assert r[n][2].kind == ("strip4" if n <= 8 else "strip16"), (n, r[n][2])
        np.testing.assert_array_equal(f32[n][0][0], f32_strips[n][0][0])
    for n in nc + STRIP_NCOLS:
        if n in DEFAULT_WALK_NCOLS:
            assert shipped[n][1] == f32[n][1], n
            np.testing.assert_array_equal(shipped[n][0][0], f32[n][0][0])
        else:
            assert shipped[n][1] == f32_strips[n][1], n
            np.testing.assert_array_equal(shipped[n][0][0], f32_strips[n][0][0])


# 2 -------------------------------------------------------------------------
@pytest.mark.parametrize("bw", xl.WALK_BWS)
def test_f32_walk_8B_form_bitwise_the_f64_walks_on_widened_blocks(bw):
    """The 8-B form gives every chain the operands, in the order, the f64 walks
    see on the widened blocks: bitwise equal products.  The arm's default form
    is the 16-B one, forced."""
    B = gblocks(bw)
    form1 = run(B, WALK_NCOLS, env=FORM1)
    pin = run(B, WALK_NCOLS, bits=64, widen=True)
    forced = run(B, WALK_NCOLS, env=dict(WALK, SGV_F32_FORM=SHIPPED_FORM))
    dflt = walked_f32(bw)
    assert not np.array_equal(W(B[0].data), B[0].data)          # the rounding is real
    for n in WALK_NCOLS:
        assert [(r[n][2].kind, r[n][2].load_form) for r in (form1, pin, forced, dflt)] == [
            ("walk", 1), ("walk", 1), ("walk", int(SHIPPED_FORM)), ("walk", int(SHIPPED_FORM))], n
        np.testing.assert_array_equal(form1[n][0][0], pin[n][0][0])
        np.testing.assert_array_equal(dflt[n][0][0], forced[n][0][0])
        assert not np.array_equal(dflt[n][0][0], form1[n][0][0])    # another summation order


# 3 -------------------------------------------------------------------------
@pytest.mark.parametrize("bw", xl.WALK_BWS)
def test_f32_walks_vs_numpy_and_repeatable(bw):
    """The default form within 1e-12 relative of scipy on the widened blocks,
    every column at 3-8 columns; two passes bitwise equal."""
    B = gblocks(bw)
    got = walked_f32(bw)
    M = sum(b.shape[0] for b in B)
    ref, o = np.empty((max(ALL_WALK_NCOLS), M)), 0
    for b in B:
        n = b.shape[0]
        ref[:, o:o + n] = b.widened().matmul(rhs(M, max(ALL_WALK_NCOLS))[:, o:o + n])
        o += n
    worst = 0.0
    for n in ALL_WALK_NCOLS:
        worst = max([worst] + [maxrel(got[n][0][0][j], ref[j]) for j in range(n)])
        np.testing.assert_array_equal(got[n][0][0], got[n][0][1])
    print("bw=%d: worst column vs scipy on the widened blocks %.3e" % (bw, worst))
    assert worst < 1e-12, worst


@pytest.mark.parametrize("bw", xl.WALK_BWS)
def test_f32_walk_sums_are_a_function_of_the_block_alone(bw):
    """A block's sums are bitwise the same alone and between other band blocks,
    in either order, at 3-8 columns (what keeps 1 = N ranks bitwise).  The block has W + 1
    panels: a whole walk, then a trailing one with head panels and carries."""
    B = gblocks(bw)
    Wp = max(4, 2 * (xl.ring_slots(bw) - 1))
    mid = next(b for b in B if -(-b.shape[0] // 256) == Wp + 1)
    n = mid.shape[0]
    V = rhs(n, max(ALL_WALK_NCOLS))

    def sums(blocks):
        o = sum(b.shape[0] for b in blocks[:blocks.index(mid)])
        sizes = [b.shape[0] for b in blocks]
        eng = Engine(sizes, K=1)
        eng.set_ld_precision(32)
        for i, b in enumerate(blocks):
            eng.set_ld_block_csr(0, i, b)
        out = {}
        for nc in ALL_WALK_NCOLS:
            X = np.array(rhs(sum(sizes), nc))
            X[:, o:o + n] = V[:nc]
            out[nc] = np.array(eng.ld_matvec(0, X))[:, o:o + n]
        assert_walks(eng, 0, sum(sizes))
        eng.close()
        return out

    with environ(WALK):
        alone = sums([mid])
        for blocks in ([B[0], mid, B[-1]], [B[-1], mid, B[0]]):
            got = sums(blocks)
            for nc in ALL_WALK_NCOLS:
                np.testing.assert_array_equal(got[nc], alone[nc])


# 4 -------------------------------------------------------------------------
@pytest.mark.parametrize("bw", xl.WALK_BWS)
def test_f32_walk_forms_exact(bw):
    """(a) The 8-B form on band-only f32 engines against the exact reference
    and the 16-B form beside it (test_band_forms_exact[f32-*] holds what ships:
    the strips)."""
    dn, dw = data(("walk", bw), "narrow"), data(("walk", bw), "wide")
    for tag, env, lf in (("f32_8B", FORM1, 1), ("f32_16B", WALK, 2)):
        with environ(env):
            eng = two_matrix_engine(dn, dw, lambda e: e.set_ld_precision(32), 2, 32)
            # 1-2 columns on the strips, 3-8 on the walks, 9-16 on the 16x16x4 strips
            epilogue_gate(eng, dn, dw, ALL, (tag, bw), kinds("strip4", "walk", load_form=lf))
            nan_gate(eng, dn, nan_cols(ALL), (tag, bw))
            for ld in (0, 1):
                assert_walks(eng, ld, dn.M)
            eng.close()


def test_f32_coupled_pieces_exact():
    """(b) The xl.COUPLED band stored at 32 bits and cut into coupled pieces, on
    the walks: their and k_walk_fin's epilogues with coupling sums."""
    from sgvamp import band_cuts

    ncols = [1, 2, 3, 4, 5, 6, 7, 8, 16]
    dn, dw = data("coupled", "narrow"), data("coupled", "wide")
    with environ(WALK):
        eng = sizes = None
        for ld, d in ((0, dn), (1, dw)):
            L = BlockLD.from_csr(d.blocks[0].scipy_csr(), block_sizes=[d.M])
            cuts = band_cuts([L], L.block_sizes, piece=xl.COUPLED["piece"])
            P, cpl = L.pieces(cuts)
            assert len(P.block_sizes) == 4 and P.block_sizes[-1] % 256 != 0, P.block_sizes
            if eng is None:
                sizes = P.block_sizes
                eng = Engine(sizes, K=2, ld_of=[0, 1])
                eng.set_ld_precision(32)
            assert P.block_sizes == sizes and sorted(cpl) == [0, 1, 2]
            for b in range(len(sizes)):
                P.upload(eng, ld, b)
                assert eng.ld_block_format(ld, b) == 2 and eng.ld_block_precision(ld, b) == 32
            for gb, (nr, nc, C) in cpl.items():
                eng.set_ld_coupling(ld, gb, nr, nc, C)
        epilogue_gate(eng, dn, dw, ncols, "f32 coupled", kinds("strip4", "walk", load_form=2))
        nan_gate(eng, dn, nan_cols(ncols), "f32 coupled")
        for ld in (0, 1):
            assert_walks(eng, ld, dn.M)
        eng.close()


def test_history_independence_across_element_types():
    """(c) The hist_band blocks twice in one engine, as an f64 and as an f32
    band matrix, both on the walks (shared head / carry buffers and Pk layouts): a fixed
    pseudo-random sequence of passes, every column count, mask and run value,
    every result the exact reference."""
    band = data("hist_band", "narrow")
    with environ(WALK):
        eng = Engine(xl.HIST_SIZES, K=2, ld_of=[0, 1])
        upload(eng, 0, band)
        eng.set_ld_precision(32)
        upload(eng, 1, band)
        for b in range(len(xl.HIST_SIZES)):
            assert [eng.ld_block_format(ld, b) for ld in range(2)] == [2, 2]
            assert [eng.ld_block_precision(ld, b) for ld in range(2)] == [64, 32]
        rs = np.random.RandomState(2025)
        cells = list(rs.permutation(32)) + list(rs.randint(32, size=16))
        for step, cell in enumerate(cells):
            ld, ncol = int(cell) // 16, int(cell) % 16 + 1
            full = (1 << ncol) - 1
            dm, ym = int(rs.randint(1 << 16)) & full, int(rs.randint(1 << 16)) & full
            run_ = int(rs.choice([-1, -1, 1, 0]))
            w = "alias" if rs.randint(2) else band.W[:ncol]
            c1, c2 = xl.narrow_coeffs(ncol)
            assert_form(eng, ld, ncol, (kinds("valu", "walk", load_form=1),
                                        kinds("strip4", "walk", load_form=2))[ld], ("history", step))
            got = call(eng, ld, band, ncol, c1, c2, w if dm else None, dm, ym, run=run_)
            tag = ("history", step, ld, ncol, hex(dm), hex(ym), run_)
            if run_ == 0:
                np.testing.assert_array_equal(got[0], np.full_like(got[0], OUT_FILL), err_msg=str(tag))
                np.testing.assert_array_equal(got[1], np.full_like(got[0], YOUT_FILL), err_msg=str(tag))
            else:
                expect(band, ncol, c1, c2, w if dm else None, dm, ym, tag, got)
        for ld in (0, 1):
            assert_walks(eng, ld, band.M)
        eng.close()


# 5 -------------------------------------------------------------------------
@pytest.mark.parametrize("K,s,damp,prior", [(4, 0.05, True, "em"), (2, 0.0, False, "mle")])
def test_vamp_f32_band_ld_vs_oracle(K, s, damp, prior, tmp_path):
    """test_vamp_band_ld_vs_oracle with ld_precision="f32" on the walks: whole VAMP iterations
    on one banded LD matrix of 8,000 markers, bw = 600, against the oracle on
    the same CSR with its values rounded to f32 and widened: xhat <= 1e-8
    relative, CG counts and EM steps exact, the band stored at 32 bits.  The
    passes carry 3-8 columns as cohorts stop: both column groups of the walks."""
    M, bw, N = 8000, 600, 5000
    A = vo.banded_ld(M, bw, seed=21)
    A.data = W(A.data)
    rs = np.random.RandomState(4)
    cm = M // 20
    beta = np.zeros(M)
    beta[rs.choice(M, cm, replace=False)] = rs.normal(0, np.sqrt(0.5 / cm), cm) * np.sqrt(N)
    r = [A @ beta + rs.normal(size=M) * np.sqrt(0.5) for _ in range(K)]
    Ns = [float(N)] * K
    Nt = sum(Ns)
    a = np.array(Ns) / Nt
    prior_vars, prior_probs = [0.0, 0.5 / cm], [0.95, 0.05]
    L = BlockLD.from_csr(A, s=s)
    its = 6
    with environ(WALK):
        v = VAMP(N=Ns, Nt=Nt, M=M, K=K, rho=0.5, gamw=2.0, gam1=1e-6, a=a, prior_vars=prior_vars,
                 prior_probs=prior_probs, out_dir=str(tmp_path), out_name="band", seed=9,
                 write_files=False, ld_precision="f32")
        xh = v.infer(L, np.stack(r), its, x0=beta, lmmse_damp=damp, prior_update=prior)
        assert v.engine.ld_block_format(0, 0) == 2 and v.engine.ld_block_precision(0, 0) == 32
        assert_walks(v.engine, 0, M)    # the run's band passes took the walks: one more says so
    t = vo.infer([vo.CsrLD(A, s=s)], [0] * K, r, Ns, its, rho=0.5, gamw=2.0, gam1=1e-6,
                 prior_vars=prior_vars, prior_probs=prior_probs, x0=beta, seed=9,
                 lmmse_damp=damp, reducer=vo.Reducer("blocked", bounds=np.array([0, M])),
                 rs_recurrence=True, prior_update=prior)
    worst = 0.0
    for it in range(its):
        worst = max(worst, maxrel(xh[it].ravel() / np.sqrt(Nt), np.asarray(t["xhat"][it]).ravel()))
    print("K=%d %s: xhat vs the oracle on the widened matrix %.3e" % (K, prior, worst))
    assert worst < 1e-8, worst
    assert [h["cg_iters"] for h in v.history] == [[list(c) for c in x] for x in t["cg_iters"]]
    if prior == "em":
        assert [h.get("em_steps") for h in v.history][1:] == list(t["em_steps"])
    v.engine.close()
