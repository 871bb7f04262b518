"""Opt-in f32 storage of packed LD blocks (sgv_set_ld_precision 32): R is
rounded once, on store, to the nearest f32; every product and sum stays f64.

The references are therefore exact-input ones: numpy on the WIDENED blocks
W(B) = B.astype(float32).astype(float64), held to the project's 1e-12 bar for
every LD kernel.  An f32 matrix runs the 16-B load form of the float strip
kernels (a float4 per lane feeding two 32-column steps; a row's terms added in
another fixed order).  The 8-B form (SGV_AB=1 SGV_F32_FORM=1) stays compiled:
it loads the same sub-tile in the same step order as the double kernels, so it
is pinned bit for bit against the f64 strip kernels run on the widened blocks.

Measured on an MI355X (worst column of every case): products vs numpy 2.4e-15,
band beside triangle 2.5e-15; end to end vs the reference's golden xhat 7.8e-7
(k4_shared_s_damp; the other cases <= 1.0e-7), vs the oracle on the widened
blocks 2.9e-13, all counts equal.  The whole file takes 2 s.
"""
import contextlib
import os

import numpy as np
import pytest

import hip_backend as hb
from engine import Engine
from oracle import vamp_oracle as vo
from sgvamp import VAMP, BlockLD
from tests.golden import Case

pytestmark = pytest.mark.gpu

RIDGE = 0.1
# 4700 = 19 panels: one column parity has 10, so its last chunk is cut into an
# 8 + 2-panel strip pair; the small blocks put the ragged chunk end on, past and
# before wave (128-column) boundaries
SIZES = [4700, 1281, 513, 257, 1]
# both 4x4x4 group counts, the 16x16x4 kernel, and 1-2 columns on the strips
NCOLS = [1, 2, 3, 4, 5, 8, 9, 16]
# the f64 arm of the pin: every column count on the f64 512-column strip kernels
F64_STRIPS = {"SGV_AB": "1", "SGV_MF_WIDE": "0", "SGV_MF_PAIR": "0", "SGV_BAND_WALK": "0"}
FORM1 = {"SGV_AB": "1", "SGV_F32_FORM": "1"}   # the f32 arm of the pin: 8-B loads
FORM2 = {"SGV_AB": "1", "SGV_F32_FORM": "2"}   # the default form, forced
AB_KEYS = ("SGV_AB", "SGV_MF_WIDE", "SGV_MF_PAIR", "SGV_BAND_WALK", "SGV_MF_WIDE_IDLE",
           "SGV_F32_FORM")


def maxrel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


def W(B):
    """B rounded to the nearest f32 (ties to even), widened back: what is stored."""
    return B.astype(np.float32).astype(np.float64)


_blocks = {}


def block(n):
    """Exactly symmetric random n x n block with general f64 entries (~ N(0, 1/n)),
    so that rounding to f32 really happens; one per size."""
    if n not in _blocks:
        A = np.random.RandomState(1000 + n).standard_normal((n, n)) / np.sqrt(n)
        U = np.triu(A)
        _blocks[n] = U + np.triu(A, 1).T
    return _blocks[n]


_vecs = {}


def vec(n, ncol):
    if (n, ncol) not in _vecs:
        _vecs[(n, ncol)] = np.random.RandomState(7 * n + ncol).normal(size=(ncol, n))
    return _vecs[(n, ncol)]


def rhs(sizes, ncol):
    return np.concatenate([vec(n, ncol) for n in sizes], axis=1)


@contextlib.contextmanager
def environ(env):
    old = {k: os.environ.get(k) for k in AB_KEYS}
    try:
        for k in AB_KEYS:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k in AB_KEYS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def assert_strips(eng, ncol, bits, env):
    """The next ncol-column pass reports what every arm of this file claims: the
    4-wave 512-column strips (the 16x16x4 ones above 8 columns) in the arm's load
    form -- an f32 matrix the 16-B form unless SGV_F32_FORM=1, an f64 one the 8-B."""
    form = eng.ld_pass_form(0, ncol)
    lf = 1 if bits == 64 or (env or {}).get("SGV_F32_FORM") == "1" else 2
    assert (form.kind, form.load_form) == ("strip4" if ncol <= 8 else "strip16", lf), (
        ncol, bits, env, form)


def products(sizes, ncols, bits=32, env=None, repeat=1, mfma_min=None, widen=False, checks=None):
    """{ncol: [Y, ...]}: `repeat` products per column count on a fresh engine
    holding block(n) (widen: W(block(n))) for n in sizes at `bits`; checks(eng)
    runs before the engine closes."""
    with environ(env or {}):
        eng = Engine(sizes, K=1)
        eng.set_ld_precision(bits)
        if mfma_min is not None:
            eng.set_mfma_min(mfma_min)
        for b, n in enumerate(sizes):
            eng.set_ld_block(0, b, W(block(n)) if widen else block(n))
        eng.set_ridge(RIDGE)
        out = {}
        for ncol in ncols:
            V = rhs(sizes, ncol)
            assert_strips(eng, ncol, bits, env)
            out[ncol] = [np.array(eng.ld_matvec(0, V)) for _ in range(repeat)]
        if checks:
            checks(eng)
        eng.close()
    return out


_main = {}


def main_products():
    """Two f32 products per column count on the SIZES engine (shared), with the
    engine's own report of what it stores."""
    if not _main:
        info = {}

        def checks(eng):
            info["prec"] = [eng.ld_block_precision(0, b) for b in range(len(SIZES))]
            info["fmt"] = [eng.ld_block_format(0, b) for b in range(len(SIZES))]
            info["bytes"] = eng.stored_bytes(0)

        _main["Y"] = products(SIZES, NCOLS, repeat=2, checks=checks)
        _main["info"] = info
    return _main


_ref = {}


def ref_ld():
    if not _ref:
        _ref["L"] = vo.BlockLD([W(block(n)) for n in SIZES], s=RIDGE)
    return _ref["L"]


# 1 -------------------------------------------------------------------------
@pytest.mark.parametrize("ncol", NCOLS)
def test_f32_products_vs_numpy(ncol):
    """Every column within 1e-12 relative of numpy on the widened blocks."""
    Y = main_products()["Y"][ncol][0]
    V = rhs(SIZES, ncol)
    for j in range(ncol):
        err = maxrel(Y[j], ref_ld().matvec_Rs(V[j]))
        print("ncol=%d column %d: maxrel %.3e" % (ncol, j, err))
        assert err < 1e-12, (ncol, j, err)


def test_f32_storage_report():
    """Packed triangles at 32 bits, half the f64 engine's stored bytes."""
    info = main_products()["info"]
    assert info["prec"] == [32] * len(SIZES)
    assert info["fmt"] == [1] * len(SIZES)
    eng = Engine(SIZES, K=1)
    assert eng.ld_block_precision(0, 0) == -1
    for b, n in enumerate(SIZES):
        eng.set_ld_block(0, b, block(n))
    assert [eng.ld_block_precision(0, b) for b in range(len(SIZES))] == [64] * len(SIZES)
    b64 = eng.stored_bytes(0)
    with pytest.raises(hb.HipError):
        eng.set_ld_precision(16)
    eng.close()
    print("stored bytes f64 %d f32 %d" % (b64, info["bytes"]))
    assert info["bytes"] * 2 == b64
    assert b64 == 8.0 * sum(min(256, n - r0) * (n - r0) for n in SIZES for r0 in range(0, n, 256))


# 2 -------------------------------------------------------------------------
class UpperCsr:
    """The upper triangle of a dense block as CSR arrays (Engine.set_ld_block_csr)."""

    def __init__(self, B, bw):
        n = B.shape[0]
        self.shape = B.shape
        cols = [np.arange(i, min(n, i + bw + 1)) for i in range(n)]
        self.indptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])])
        self.indices = np.concatenate(cols)
        self.data = np.concatenate([B[i, c] for i, c in enumerate(cols)])


def test_f32_round_trip():
    """get_ld_block returns exactly the stored values, symmetric: W(B), through
    the dense upload and through the CSR upload."""
    sizes = [1281, 257]
    eng = Engine(sizes, K=1)
    eng.set_ld_precision(32)
    for b, n in enumerate(sizes):
        eng.set_ld_block(0, b, block(n))
    for b, n in enumerate(sizes):
        np.testing.assert_array_equal(eng.get_ld_block(0, b), W(block(n)))
    for b, n in enumerate(sizes):
        eng.set_ld_block_csr(0, b, UpperCsr(block(n), n))
        assert eng.ld_block_precision(0, b) == 32 and eng.ld_block_format(0, b) == 1
    for b, n in enumerate(sizes):
        np.testing.assert_array_equal(eng.get_ld_block(0, b), W(block(n)))
    # a finite entry outside f32's range: refused, the block left unset
    big = block(257).copy()
    big[3, 5] = big[5, 3] = 1e39
    with pytest.raises(hb.HipError, match="f32"):
        eng.set_ld_block(0, 1, big)
    assert eng.ld_block_precision(0, 1) == -1
    eng.close()


# 3 -------------------------------------------------------------------------
def band_block(nb, bw):
    i = np.arange(nb)
    return np.where(np.abs(i[:, None] - i[None, :]) <= bw, block(nb), 0.0)


def band_products(bits, ncols, env=None, widen=False, mfma_min=None):
    nb, bw = 3000, 300
    band = band_block(nb, bw)
    out, info = {}, {}
    with environ(env or {}):
        eng = Engine([nb, 1281], K=1)
        eng.set_ld_precision(bits)
        if mfma_min is not None:
            eng.set_mfma_min(mfma_min)
        eng.set_ld_block_csr(0, 0, UpperCsr(W(band) if widen else band, bw))
        eng.set_ld_block(0, 1, W(block(1281)) if widen else block(1281))
        info["fmt"] = [eng.ld_block_format(0, b) for b in range(2)]
        info["prec"] = [eng.ld_block_precision(0, b) for b in range(2)]
        eng.set_ridge(RIDGE)
        for ncol in ncols:
            assert_strips(eng, ncol, bits, env)
            assert eng.ld_pass_form(0, ncol).fin_form == (1 if ncol <= 8 else 4)   # ragged strips
            out[ncol] = np.array(eng.ld_matvec(0, rhs([nb, 1281], ncol)))
        info["band"] = eng.get_ld_block(0, 0)
        eng.close()
    return out, info


def test_f32_band_beside_triangle():
    """A packed band and a triangle, both f32: the ragged strip items.  Within
    1e-12 of numpy on the widened matrices (default form and the 8-B form), the
    8-B form bitwise the f64 strip kernels' products on them."""
    ncols = [3, 8, 16]
    got, info = band_products(32, ncols)
    assert info["fmt"] == [2, 1] and info["prec"] == [32, 32]
    band = band_block(3000, 300)
    np.testing.assert_array_equal(info["band"], W(band))
    L = vo.BlockLD([W(band), W(block(1281))], s=RIDGE)
    for ncol in ncols:
        V = rhs([3000, 1281], ncol)
        for j in range(ncol):
            err = maxrel(got[ncol][j], L.matvec_Rs(V[j]))
            print("band ncol=%d column %d: maxrel %.3e" % (ncol, j, err))
            assert err < 1e-12, (ncol, j, err)
    form1, _ = band_products(32, ncols, env=FORM1)
    pin, pinfo = band_products(64, ncols, env=F64_STRIPS, widen=True, mfma_min=1)
    assert pinfo["fmt"] == [2, 1] and pinfo["prec"] == [64, 64]
    for ncol in ncols:
        np.testing.assert_array_equal(form1[ncol], pin[ncol])


# 4 -------------------------------------------------------------------------
def test_f32_function_of_block_alone_and_repeatable():
    """The 1281-marker block's f32 sums are bitwise the same whatever else the
    engine holds and wherever the block sits; two passes are bitwise equal."""
    ncols = [2, 4, 8, 16]
    alone = products([1281], ncols)
    for sizes in ([4700, 1281, 513], [513, 1281, 4700]):
        got = products(sizes, ncols)
        o = sum(sizes[:sizes.index(1281)])
        for ncol in ncols:
            np.testing.assert_array_equal(got[ncol][0][:, o:o + 1281], alone[ncol][0])
    for ncol in NCOLS:
        a, b = main_products()["Y"][ncol]
        np.testing.assert_array_equal(a, b)


# 5 -------------------------------------------------------------------------
def test_f32_ignores_mfma_min():
    """set_mfma_min(0) (f64: the VALU pass) does not move an f32 matrix off the
    strips: bitwise the default's products."""
    sizes = [1281, 513]
    default = products(sizes, [2, 8])
    valu = products(sizes, [2, 8], mfma_min=0)
    for ncol in (2, 8):
        np.testing.assert_array_equal(valu[ncol][0], default[ncol][0])


# 6 -------------------------------------------------------------------------
def test_mixed_precision_in_one_matrix_refused():
    """A 64-bit and a 32-bit packed block in one LD matrix: the first pass fails
    and names the matrix.  Two LD matrices of one engine may differ."""
    sizes = [513, 257]
    eng = Engine(sizes, K=2, ld_of=[0, 1])
    eng.set_ridge(RIDGE)
    eng.set_ld_precision(64)
    eng.set_ld_block(1, 0, block(513))
    eng.set_ld_precision(32)
    eng.set_ld_block(1, 1, block(257))
    eng.set_ld_block(0, 0, block(513))     # LD 0: all f32
    eng.set_ld_block(0, 1, block(257))
    V = rhs(sizes, 4)
    with pytest.raises(hb.HipError, match="LD matrix 1"):
        eng.ld_matvec(1, V)
    eng.set_ld_precision(64)               # LD 1: all f64
    eng.set_ld_block(1, 1, block(257))
    assert [eng.ld_block_precision(0, b) for b in range(2)] == [32, 32]
    assert [eng.ld_block_precision(1, b) for b in range(2)] == [64, 64]
    Y32 = np.array(eng.ld_matvec(0, V))
    Y64 = np.array(eng.ld_matvec(1, V))
    eng.close()
    L32 = vo.BlockLD([W(block(n)) for n in sizes], s=RIDGE)
    L64 = vo.BlockLD([block(n) for n in sizes], s=RIDGE)
    for j in range(4):
        assert maxrel(Y32[j], L32.matvec_Rs(V[j])) < 1e-12, j
        assert maxrel(Y64[j], L64.matvec_Rs(V[j])) < 1e-12, j
    assert not np.array_equal(Y32, Y64)    # the rounding is real


# 7 -------------------------------------------------------------------------
def test_f32_generator_rounds_on_store():
    """synth_ld_g computes G G^T in f64 and rounds on store: the f32 engine's
    blocks are exactly W(the f64 engine's blocks)."""
    sizes, nsamp = [700, 300], 500
    got = {}
    for bits in (64, 32):
        eng = Engine(sizes, K=1)
        eng.set_ld_precision(bits)
        eng.synth_ld_g(0, 11, nsamp, np.zeros(sum(sizes)))
        assert [eng.ld_block_precision(0, b) for b in range(2)] == [bits, bits]
        got[bits] = [eng.get_ld_block(0, b) for b in range(2)]
        eng.close()
    for b in range(2):
        assert not np.array_equal(got[64][b], W(got[64][b]))
        np.testing.assert_array_equal(got[32][b], W(got[64][b]))


# 8 -------------------------------------------------------------------------
def test_f32_form1_bitwise_the_f64_strips_on_widened_blocks():
    """The 8-B form of the float strip kernels gives every MFMA chain the operands,
    in the order, the double ones see on the widened matrix: bitwise equal
    products, at every column count (f64 arm: 512-column strips forced, mfma_min
    = 1).  The default is the 16-B form: the forced one's bits, not form 1's."""
    form1 = products(SIZES, NCOLS, env=FORM1)
    pin = products(SIZES, NCOLS, bits=64, env=F64_STRIPS, mfma_min=1, widen=True)
    form2 = products(SIZES, [4, 16], env=FORM2)
    for ncol in NCOLS:
        np.testing.assert_array_equal(form1[ncol][0], pin[ncol][0])
    for ncol in (4, 16):
        np.testing.assert_array_equal(main_products()["Y"][ncol][0], form2[ncol][0])
        assert not np.array_equal(form2[ncol][0], form1[ncol][0])


# 9 -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k1_defaults", "k2_shared", "k4_shared_s_damp", "k10_shared",
                                  "k1_blocks_csr_s_damp"])
def test_vamp_f32_end_to_end(name, tmp_path):
    """VAMP(ld_precision="f32") on golden cases: (a) within the project's 1e-5
    parity bar of the reference's golden xhat; (b) within 1e-8 of the oracle run
    on the widened blocks, with its CG iteration counts, CG info and EM steps;
    (c) every block stored at 32 bits."""
    c = Case(name)
    f = c.flags
    lds = [BlockLD(blocks, s=f["s"]) for blocks in c.ld_blocks]
    R = lds[0] if len(lds) == 1 else [lds[c.ld_of[k]] for k in range(c.K)]
    Nt = sum(c.N)
    v = VAMP(N=c.N, Nt=Nt, M=c.M, K=c.K, rho=f["rho"], gamw=f["gamw"], gam1=f["gam1"],
             a=np.array(c.N) / Nt, prior_vars=f["prior_vars"], prior_probs=f["prior_probs"],
             out_dir=str(tmp_path), out_name=c.name, seed=f["seed"], ld_precision="f32")
    xh = v.infer(R, c.r, f["iterations"], x0=c.x0, cg_maxit=f["cg_maxit"],
                 em_prior_maxit=f["em_prior_maxit"], learn_gamw=f["learn_gamw"],
                 lmmse_damp=f["lmmse_damp"], prior_update=f["prior_update"],
                 update_prior_from=f["update_prior_from"])
    prec = {v.engine.ld_block_precision(l, b) for l in range(v.engine.nld)
            for b in range(len(v.engine.block_sizes))}
    v.engine.close()
    wlds = [vo.BlockLD([W(B) for B in blocks], s=f["s"]) for blocks in c.ld_blocks]
    with np.errstate(all="ignore"):
        t = vo.infer(wlds, c.ld_of, list(c.r), c.N, f["iterations"], x0=c.x0, **c.kwargs())
    ea = eb = 0.0
    for it in range(f["iterations"]):
        x = xh[it].ravel() / np.sqrt(Nt)
        ea = max(ea, maxrel(x, c.xhat[it]))
        eb = max(eb, maxrel(x, np.asarray(t["xhat"][it])))
    print("%s: vs golden %.3e, vs oracle on widened blocks %.3e" % (name, ea, eb))
    assert ea < 1e-5, ea                                              # (a)
    assert eb < 1e-8, eb                                              # (b)
    cg = np.array([h["cg_iters"] for h in v.history])
    np.testing.assert_array_equal(cg, np.array(t["cg_iters"]))
    info = np.array([h["cg_info"] for h in v.history])
    np.testing.assert_array_equal(info, np.array(t["cg_info"]))
    assert [h["em_steps"] for h in v.history if "em_steps" in h] == list(t["em_steps"])
    assert prec == {32}                                               # (c)
