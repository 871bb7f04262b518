"""Exact-arithmetic gate of every LD pass form and its fused epilogue.

The inputs (tests/exact_ld.py) make every product and partial sum exactly
representable in f64 in any order, so every form of every pass -- whatever its
summation order, FMA contraction or storage -- must equal ONE integer reference
bit for bit: out, the carried yout and the panel dots, through
Engine.ld_pass_ex (sgv_ld_pass_ex: the whole PassArgs, the dots through the
CG's ordered reduction).  No tolerance appears in this file.

Every form names the kernel form it expects per column count, and the gate
asserts Engine.ld_pass_form against it before the passes: a switch that
silently fell back to another form would leave every product right and the
form uncovered.
"""
import contextlib
import os

import numpy as np
import pytest

from engine import Engine
from tests import exact_ld as xl

pytestmark = pytest.mark.gpu

AB_KEYS = ("SGV_AB", "SGV_MF_WIDE", "SGV_MF_PAIR", "SGV_MF_WIDE_IDLE", "SGV_BAND_WALK",
           "SGV_FIN_FORM", "SGV_F32_FORM")
YS = (xl.YS1, xl.YS0)
OUT_FILL, YOUT_FILL = -12345.5, 54321.25      # what out / yout hold before a pass
DOT_ALT, YOUT_ALT = 0x5555, 0x6666            # dot only, yout only, both, neither: columns 0..3


@contextlib.contextmanager
def environ(env):
    """The A/B switches `env` (SGV_AB=1 added) for the life of an engine: some
    are read when the plan is built, some at every launch."""
    old = {k: os.environ.get(k) for k in AB_KEYS}
    try:
        for k in AB_KEYS:
            os.environ.pop(k, None)
        if env:
            os.environ.update(dict(env, SGV_AB="1"))
        yield
    finally:
        for k in AB_KEYS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


class Data:
    """One regime's blocks with 16 right-hand sides, dot weights and the exact
    products R V and |R| |V|, computed once; a pass of ncol columns takes the
    first ncol (so every column count shares one reference, left unchanged)."""

    def __init__(self, blocks, regime, seed):
        self.blocks, self.regime, self.bits = blocks, regime, regime["bits"]
        self.sizes = [xl.block_size(B) for B in blocks]
        self.M = sum(self.sizes)
        self.V = xl.exact_rhs(16, self.M, regime["vmax"].bit_length(), seed)
        self.W = xl.exact_weights(16, self.M, regime.get("wmax", 1), seed + 1)
        xl.check_blocks(blocks, self.bits)
        self.RV = xl.matmul(blocks, self.V)
        self.RA = xl.abs_bound(blocks, self.V)
        for a in (self.V, self.W, self.RV, self.RA):
            a.setflags(write=False)

    def prefix(self, nblocks):
        """The same data restricted to the first nblocks blocks."""
        d = object.__new__(Data)
        d.blocks, d.regime, d.bits = self.blocks[:nblocks], self.regime, self.bits
        d.sizes = self.sizes[:nblocks]
        d.M = sum(d.sizes)
        d.V, d.W, d.RV, d.RA = (a[:, :d.M] for a in (self.V, self.W, self.RV, self.RA))
        return d


_data = {}


def data(kind, regime_name):
    key = (kind, regime_name)
    if key not in _data:
        regime = xl.NARROW if regime_name == "narrow" else xl.WIDE
        bits = regime["bits"]
        if kind == "tri":
            blocks = [xl.exact_block(n, bits, 11) for n in xl.TRI_SIZES]
        elif kind == "nonsym":
            blocks = [xl.exact_block(n, bits, 12, symmetric=False) for n in xl.DENSE_SIZES]
        elif kind == "mixed":   # band blocks beside triangles: strips with the ragged finalize
            blocks = [xl.Band(1537, bits, 16, 300), xl.exact_block(1281, bits, 11),
                      xl.Band(2305, bits, 16, 40), xl.exact_block(513, bits, 11)]
        elif kind == "hist_tri":
            blocks = [xl.exact_block(n, bits, 11) for n in xl.HIST_SIZES]
        elif kind == "hist_band":
            blocks = [xl.Band(n, bits, 14, bw) for n, bw in zip(xl.HIST_SIZES, xl.HIST_BWS)]
        elif kind == "coupled":
            blocks = [xl.Band(xl.COUPLED["M"], bits, 15, xl.COUPLED["bw"])]
        else:                   # ("walk", bw)
            blocks = [xl.Band(n, bits, 13, kind[1]) for n in xl.walk_sizes(kind[1])]
        _data[key] = Data(blocks, regime, 100 + len(_data))
    return _data[key]


def upload(eng, ld, d):
    for b, B in enumerate(d.blocks):
        if isinstance(B, xl.Band):
            eng.set_ld_block_csr(ld, b, B)
        else:
            eng.set_ld_block(ld, b, B)


def call(eng, ld, d, ncol, c1, c2, w=None, dot_mask=0, yout_mask=0, run=-1, V=None):
    """One ld_pass_ex over the first ncol columns of d (or V), out and yout
    pre-filled; w: None (no dots), "alias" (the CG's p.q) or the weights."""
    V = d.V[:ncol] if V is None else V
    wd = None if w is None or isinstance(w, str) else w
    return eng.ld_pass_ex(ld, V, c1, c2, w=wd, dot_mask=dot_mask, yout_mask=yout_mask,
                          ys1=YS[0], ys0=YS[1], run=run, out=np.full_like(V, OUT_FILL),
                          yout=np.full_like(V, YOUT_FILL))


def expect(d, ncol, c1, c2, w, dot_mask, yout_mask, tag, got):
    """got = (out, yout, dots) equals the exact reference: out everywhere, yout
    on its mask and untouched elsewhere, the dots on their mask."""
    V = d.V[:ncol]
    wv = None if w is None else (V if isinstance(w, str) else w)
    xl.check_exact(None, V, c1, c2, d.bits, w=wv, ys=YS if yout_mask else None, RA=d.RA)
    out, yout, dots = xl.reference(d.RV[:ncol], V, c1, c2, w=wv, ys=YS)
    np.testing.assert_array_equal(got[0], out, err_msg="out %s" % (tag,))
    for j in range(ncol):
        want = yout[j] if yout_mask >> j & 1 else np.full(d.M, YOUT_FILL)
        np.testing.assert_array_equal(got[1][j], want, err_msg="yout %s column %d" % (tag, j))
        if dot_mask >> j & 1:
            assert got[2][j] == dots[j], ("dot", tag, j, got[2][j], dots[j])


def kinds(small, mid, **more):
    """ncol -> the PassForm fields a form expects: the packed kind `small` at 1-2
    columns, `mid` at 3-8, the 16x16x4 strips above; `more` at every count."""
    return lambda n: dict(kind=small if n <= 2 else mid if n <= 8 else "strip16", **more)


def assert_form(eng, ld, ncol, want, tag):
    """The form the next pass of ncol columns over ld reports is `want`(ncol),
    with what follows from the kind: the VALU class, the Pk layout of an MFMA
    pass, the 9-16-column counter flag, no finalize form without strip finalize."""
    f = eng.ld_pass_form(ld, ncol)
    w = dict(want(ncol))
    if w["kind"] == "valu":
        w.update(valu_class=0 if ncol <= 2 else 1 if ncol <= 4 else 2 if ncol <= 8 else 3,
                 pk_width=0, load_form=0, fin_form=0)
    elif w["kind"] != "none":
        w.update(pk_width=4 if ncol <= 4 else 8 if ncol <= 8 else 16, pk_paired=4 < ncol <= 8)
    w.setdefault("mfma16", w["kind"] == "strip16")
    if w["kind"] == "wide":
        w.setdefault("idle_exit", True)
    else:
        w.setdefault("rest_kind", "none")
    got = {k: getattr(f, k) for k in w}
    assert got == w, (tag, ld, ncol, f)


def epilogue_gate(eng, dn, dw, ncols, tag, want, ld_n=0, ld_w=1):
    """Every column count of one form on one engine: the reported form, then the
    narrow-regime epilogue calls (out, yout, dots), the wide-bit call (out), the
    two run calls."""
    for ncol in ncols:
        for ld in (ld_n, ld_w):
            assert_form(eng, ld, ncol, want, tag)
        full = (1 << ncol) - 1
        c1, c2 = xl.narrow_coeffs(ncol)
        W = dn.W[:ncol]
        # alternating, non-identical masks with distinct weights
        dm, ym = DOT_ALT & full, YOUT_ALT & full
        first = call(eng, ld_n, dn, ncol, c1, c2, W, dm, ym)
        expect(dn, ncol, c1, c2, W, dm, ym, (tag, ncol, "alt"), first)
        # everything on, the dots aliasing the input (the CG's pass)
        got = call(eng, ld_n, dn, ncol, c1, c2, "alias", full, full)
        expect(dn, ncol, c1, c2, "alias", full, full, (tag, ncol, "all"), got)
        # nothing but out
        got = call(eng, ld_n, dn, ncol, c1, c2)
        expect(dn, ncol, c1, c2, None, 0, 0, (tag, ncol, "none"), got)
        # wide-bit: out only
        k1, k2 = xl.wide_coeffs(ncol)
        got = call(eng, ld_w, dw, ncol, k1, k2)
        expect(dw, ncol, k1, k2, None, 0, 0, (tag, ncol, "wide-bit"), got)
        assert np.median(xl.significant_bits(got[0], dw.bits)) > 24
        # run = 0: a no-op, out and yout come back as they went in
        out, yout, _ = call(eng, ld_n, dn, ncol, c1, c2, W, dm, full, run=0)
        np.testing.assert_array_equal(out, np.full_like(out, OUT_FILL), err_msg=str((tag, ncol)))
        np.testing.assert_array_equal(yout, np.full_like(out, YOUT_FILL), err_msg=str((tag, ncol)))
        # run = 1 is run = -1
        got = call(eng, ld_n, dn, ncol, c1, c2, W, dm, ym, run=1)
        for a, b in zip(got[:2], first[:2]):
            np.testing.assert_array_equal(a, b, err_msg="run=1 %s" % ((tag, ncol),))
        expect(dn, ncol, c1, c2, W, dm, ym, (tag, ncol, "run=1"), got)


def nan_gate(eng, dn, ncols, tag, ld=0):
    """A diverged cohort stays in its column: one column all NaN, every other
    column's out, yout and dot bitwise the reference's, the NaN column all NaN."""
    for ncol in ncols:
        full = (1 << ncol) - 1
        c1, c2 = xl.narrow_coeffs(ncol)
        bad = ncol - 2
        V = np.array(dn.V[:ncol])
        V[bad] = np.nan
        for w in (dn.W[:ncol], "alias"):
            out, yout, dots = call(eng, ld, dn, ncol, c1, c2, w, full, full, V=V)
            wv = dn.V[:ncol] if isinstance(w, str) else w
            ro, ry, rd = xl.reference(dn.RV[:ncol], dn.V[:ncol], c1, c2, w=wv, ys=YS)
            for j in range(ncol):
                if j == bad:
                    assert np.isnan(out[j]).all() and np.isnan(yout[j]).all() and np.isnan(dots[j]), \
                        (tag, ncol, j)
                    continue
                np.testing.assert_array_equal(out[j], ro[j], err_msg=str((tag, ncol, j)))
                np.testing.assert_array_equal(yout[j], ry[j], err_msg=str((tag, ncol, j)))
                assert dots[j] == rd[j], (tag, ncol, j, dots[j], rd[j])


def nan_cols(ncols):
    return [n for n in (5, 8, 13) if n in ncols]


def two_matrix_engine(dn, dw, setup=None, fmt=None, bits=None):
    """An engine holding the narrow-regime matrix as LD 0, the wide-bit one as LD 1."""
    eng = Engine(dn.sizes, K=2, ld_of=[0, 1])
    if setup:
        setup(eng)
    upload(eng, 0, dn)
    upload(eng, 1, dw)
    for ld in (0, 1):
        for b in range(len(dn.sizes)):
            if fmt is not None:
                want = fmt(dn.sizes[b]) if callable(fmt) else fmt
                assert eng.ld_block_format(ld, b) == want, (ld, b)
            if bits is not None and eng.ld_block_format(ld, b) != 0:
                assert eng.ld_block_precision(ld, b) == bits, (ld, b)
    return eng


# ---- triangle, dense and f32 geometry ---------------------------------------
ALL = list(range(1, 17))
TRI_FORMS = {
    # name: (A/B switches, engine setup, columns, data kind, blocks kept, format, stored bits,
    #        the form expected per column count)
    # triangles: no strip is ragged (finalize 4); the wide form has no strip finalize
    "default": ({}, None, ALL, "tri", None, 1, 64,
                kinds("valu", "wide", load_form=1, dense=False)),
    "valu": ({}, lambda e: e.set_mfma_min(0), ALL, "tri", None, 1, 64,
             lambda n: dict(kind="valu")),
    "strips4": ({"SGV_MF_WIDE": "0", "SGV_MF_PAIR": "0"}, None, list(range(3, 17)), "tri", None,
                1, 64, kinds("valu", "strip4", load_form=1, fin_form=4)),
    "pair": ({"SGV_MF_PAIR": "1"}, None, list(range(3, 9)), "tri", None, 1, 64,
             kinds("valu", "pair", load_form=1, fin_form=4)),
    "wide": ({"SGV_MF_WIDE": "1"}, None, list(range(3, 9)), "tri", None, 1, 64,
             kinds("valu", "wide", load_form=1, fin_form=0, rest_kind="none")),
    "dense": ({}, lambda e: e.set_ld_packing(False), ALL, "tri", len(xl.DENSE_SIZES), 0, 64,
              lambda n: dict(kind="none", dense=True)),
    # the block of one marker is symmetric, so packed: it runs as a triangle beside the squares
    "nonsym": ({}, None, ALL, "nonsym", None, lambda n: 0 if n > 1 else 1, 64,
               kinds("valu", "wide", dense=True)),
    "f32_16B": ({}, lambda e: e.set_ld_precision(32), ALL, "tri", None, 1, 32,
                kinds("strip4", "strip4", load_form=2, fin_form=4)),
    "f32_8B": ({"SGV_F32_FORM": "1"}, lambda e: e.set_ld_precision(32), ALL, "tri", None, 1, 32,
               kinds("strip4", "strip4", load_form=1, fin_form=4)),
    # mixed: the triangles wide, the band blocks' ragged 512-column strips behind them
    "fin1": ({"SGV_FIN_FORM": "1"}, None, list(range(3, 17)), "mixed", None, None, 64,
             lambda n: dict(kinds("valu", "wide", fin_form=1)(n),
                            **({"rest_kind": "strip4"} if n <= 8 else {}))),
    "fin4": ({"SGV_FIN_FORM": "4"}, None, list(range(3, 17)), "mixed", None, None, 64,
             lambda n: dict(kinds("valu", "wide", fin_form=4)(n),
                            **({"rest_kind": "strip4"} if n <= 8 else {}))),
}


@pytest.mark.parametrize("form", list(TRI_FORMS))
def test_triangle_forms_exact(form):
    """Every pass form over dense-triangle, full-square and f32 storage, each at
    all of its column counts on one engine holding TRI_SIZES (the full-square
    forms without 8449; the finalize forms on a plan mixing bands and triangles)."""
    env, setup, ncols, kind, keep, fmt, bits, want = TRI_FORMS[form]
    dn, dw = data(kind, "narrow"), data(kind, "wide")
    if keep is not None:
        dn, dw = dn.prefix(keep), dw.prefix(keep)
    with environ(env):
        eng = two_matrix_engine(dn, dw, setup, fmt, bits)
        if kind == "mixed":
            assert {eng.ld_block_format(0, b) for b in range(len(dn.sizes))} == {1, 2}
        epilogue_gate(eng, dn, dw, ncols, form, want)
        nan_gate(eng, dn, nan_cols(ncols), form)
        eng.close()


# ---- band geometry: walks, band strips, VALU, f32 ---------------------------
# bw -> are the band's 512-column strips ragged: a panel stores round_up(256 + bw,
# 256) columns -- 512 or 1,024 at bw = 200 / 600, whole 512-column items; 768 or
# 1,280 at bw = 300 / 1,000, whose strips end in a 256-column item
BAND_RAGGED = {200: False, 300: True, 600: False, 1000: True}


def band_strips(bw, small, **more):
    """The band strips' form: the ragged set takes the 4-wave kernel and, up to 8
    columns, finalize 1; the even set the kernel of the launch-tail model
    (BAND_STRIPS_EVEN) and finalize 4."""
    def want(n):
        w = kinds(small, "strip4" if BAND_RAGGED[bw] else BAND_STRIPS_EVEN, **more)(n)
        if w["kind"] != "valu":
            w["fin_form"] = 1 if BAND_RAGGED[bw] and n <= 8 else 4
        return w
    return want


# walk_sizes(200) and walk_sizes(600) make fewer strips than either strip kernel
# has slots on the 256 CUs of an MI355X, so the tail model (ldplan.hip
# mfma_pair_choice) sees the pair kernel's 256 slots twice as well filled as the
# 4-wave kernel's 512, far above its 3 % margin: the "strips" arm of these two
# runs the wave-pair strips, that of bw = 300 and 1,000 the 4-wave ones
BAND_STRIPS_EVEN = "pair"
BAND_FORMS = {
    # 1-2 VALU, 3-8 the walks, 9-16 the band strips
    "walks": ({}, None, ALL, lambda bw: kinds("valu", "walk", load_form=1)),
    "strips": ({"SGV_BAND_WALK": "0"}, None, ALL,
               lambda bw: band_strips(bw, "valu", load_form=1)),
    "valu": ({}, lambda e: e.set_mfma_min(0), ALL, lambda bw: lambda n: dict(kind="valu")),
    # SGV_F32_WALK set in the shell fails here: the 3-8-column passes would report the walks
    "f32": ({}, lambda e: e.set_ld_precision(32), ALL,
            lambda bw: lambda n: dict(band_strips(bw, "strip4", load_form=2)(n),
                                      kind="strip4" if n <= 8 else "strip16")),
}


@pytest.mark.parametrize("bw", xl.WALK_BWS)
@pytest.mark.parametrize("form", list(BAND_FORMS))
def test_band_forms_exact(form, bw):
    """Band blocks only (so the plan takes walks), one engine per ring size R =
    2..5: P = R + 1 .. 2 W + 2 panels with ragged, half and whole last panels --
    blocks shorter than a walk, exactly W, W + 1 and 2 W panels, trailing walks
    of 1 .. R - 2 panels, single carry slots."""
    env, setup, ncols, want = BAND_FORMS[form]
    dn, dw = data(("walk", bw), "narrow"), data(("walk", bw), "wide")
    with environ(env):
        eng = two_matrix_engine(dn, dw, setup, 2, 32 if form == "f32" else 64)
        epilogue_gate(eng, dn, dw, ncols, (form, bw), want(bw))
        nan_gate(eng, dn, nan_cols(ncols), (form, bw))
        eng.close()


# ---- coupled band pieces -----------------------------------------------------
def test_coupled_pieces_exact():
    """One band cut into coupled pieces with a ragged last piece: the pieces'
    passes plus the corner couplings equal the whole band's exact product."""
    from sgvamp import BlockLD, band_cuts

    ncols = [1, 2, 3, 4, 5, 6, 7, 8, 16]
    dn, dw = data("coupled", "narrow"), data("coupled", "wide")
    sizes = None
    with environ({}):
        eng = None
        for ld, d in ((0, dn), (1, dw)):
            L = BlockLD.from_csr(d.blocks[0].scipy_csr(), block_sizes=[d.M])
            cuts = band_cuts([L], L.block_sizes, piece=xl.COUPLED["piece"])
            P, cpl = L.pieces(cuts)
            assert len(P.block_sizes) == 4 and P.block_sizes[-1] % 256 != 0, P.block_sizes
            if eng is None:
                sizes = P.block_sizes
                eng = Engine(sizes, K=2, ld_of=[0, 1])
            assert P.block_sizes == sizes and sorted(cpl) == [0, 1, 2]
            for b in range(len(sizes)):
                P.upload(eng, ld, b)
                assert eng.ld_block_format(ld, b) == 2
            for gb, (nr, nc, C) in cpl.items():
                eng.set_ld_coupling(ld, gb, nr, nc, C)
        # band pieces only: 1-2 VALU, 3-8 the walks, 16 the band strips
        epilogue_gate(eng, dn, dw, ncols, "coupled", kinds("valu", "walk", load_form=1))
        nan_gate(eng, dn, nan_cols(ncols), "coupled")
        eng.close()


# ---- history independence ----------------------------------------------------
def test_history_independence():
    """A pass's result does not depend on what ran before it on the context: a
    fixed pseudo-random sequence of passes over an f64 triangle, an f64 band and
    an f32 triangle of one partition, every column count, mask and run value --
    every result the exact reference (stale partials, head/carry buffers, Pk
    layouts left by a pass of another width, counters)."""
    tri, band = data("hist_tri", "narrow"), data("hist_band", "narrow")
    per_ld = [tri, band, tri]
    with environ({}):
        eng = Engine(xl.HIST_SIZES, K=3, ld_of=[0, 1, 2])
        upload(eng, 0, tri)
        upload(eng, 1, band)
        eng.set_ld_precision(32)
        upload(eng, 2, tri)
        for b in range(len(xl.HIST_SIZES)):
            assert [eng.ld_block_format(ld, b) for ld in range(3)] == [1, 2, 1]
            assert [eng.ld_block_precision(ld, b) for ld in range(3)] == [64, 64, 32]
        want = [kinds("valu", "wide", load_form=1), kinds("valu", "walk", load_form=1),
                kinds("strip4", "strip4", load_form=2, fin_form=4)]
        rs = np.random.RandomState(2024)
        # every (matrix, column count) cell once in a shuffled order, then 24 more
        cells = list(rs.permutation(48)) + list(rs.randint(48, size=24))
        for step, cell in enumerate(cells):
            ld, ncol = int(cell) // 16, int(cell) % 16 + 1
            full = (1 << ncol) - 1
            dm, ym = int(rs.randint(1 << 16)) & full, int(rs.randint(1 << 16)) & full
            run = int(rs.choice([-1, -1, 1, 0]))
            w = "alias" if rs.randint(2) else per_ld[ld].W[:ncol]
            c1, c2 = xl.narrow_coeffs(ncol)
            d = per_ld[ld]
            assert_form(eng, ld, ncol, want[ld], ("history", step))
            got = call(eng, ld, d, ncol, c1, c2, w if dm else None, dm, ym, run=run)
            tag = ("history", step, ld, ncol, hex(dm), hex(ym), run)
            if run == 0:
                np.testing.assert_array_equal(got[0], np.full_like(got[0], OUT_FILL), err_msg=str(tag))
                np.testing.assert_array_equal(got[1], np.full_like(got[0], YOUT_FILL), err_msg=str(tag))
            else:
                expect(d, ncol, c1, c2, w if dm else None, dm, ym, tag, got)
        eng.close()
