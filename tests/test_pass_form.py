"""The LD pass's form decision (csrc/pass_form.cpp) on a machine without a GPU,
through sgv_pass_form_model: the whole product of plan shapes, column counts,
sgv_set_mfma_min values and switch settings -- every case, none sampled --
against the rules the dispatcher had before the decision was one function, and
a literal table of the default form on the plan shapes that exist."""
import ctypes
import itertools

import numpy as np
import pytest

import hip_backend as hb

KIND = {n: i for i, n in enumerate(hb.PASS_KINDS)}
PF = {n: i for i, n in enumerate(hb.PASS_FORM_FIELDS)}
PS = {n: i for i, n in enumerate(hb.PLAN_SHAPE_FIELDS)}
MFMA_MINS = (0, 1, 3, 9)
# each switch: unset (-1) first, then each of its values, in hb.PASS_SWITCHES order
SW_VALUES = ((-1, 0), (-1, 1), (-1, 0, 1), (-1, 0, 1), (-1, 0), (-1, 1, 2), (-1, 1, 4))
BAND_WALK, F32_WALK, MF_WIDE, MF_PAIR, MF_WIDE_IDLE, F32_FORM, FIN_FORM = range(7)


def _model():
    """sgv_pass_form_model taking addresses: four million calls in a few seconds."""
    lib = hb.load()
    vp = ctypes.c_void_p
    proto = ctypes.CFUNCTYPE(ctypes.c_int, vp, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int)
    return proto(("sgv_pass_form_model", lib))


def shapes(bits):
    """[nc 16][walks 2][wide 2][rest 2][ragged 2][pair 3] plan shapes of one
    element type: packed panels, no dense block, every set in one block group;
    the rest set is as ragged and as paired as the 512-column set."""
    rows, ncs = [], []
    for nc, walks, wide, rest, ragged, pair in itertools.product(
            range(1, 17), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1, 2)):
        s = np.zeros(len(PS), dtype=np.int32)
        s[[PS["bits"], PS["packed"], PS["walks"], PS["wide"], PS["rest"]]] = bits, 1, walks, wide, rest
        s[[PS["ragged"], PS["rest_ragged"], PS["pair"], PS["rest_pair"]]] = ragged, ragged, pair, pair
        s[[PS["wide_idle"], PS["ngrp"], PS["wide_ngrp"], PS["rest_ngrp"]]] = 1
        rows.append(s)
        ncs.append(nc)
    return np.array(rows), np.array(ncs)


SWITCH_GRID = np.array(list(itertools.product(*SW_VALUES)), dtype=np.int32)
GRID_SHAPE = tuple(len(v) for v in SW_VALUES)


@pytest.fixture(scope="module")
def sweep():
    """{(bits, mfma_min): (shapes [768][14], nc [768], forms [768][648][12])}."""
    fn = _model()
    out = {}
    sw0, swn = SWITCH_GRID.ctypes.data, SWITCH_GRID.shape[0]
    for bits in (64, 32):
        S, nc = shapes(bits)
        for mm in MFMA_MINS:
            F = np.full((S.shape[0], swn, len(PF)), -99, dtype=np.int32)
            o = F.ctypes.data
            for i in range(S.shape[0]):
                a, n = S.ctypes.data + S.strides[0] * i, int(nc[i])
                for j in range(swn):
                    if fn(a, sw0 + 28 * j, mm, n, o, 12):
                        raise AssertionError((bits, mm, i, j))
                    o += 48
            assert (F != -99).all()
            out[(bits, mm)] = (S, nc, F)
    return out


def cases(sweep):
    """Per (bits, mfma_min): the shape columns broadcast over the switch grid."""
    for (bits, mm), (S, nc, F) in sweep.items():
        col = lambda a: np.asarray(a)[:, None]
        sh = {k: col(S[:, i]) for k, i in PS.items()}
        sw = {k: SWITCH_GRID[None, :, k] for k in range(7)}
        f = {k: F[:, :, i] for k, i in PF.items()}
        mf = np.broadcast_to((bits == 32) | ((mm > 0) & (col(nc) >= mm)), f["kind"].shape)
        yield bits, mm, col(nc), sh, sw, f, mf


def test_rules(sweep):
    """The dispatcher's rules, each as an iff over the whole product."""
    for bits, mm, nc, sh, sw, f, mf in cases(sweep):
        k = f["kind"]
        # f64: MFMA iff mfma_min > 0 and nc >= mfma_min, else the VALU class; f32: always MFMA
        assert ((k == KIND["valu"]) == ~mf).all()
        cls = np.where(nc <= 2, 0, np.where(nc <= 4, 1, np.where(nc <= 8, 2, 3)))
        assert (f["valu_class"] == np.where(mf, -1, cls)).all()
        if bits == 32:
            assert not np.isin(k, [KIND["valu"], KIND["pair"], KIND["wide"]]).any()
            assert (f["rest_kind"] == KIND["none"]).all()
        walk = (mf & (sh["walks"] == 1) & (nc <= 8) & (sw[BAND_WALK] != 0)
                & ((bits == 64) | ((nc >= 3) & (sw[F32_WALK] == 1))))
        assert ((k == KIND["walk"]) == walk).all()
        wide = (mf & ~walk & (bits == 64) & (sh["wide"] == 1) & (nc >= 3) & (nc <= 8)
                & ((sw[MF_WIDE] == 1) | ((sw[MF_WIDE] == -1) & (sw[MF_PAIR] == -1))))
        assert ((k == KIND["wide"]) == wide).all()
        strips = mf & ~walk & ~wide
        pair_set = (bits == 64) & (sh["ragged"] == 0) & (sh["pair"] >= 1) & (nc <= 8)
        assert ((k == KIND["pair"]) == (strips & pair_set)).all()
        assert ((k == KIND["strip16"]) == (mf & (nc > 8))).all()
        assert ((k == KIND["strip4"]) == (strips & ~pair_set & (nc <= 8))).all()
        assert (f["mfma16"] == (k == KIND["strip16"])).all()
        # under a wide pass rest runs behind it as 512-column strips
        rest = wide & (sh["rest"] == 1)
        assert (f["rest_kind"] == np.where(rest, np.where(pair_set, KIND["pair"], KIND["strip4"]),
                                           KIND["none"])).all()
        assert (f["idle_exit"] == wide).all()
        # Pk: 4 / 8 / 16 doubles per row, paired at 5-8 columns (walks: above 4, and they stop at 8)
        assert (f["pk_width"] == np.where(mf, np.where(nc > 8, 16, np.where(nc <= 4, 4, 8)), 0)).all()
        assert (f["pk_paired"] == (mf & (nc > 4) & (nc <= 8))).all()
        # finalize: forced, else 1 for ragged sets at up to 8 columns, else 4; none without strips
        fin = np.where(sw[FIN_FORM] > 0, sw[FIN_FORM], np.where((sh["ragged"] == 1) & (nc <= 8), 1, 4))
        assert (f["fin_form"] == np.where(strips | rest, fin, 0)).all()
        # load form: f64 the 8-B one; f32 the switch, else the default (16 B, strips and walks)
        lf = 1 if bits == 64 else np.where(sw[F32_FORM] > 0, sw[F32_FORM], 2)
        assert (f["load_form"] == np.where(mf, lf, 0)).all()
        assert (f["dense"] == 0).all() and (f["side"] == 0).all() and (f["rest_side"] == 0).all()


def test_unset_is_the_documented_default(sweep):
    """A switch left unset gives the form of its documented default (DESIGN.md
    Appendix B) where that default is one of its values: SGV_MF_WIDE 1 (with
    SGV_MF_PAIR unset), SGV_F32_FORM 2, SGV_FIN_FORM 1 for ragged sets at up to
    8 columns and 4 otherwise.  The other four have no value that spells their
    default (walks on, f32 walks off, pair by the model, idle exit on):
    test_rules holds those."""
    for bits, mm, nc, sh, sw, f, mf in cases(sweep):
        F = np.stack([f[k] for k in hb.PASS_FORM_FIELDS], axis=-1)
        G = F.reshape((F.shape[0],) + GRID_SHAPE + (F.shape[-1],))
        idx = lambda ax, i: (slice(None),) * (1 + ax) + (i,)
        np.testing.assert_array_equal(G[idx(MF_WIDE, 0)][idx(MF_PAIR - 1, 0)],
                                      G[idx(MF_WIDE, 2)][idx(MF_PAIR - 1, 0)])
        np.testing.assert_array_equal(G[idx(F32_FORM, 0)], G[idx(F32_FORM, 2)])
        fin1 = ((sh["ragged"] == 1) & (nc <= 8)).reshape((-1,) + (1,) * 7)
        np.testing.assert_array_equal(
            G[idx(FIN_FORM, 0)], np.where(fin1, G[idx(FIN_FORM, 1)], G[idx(FIN_FORM, 2)]))


def test_each_switch_moves_only_its_rows(sweep):
    """Against the same case with the switch unset, a switch changes only the
    rows its line in Appendix B claims, and only the fields it is about."""
    fields = np.array(hb.PASS_FORM_FIELDS)
    for bits, mm, nc, sh, sw, f, mf in cases(sweep):
        F = np.stack([f[k] for k in hb.PASS_FORM_FIELDS], axis=-1)
        G = F.reshape((F.shape[0],) + GRID_SHAPE + (F.shape[-1],))
        ncg = nc.reshape((-1,) + (1,) * 6)
        shg = {k: v.reshape((-1,) + (1,) * 6) for k, v in sh.items()}

        def moved(ax, i):
            """rows and fields that differ between value i and unset of switch ax"""
            at = lambda j: G[(slice(None),) * (1 + ax) + (j,)]
            d = at(i) != at(0)
            return at(0), d.any(axis=-1), set(fields[d.any(axis=tuple(range(d.ndim - 1)))])

        base, rows, what = moved(BAND_WALK, 1)        # 0: the walks' passes, onto strips
        assert (rows == (base[..., PF["kind"]] == KIND["walk"])).all()
        base, rows, what = moved(F32_WALK, 1)         # 1: f32 walk plans at 3-8 columns, onto the walks
        assert not (rows & ~((bits == 32) & (shg["walks"] == 1) & (ncg >= 3) & (ncg <= 8))).any()
        for i in (1, 2):                              # wide / pair: f64 3-8-column passes over wide strips
            for ax in (MF_WIDE, MF_PAIR):
                base, rows, what = moved(ax, i)
                assert not (rows & ~((bits == 64) & (shg["wide"] == 1) & (ncg >= 3) & (ncg <= 8))).any()
                assert not rows[base[..., PF["kind"]] == KIND["walk"]].any()
        base, rows, what = moved(MF_WIDE_IDLE, 1)     # read when the plan is built: no pass moves
        assert not rows.any()
        for i in (1, 2):                              # the float kernels' loads and nothing else
            base, rows, what = moved(F32_FORM, i)
            assert what <= {"load_form"} and (bits == 32 or not rows.any())
            base, rows, what = moved(FIN_FORM, i)     # the strip finalize where one runs
            assert what <= {"fin_form"} and not rows[base[..., PF["fin_form"]] == 0].any()


def test_plan_kept_values_and_dense_blocks():
    """What the plan keeps reaches the form unchanged -- the wide kernel's idle
    exit, the block groups' side streams -- and dense row groups run beside any
    packed kind, alone without packed panels."""
    wide = dict(packed=1, wide=1, rest=1, ragged=1, rest_ragged=1)
    for idle, g, wg, rg, dense in itertools.product((0, 1), (1, 3), (1, 2), (1, 8), (0, 1)):
        shape = dict(wide, wide_idle=idle, ngrp=g, wide_ngrp=wg, rest_ngrp=rg, dense=dense)
        f = hb.pass_form_model(shape, {}, 3, 4)
        assert (f.kind, f.idle_exit, f.side, f.rest_side, f.dense) == ("wide", bool(idle), wg > 1,
                                                                      rg > 1, bool(dense))
        f = hb.pass_form_model(shape, {}, 3, 16)
        assert (f.kind, f.idle_exit, f.side, f.rest_side, f.dense) == ("strip16", False, g > 1,
                                                                      False, bool(dense))
        f = hb.pass_form_model(dict(shape, packed=0), {}, 3, 4)
        assert (f.kind, f.dense, f.pk_width, f.side) == ("none", bool(dense), 0, False)


def test_model_refuses_bad_arguments():
    lib = hb.load()
    sh = np.zeros(len(PS), dtype=np.int32)
    sh[PS["bits"]] = 64
    sw = np.full(7, -1, dtype=np.int32)
    out = np.zeros(len(PF), dtype=np.int32)
    call = lambda s, w, nc, o=out, cap=len(PF): lib.sgv_pass_form_model(
        None if s is None else hb.iptr(s), None if w is None else hb.iptr(w), 3, nc,
        None if o is None else hb.iptr(o), cap)
    assert call(sh, sw, 4) == hb.SGV_OK
    for nc in (0, 17):
        assert call(sh, sw, nc) != hb.SGV_OK
    assert call(None, sw, 4) != hb.SGV_OK and call(sh, None, 4) != hb.SGV_OK
    assert call(sh, sw, 4, None) != hb.SGV_OK and call(sh, sw, 4, out, -1) != hb.SGV_OK
    bad = sh.copy()
    bad[PS["bits"]] = 16
    assert call(bad, sw, 4) != hb.SGV_OK
    for i, values in enumerate(SW_VALUES):      # a value the reader would not pass on
        w = sw.copy()
        w[i] = max(values) + 1
        assert call(sh, w, 4) != hb.SGV_OK
    out[:] = -7                                  # a shorter caller gets that prefix
    assert call(sh, sw, 4, out, 3) == hb.SGV_OK and (out[3:] == -7).all()


# The default form (no switch, mfma_min = 3) on the plan shapes that exist, read
# from the dispatcher as it stood before pass_form (ld_pass, launch_sym_mfma,
# launch_mf, fin_form, f32_form of that revision).  Per shape: (columns, (kind,
# VALU class, rest kind, load form, finalize form, Pk width, Pk paired, 9-16 flag)).
V0 = ("valu", 0, "none", 0, 0, 0, False, False)


def _mfma(kind, lf, fin, rest="none"):
    return [((3, 4), (kind, -1, rest, lf, fin, 4, False, False)),
            ((5, 6, 7, 8), (kind, -1, rest, lf, fin, 8, True, False))]


def _top(lf):
    return [(tuple(range(9, 17)), ("strip16", -1, "none", lf, 4, 16, False, True))]


def _f32(fin):
    return ([((1, 2), ("strip4", -1, "none", 2, fin, 4, False, False))] + _mfma("strip4", 2, fin)
            + _top(2))


TRI = dict(packed=1, wide=1)
BAND = dict(packed=1, ragged=1)
DEFAULT_TABLE = {
    # dense triangles: the wide strips at 3-8 columns, whichever 512-column kernel the plan chose
    "triangles f64": (dict(TRI), [((1, 2), V0)] + _mfma("wide", 1, 0) + _top(1)),
    "triangles f64, pair by the model": (dict(TRI, pair=1), [((1, 2), V0)] + _mfma("wide", 1, 0) + _top(1)),
    # an f32 plan builds no wide strips and, by default, no walk tables
    "triangles f32": (dict(packed=1, bits=32), _f32(4)),
    "triangles f32, pair by the model": (dict(packed=1, bits=32, pair=1), _f32(4)),
    "walk-eligible bands f64": (dict(BAND, walks=1), [((1, 2), V0)] + _mfma("walk", 1, 0) + _top(1)),
    "walk-eligible bands f32": (dict(BAND, bits=32), _f32(1)),
    "bands beyond the walks f64": (dict(BAND), [((1, 2), V0)] + _mfma("strip4", 1, 1) + _top(1)),
    "bands beyond the walks f32": (dict(BAND, bits=32), _f32(1)),
    # triangles and bands: the triangles wide, the bands' ragged strips behind them
    "mixed f64": (dict(BAND, wide=1, rest=1, rest_ragged=1),
                  [((1, 2), V0)] + _mfma("wide", 1, 1, rest="strip4") + _top(1)),
    "mixed f32": (dict(BAND, bits=32), _f32(1)),
    "full squares": (dict(dense=1), [(tuple(range(1, 17)), ("none", -1, "none", 0, 0, 0, False, False))]),
}


@pytest.mark.parametrize("name", list(DEFAULT_TABLE))
def test_default_form_table(name):
    shape, rows = DEFAULT_TABLE[name]
    seen = []
    for ncols, want in rows:
        for nc in ncols:
            f = hb.pass_form_model(shape, {}, 3, nc)
            got = (f.kind, f.valu_class, f.rest_kind, f.load_form, f.fin_form, f.pk_width,
                   f.pk_paired, f.mfma16)
            assert got == want, (name, nc, f)
            assert f.dense == bool(shape.get("dense")) and f.idle_exit == (f.kind == "wide")
            seen.append(nc)
    assert seen == list(range(1, 17))
