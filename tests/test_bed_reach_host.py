"""Distance-windowed LD from .bed genotypes, host side (no GPU): the definition of
include/sgvamp_hip.h, "distance-windowed genotype LD", restated here with loops.

  reach   hi[i] = max{ j : i <= j < n, pos[j] - pos[i] <= D } (that f64 subtraction
          and comparison), cut to i + W where a marker window is given too;
  kept    (i, j), j >= i, iff j <= hi[i]; exactly 0.0 elsewhere; the mirror below;
  taper   acc * (1.0 - (pos[j] - pos[i]) / D).

BedLD.reach against the double loop; BedLD.block and GenoCoupling.host against
tests/bed_ref.R under a mask and weight built here (the bar is tests/
test_gpu_geno_ld.py's 1e-12 for this contraction, the support exact); pieces plus
couplings against the uncut block; every refusal; chromosome_blocks; and the
reason for the taper: the hard window's smallest eigenvalue is < -0.1 on three
panels, the tapered one's > 0 (recorded: -0.298 / +0.265, -0.650 / +0.153,
-0.543 / +0.118)."""
import functools

import numpy as np
import pytest

from tests import bed_ref

from ldio import BedLD, GenoCoupling, chromosome_blocks, load_bed_ld, read_bed, write_bed
from sgvamp import BlockLD, band_cuts

TOL = 1e-12    # tests/test_gpu_geno_ld.py's bar for this contraction


def maxrel(a, b):
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


def clustered(n):
    """Positions with ties and gaps from 0 to 400: the reach varies along the block."""
    return np.cumsum(np.random.RandomState(3).choice([0, 1, 5, 50, 400], n,
                                                     p=[.1, .3, .3, .2, .1])).astype(np.float64)


def brute_hi(pos, D, W=None):
    n = len(pos)
    hi = np.empty(n, dtype=np.int64)
    for i in range(n):
        h = i
        for j in range(i, n):
            if pos[j] - pos[i] <= D and (W is None or j - i <= W):
                h = j
        hi[i] = h
    return hi


def ref_block(R, hi, pos=None, D=None):
    """The definition, row by row, from a full symmetric R."""
    n = R.shape[0]
    out = np.zeros((n, n))
    for i in range(n):
        j = np.arange(i, hi[i] + 1)
        v = R[i, j]
        if pos is not None:
            v = v * (1.0 - (pos[j] - pos[i]) / D)
        out[i, j] = v
        out[j, i] = v
    return out


def bim(n, bp=None, cm=None, chrom=None):
    bp = np.arange(1, n + 1) if bp is None else bp
    cm = np.zeros(n) if cm is None else cm
    chrom = ["1"] * n if chrom is None else chrom
    return [(str(chrom[i]), "rs%d" % i, repr(float(cm[i])), str(int(bp[i])), "A", "G")
            for i in range(n)]


def fam(N):
    return bed_ref.bim_fam(1, N)[1]


def panel(tmp_path, codes, name="p", **kw):
    return read_bed(write_bed(str(tmp_path / name), codes, bim(codes.shape[0], **kw),
                              fam(codes.shape[1])))


# ---- reach -----------------------------------------------------------------------
def test_read_bed_keeps_the_bim_columns(tmp_path):
    codes = bed_ref.draw_codes(6, 16, seed=1)
    p = panel(tmp_path, codes, bp=[5, 5, 9, 20, 21, 40], cm=[0, .25, .25, 1.5, 2, 2.125],
              chrom=["1", "1", "1", "2", "2", "X"])
    assert p.ids == ["rs%d" % i for i in range(6)]
    assert p.chrom == ["1", "1", "1", "2", "2", "X"]
    np.testing.assert_array_equal(p.positions("bp"), [5, 5, 9, 20, 21, 40])
    np.testing.assert_array_equal(p.positions("cm", [5, 1]), [2.125, .25])
    from ldio import BedPanel
    old = BedPanel(p.prefix, p.rows, p.N, p.ids)          # the positional signature stays
    assert old.chrom is None and old.bp is None and old.M == 6
    with pytest.raises(ValueError, match="carries no base-pair positions"):
        old.positions("bp")


def test_reach_against_the_double_loop(tmp_path):
    n = 300
    codes = bed_ref.draw_codes(n, 16, seed=2)
    bp = clustered(n)
    rs = np.random.RandomState(4)
    cm = np.cumsum(rs.choice([0.0, 0.0, 0.001, 0.0625, 0.3, 1.7], n))   # ties, non-integers
    p = panel(tmp_path, codes, bp=bp, cm=cm)
    assert (np.diff(bp) == 0).any() and (np.diff(cm) == 0).any()
    cases = [dict(window_kb=4.0), dict(window_kb=0.4), dict(window_kb=40.0),
             dict(window_cm=0.3), dict(window_cm=2.0), dict(window_cm=0.0625),
             dict(window_kb=4.0, window=20), dict(window_cm=2.0, window=3),
             dict(window_kb=4.0, window=1000)]
    for kw in cases:
        L = BedLD(p, [n], **kw)
        pos = bp if "window_kb" in kw else cm
        D = 1000.0 * kw["window_kb"] if "window_kb" in kw else kw["window_cm"]
        ref = brute_hi(pos, D, kw.get("window"))
        hi = L.reach(0)
        assert hi.dtype == np.int32
        np.testing.assert_array_equal(hi, ref, err_msg=str(kw))
        assert (np.diff(hi) >= 0).all() and (hi >= np.arange(n)).all()
        assert L.band_width(0) == int(np.max(ref - np.arange(n)))
        assert L.by_reach and L.symmetric(0) and L.block_csr(0) is None
    # two blocks: the reach stays inside each
    L = BedLD(p, [120, 180], window_kb=4.0)
    np.testing.assert_array_equal(L.reach(1), brute_hi(bp[120:], 4000.0))
    np.testing.assert_array_equal(L.reach(0), brute_hi(bp[:120], 4000.0))


def test_reach_isolated_and_everything(tmp_path):
    n = 50
    codes = bed_ref.draw_codes(n, 16, seed=3)
    p = panel(tmp_path, codes, bp=1000 * np.arange(n), cm=0.5 * np.arange(n))
    iso = BedLD(p, [n], window_kb=0.5)            # every gap is 1,000 bp
    np.testing.assert_array_equal(iso.reach(0), np.arange(n))
    assert iso.band_width(0) == 0
    every = BedLD(p, [n], window_cm=1000.0)
    np.testing.assert_array_equal(every.reach(0), np.full(n, n - 1))
    assert every.band_width(0) == n - 1
    edge = BedLD(p, [n], window_kb=3.0)           # a distance of exactly D is inside
    np.testing.assert_array_equal(edge.reach(0), np.minimum(np.arange(n) + 3, n - 1))


def test_reach_predicate_is_the_subtraction_not_the_sum(tmp_path):
    """pos + D rounds where pos[j] - pos[i] does not: the first guess is fixed up."""
    cm = np.array([0.1, 0.3, 0.30000000000000004, 0.4, 0.7000000000000001, 0.8])
    codes = bed_ref.draw_codes(len(cm), 16, seed=4)
    p = panel(tmp_path, codes, cm=cm)
    for D in (0.2, 0.19999999999999998, 0.20000000000000004, 0.4, 0.6000000000000001, 0.1):
        np.testing.assert_array_equal(BedLD(p, [len(cm)], window_cm=D).reach(0), brute_hi(cm, D))


def test_marker_taper_positions_are_block_indices(tmp_path):
    codes = bed_ref.draw_codes(40, 16, seed=5)
    L = BedLD(panel(tmp_path, codes), [25, 15], window=6, taper="triangle")
    assert L.by_reach and L._span == 7.0
    np.testing.assert_array_equal(L.positions(1), np.arange(15.0))
    np.testing.assert_array_equal(L.reach(0), np.minimum(np.arange(25) + 6, 24))
    assert [L.band_width(b) for b in range(2)] == [6, 6]
    plain = BedLD(L.panel, [25, 15], window=6)            # a marker window alone: today's path
    assert not plain.by_reach and plain.taper is None and plain.band_width(0) == 6
    assert not BedLD(L.panel, [25, 15], window=6, taper="none").by_reach


# ---- values ----------------------------------------------------------------------
CASES = [dict(window_kb=4.0), dict(window_kb=40.0), dict(window_kb=4.0, window=30),
         dict(window_kb=4.0, taper="triangle"), dict(window_cm=1.5, taper="triangle"),
         dict(window=25, taper="triangle")]


@pytest.mark.parametrize("kw", CASES, ids=lambda kw: "-".join("%s=%s" % x for x in kw.items()))
def test_host_block_is_the_definition(tmp_path, kw):
    n = 260
    codes = bed_ref.draw_codes(n, 130, miss=0.03, seed=6)
    bp = clustered(n)
    cm = np.cumsum(np.random.RandomState(8).choice([0.0, 0.01, 0.125, 0.9], n))
    L = BedLD(panel(tmp_path, codes, bp=bp, cm=cm), [n], **kw)
    if "window_kb" in kw:
        pos, D = bp, 1000.0 * kw["window_kb"]
    elif "window_cm" in kw:
        pos, D = cm, kw["window_cm"]
    else:
        pos, D = np.arange(float(n)), kw["window"] + 1.0
    hi = brute_hi(pos, D, kw.get("window"))
    ref = ref_block(bed_ref.R(codes), hi, pos if kw.get("taper") else None, D)
    R = L.block(0)
    assert maxrel(R, ref) < TOL
    np.testing.assert_array_equal(R == 0.0, ref == 0.0)      # exact zeros outside, none lost inside
    np.testing.assert_array_equal(R, R.T)
    nobs = bed_ref.moments(codes)[0]
    assert np.max(np.abs(np.diag(R) - nobs / 130)) < 1e-12     # the diagonal's weight is 1


def test_an_entry_at_the_full_distance_is_an_explicit_zero(tmp_path):
    n = 12
    codes = bed_ref.draw_codes(n, 64, seed=7)
    L = BedLD(panel(tmp_path, codes, bp=1000 * np.arange(n)), [n], window_kb=3.0,
              taper="triangle")
    R = L.block(0)
    assert L.band_width(0) == 3
    assert not np.diag(R, 3).any() and np.diag(R, 2).all()    # kept, weight exactly 0


@functools.lru_cache(maxsize=None)
def cut_codes():
    codes = bed_ref.draw_codes(2500, 64, miss=0.03, seed=6)
    codes.setflags(write=False)
    return codes


@pytest.mark.parametrize("taper", [None, "triangle"])
def test_pieces_and_couplings_reassemble_the_block(tmp_path, taper):
    n = 2500
    codes, bp = cut_codes(), clustered(2500)
    L = BedLD(panel(tmp_path, codes, bp=bp), [n], window_kb=4.0, taper=taper)
    hi = L.reach(0)
    bw = L.band_width(0)
    assert bw == 132 and int(np.min(hi - np.arange(n))) == 0
    cuts = band_cuts([L], [n], piece=1024)
    assert cuts == [[1024, 1476]]
    P, cps = L.pieces(cuts)
    assert isinstance(P, BedLD) and P.block_sizes == [1024, 1476] and P.by_reach
    assert P.panel is L.panel and P.taper == taper
    # a piece's reach is the block's, cut at the piece's end; its width the widest inside
    np.testing.assert_array_equal(P.reach(0), np.minimum(hi[:1024], 1023))
    np.testing.assert_array_equal(P.reach(1), hi[1024:] - 1024)
    assert [P.band_width(b) for b in range(2)] == \
        [int(np.max(P.reach(b) - np.arange(len(P.reach(b))))) for b in range(2)]
    cp = cps[0]
    assert list(cps) == [0] and isinstance(cp, GenoCoupling) and (cp.nr, cp.nc) == (bw, bw)
    np.testing.assert_array_equal(cp.index, np.arange(1024 - bw, 1024 + bw))
    np.testing.assert_array_equal(cp.keep, np.clip(hi[1024 - bw:1024] - 1024 + 1, 0, bw))
    assert cp.keep[0] == 0 or bw == hi[1024 - bw] - (1024 - bw)
    assert (cp.pos is None) == (taper is None)
    if taper:
        np.testing.assert_array_equal(cp.pos, bp[1024 - bw:1024 + bw])
    R = L.block(0)
    ref = ref_block(bed_ref.R(codes), brute_hi(bp, 4000.0), bp if taper else None, 4000.0)
    assert maxrel(R, ref) < TOL
    np.testing.assert_array_equal(R == 0.0, ref == 0.0)
    A = np.zeros((n, n))
    A[:1024, :1024], A[1024:, 1024:] = P.block(0), P.block(1)
    C = cp.host()
    A[1024 - bw:1024, 1024:1024 + bw] = C
    A[1024:1024 + bw, 1024 - bw:1024] = C.T
    assert maxrel(A, R) < TOL
    np.testing.assert_array_equal(A == 0.0, R == 0.0)         # nothing else crosses the cut


def test_marker_taper_pieces_keep_the_block_indices(tmp_path):
    codes = bed_ref.draw_codes(70, 64, seed=8)
    L = BedLD(panel(tmp_path, codes), [70], window=30, taper="triangle")
    P, cps = L.pieces([[20, 25, 25]])
    assert [(cps[g].nr, cps[g].nc) for g in (0, 1)] == [(20, 25), (25, 25)]
    np.testing.assert_array_equal(cps[1].pos, np.arange(20.0, 70.0))
    np.testing.assert_array_equal(P.positions(2), np.arange(45.0, 70.0))
    R = L.block(0)
    assert maxrel(cps[0].host(), R[0:20, 20:45]) < TOL
    assert maxrel(cps[1].host(), R[20:45, 45:70]) < TOL
    np.testing.assert_array_equal(cps[1].host() == 0.0, R[20:45, 45:70] == 0.0)
    assert maxrel(P.block(1), R[20:45, 20:45]) < TOL


def test_select_and_regroup(tmp_path):
    codes = bed_ref.draw_codes(60, 130, miss=0.03, seed=9)
    bp = clustered(60)
    p = panel(tmp_path, codes, bp=bp)
    sel = np.sort(np.random.RandomState(1).permutation(60)[:48])
    L = BedLD(p, [20, 28], select=sel, window_kb=0.5, taper="triangle")
    for b, sl in enumerate((slice(0, 20), slice(20, 48))):
        pos = bp[sel[sl]]
        ref = ref_block(bed_ref.R(codes[sel[sl]]), brute_hi(pos, 500.0), pos, 500.0)
        assert maxrel(L.block(b), ref) < TOL
    assert L.regroup([20, 28]) is L
    G = L.regroup([48])
    assert type(G) is BlockLD
    np.testing.assert_array_equal(G.block(0)[:20, :20], L.block(0))
    assert not G.block(0)[:20, 20:].any()
    L2 = load_bed_ld(p.prefix, 0.0, blocks_file=None, block_size=48,
                     variants=["rs%d" % i for i in sel], window_kb=0.5)
    assert L2.block_sizes == [48] and L2.window_kb == 0.5 and L2.taper is None


# ---- refusals --------------------------------------------------------------------
def test_value_errors(tmp_path):
    n = 8
    codes = bed_ref.draw_codes(n, 16, seed=10)
    p = panel(tmp_path, codes, bp=[1, 2, 3, 10, 9, 12, 13, 14], cm=[0, 0, 0, 0, 1, 2, 3, 3])
    with pytest.raises(ValueError, match=r"LD block 0: the base-pair positions decrease from rs3 "
                                         r"\(10\.0\) to rs4 \(9\.0\)"):
        BedLD(p, [n], window_kb=1.0)
    with pytest.raises(ValueError, match=r"LD block 1: the base-pair positions decrease from rs3"):
        BedLD(p, [2, 6], window_kb=1.0)
    BedLD(p, [4, 4], window_kb=1.0)                     # positions restart at a block: fine
    with pytest.raises(ValueError, match=r"LD block 0: every marker has the cM position 0\.0.*"
                                         r"no genetic map"):
        BedLD(p, [4, 4], window_cm=1.0)
    ok = BedLD(p, [n], window_cm=1.0)                   # one block: the map is there
    assert ok.band_width(0) == 4
    for kw, msg in ((dict(taper="triangle"), "exactly one of the windows.*0 given"),
                    (dict(taper="triangle", window=3, window_cm=1.0), "exactly one.*2 given"),
                    (dict(window_kb=1.0, window_cm=1.0), "exclude each other"),
                    (dict(window_kb=0), "window in kb must be a positive number"),
                    (dict(window_cm=-1.0), "window in cM must be a positive number"),
                    (dict(window_cm="x"), "window in cM must be a positive number"),
                    (dict(window_kb=float("inf")), "window in kb must be a positive number"),
                    (dict(window=3, taper="cosine"), "taper must be one of none, triangle")):
        with pytest.raises(ValueError, match=msg):
            BedLD(p, [n], **kw)
    # a position that is not a number, found before anything is staged
    rows = bim(n)
    rows[5] = ("1", "rs5", "0", "NA", "A", "G")
    q = read_bed(write_bed(str(tmp_path / "q"), codes, rows, fam(16)))
    BedLD(q, [n], window=3)                             # untouched without a distance window
    with pytest.raises(ValueError, match=r"q\.bim: the base-pair position 'NA' of variant rs5 is "
                                         r"not a number"):
        BedLD(q, [n], window_kb=1.0)
    rows[5] = ("1", "rs5", "nan", "6", "A", "G")
    q = read_bed(write_bed(str(tmp_path / "q2"), codes, rows, fam(16)))
    with pytest.raises(ValueError, match=r"the cM position 'nan' of variant rs5 is not a number"):
        BedLD(q, [n], window_cm=1.0)
    with pytest.raises(ValueError, match="needs LD packing on"):
        ok.upload(None, 0, 0, packed=False)             # refused before the engine is touched
    with pytest.raises(ValueError, match="kept-column counts"):
        GenoCoupling(ok, 2, 2, [0, 1, 2, 3], keep=[1])
    with pytest.raises(ValueError, match="halo positions"):
        GenoCoupling(ok, 2, 2, [0, 1, 2, 3], keep=[1, 2], pos=[0.0, 1.0])


def test_marker_without_ld_in_a_halo_is_named(tmp_path):
    codes = np.array(bed_ref.draw_codes(70, 64, seed=11))
    codes[33] = 3
    L = BedLD(panel(tmp_path, codes, bp=100 * np.arange(70)), [70], window_kb=1.0,
              taper="triangle")
    _, cps = L.pieces([[30, 40]])
    assert (cps[0].nr, cps[0].nc) == (10, 10)
    with pytest.raises(ValueError, match=r"1 marker\(s\) of the coupling between LD band pieces 0 "
                                         r"and 1 have no LD.*rs33"):
        cps[0].host()


def test_parser_errors(tmp_path, capsys):
    import main

    base = ["--r-files", "r.npy", "--N", "10", "--M", "10", "--out-dir", str(tmp_path),
            "--out-name", "x"]
    bed = ["--ld-files", "p.bed", "--ld-block-size", "5"]
    npz = ["--ld-files", "R.npz"]
    for extra, msg in (
            (npz + ["--ld-window-kb", "5"], "--ld-window-kb applies to a .bed LD source only"),
            (npz + ["--ld-window-cm", "5"], "--ld-window-cm applies to a .bed LD source only"),
            (npz + ["--ld-taper", "triangle"], "--ld-taper applies to a .bed LD source only"),
            (npz + ["--ld-chr-blocks"], "--ld-chr-blocks applies to a .bed LD source only"),
            (bed + ["--ld-window-kb", "0"], "--ld-window-kb must be a positive number"),
            (bed + ["--ld-window-kb", "-2.5"], "--ld-window-kb must be a positive number"),
            (bed + ["--ld-window-cm", "wide"], "--ld-window-cm must be a positive number"),
            (bed + ["--ld-window-cm", "nan"], "--ld-window-cm must be a positive number"),
            (bed + ["--ld-window-kb", "5", "--ld-packing", "off"],
             "--ld-window-kb stores packed bands: it cannot be combined with --ld-packing off"),
            (bed + ["--ld-window-cm", "5", "--ld-packing", "off"],
             "--ld-window-cm stores packed bands: it cannot be combined with --ld-packing off"),
            (bed + ["--ld-window-kb", "5", "--ld-window-cm", "1"], "exclude each other"),
            (bed + ["--ld-taper", "triangle"], "--ld-taper needs exactly one of"),
            (bed + ["--ld-taper", "triangle", "--ld-window", "5", "--ld-window-kb", "5"],
             "--ld-taper needs exactly one of"),
            (bed + ["--ld-taper", "cosine", "--ld-window", "5"], "invalid choice"),
            (bed + ["--ld-chr-blocks"], "exclude each other: give exactly one"),
            (["--ld-files", "p.bed", "--ld-chr-blocks", "--ld-blocks", "f"],
             "exclude each other: give exactly one"),
            (["--ld-files", "p.bed", "--ld-window-kb", "5"], "needs its LD blocks")):
        with pytest.raises(SystemExit) as e:
            main.main(base + extra)
        assert e.value.code == 2
        assert msg in capsys.readouterr().err, extra


# ---- chromosome blocks -----------------------------------------------------------
def test_chromosome_blocks(tmp_path):
    n = 12
    codes = bed_ref.draw_codes(n, 16, seed=12)
    chrom = ["1"] * 5 + ["2"] * 3 + ["X"] * 4
    bp = [10, 20, 30, 40, 50, 5, 6, 7, 100, 200, 300, 400]        # restart at each chromosome
    p = panel(tmp_path, codes, bp=bp, chrom=chrom)
    assert chromosome_blocks(p) == [5, 3, 4]
    sel = np.array([0, 2, 4, 5, 8, 9, 11])
    assert chromosome_blocks(p, sel) == [3, 1, 3]
    assert chromosome_blocks(p, np.array([8, 0, 1, 9])) == [1, 2, 1]    # runs, in the run's order
    L = load_bed_ld(p.prefix, 0.0, chr_blocks=True, window_kb=0.015)
    assert L.block_sizes == [5, 3, 4]
    np.testing.assert_array_equal(L.reach(0), [1, 2, 3, 4, 4])
    np.testing.assert_array_equal(L.reach(1), [2, 2, 2])
    np.testing.assert_array_equal(L.reach(2), [0, 1, 2, 3])
    with pytest.raises(ValueError, match="positions decrease from rs4"):
        load_bed_ld(p.prefix, 0.0, block_size=n, window_kb=0.015)      # one block crosses them
    L = load_bed_ld(p.prefix, 0.0, chr_blocks=True, variants=["rs%d" % i for i in sel], window=2)
    assert L.block_sizes == [3, 1, 3]
    from ldio import BedPanel
    with pytest.raises(ValueError, match="no chromosome column"):
        chromosome_blocks(BedPanel(p.prefix, p.rows, p.N, p.ids))


# ---- why the taper: positive semi-definiteness ------------------------------------
def lam_min(A):
    return float(np.linalg.eigvalsh(A)[0])


@pytest.mark.parametrize("case", ["2500-W200", "700-W100", "700-D4000"])
def test_hard_window_is_indefinite_and_the_taper_is_psd(case):
    """Conditions on the inputs chosen here (recorded: -0.298 / +0.265, -0.650 /
    +0.153, -0.543 / +0.118): R = G G^T is PSD, its hard window is not, its Schur
    product with the triangular weight is."""
    if case == "2500-W200":
        codes = bed_ref.draw_codes(2500, 500, miss=0.03, seed=31)
        pos, D, W = np.arange(2500.0), 201.0, 200
    else:
        codes = bed_ref.draw_codes(700, 130, miss=0.03, seed=7)
        pos, D, W = (np.arange(700.0), 101.0, 100) if case == "700-W100" else \
            (clustered(700), 4000.0, None)
    n = len(pos)
    if W is None:
        hi = brute_hi(pos, D)
        assert int(np.min(hi - np.arange(n))) == 0 and int(np.max(hi - np.arange(n))) == 124
        assert (np.diff(pos) == 0).any()
    else:
        hi = np.minimum(np.arange(n) + W, n - 1)
    R = bed_ref.R(codes)
    hard, soft = lam_min(ref_block(R, hi)), lam_min(ref_block(R, hi, pos, D))
    print("%s: lambda_min hard %.3f, tapered %+.3f" % (case, hard, soft))
    assert hard < -0.1
    assert soft > 0.0
