"""Windowed LD from .bed genotypes, host side (no GPU): BedLD(window=W)'s host
evaluation against the NumPy restatement (tests/bed_ref.R masked to |i - j| <= W,
the definition of include/sgvamp_hip.h, "windowed genotype LD"), its band width,
the band cut, the pieces and their couplings' halo rows, the marker order the
window counts in, and the command line's refusals."""
import numpy as np
import pytest

from tests import bed_ref

from ldio import BedLD, GenoCoupling, load_bed_ld, read_bed, write_bed
from sgvamp import BlockLD, band_cuts

TOL = 1e-12    # tests/test_gpu_geno_ld.py's bar for this contraction


def maxrel(a, b):
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


def masked(R, W):
    i = np.arange(R.shape[0])
    return np.where(np.abs(i[:, None] - i[None, :]) <= W, R, 0.0)


def _panel(tmp_path, codes, name="p"):
    return write_bed(str(tmp_path / name), codes, *bed_ref.bim_fam(*codes.shape))


@pytest.mark.parametrize("W", [1, 7, 64, 149, 155])
def test_host_block_is_the_masked_reference(tmp_path, W):
    codes = bed_ref.draw_codes(150, 130, miss=0.03, seed=3)
    L = BedLD(read_bed(_panel(tmp_path, codes)), [150], window=W)
    R, ref = L.block(0), masked(bed_ref.R(codes), W)
    assert maxrel(R, ref) < TOL
    np.testing.assert_array_equal(R == 0.0, ref == 0.0)       # exact zeros outside, none lost inside
    np.testing.assert_array_equal(R, R.T)
    assert L.symmetric(0) and L.block_csr(0) is None


def test_two_blocks_window_stays_inside_each(tmp_path):
    codes = bed_ref.draw_codes(90, 64, seed=4)
    L = load_bed_ld(_panel(tmp_path, codes), 0.0, block_size=50, window=5)
    assert L.block_sizes == [50, 40] and L.window == 5
    for b, sl in enumerate((slice(0, 50), slice(50, 90))):
        assert maxrel(L.block(b), masked(bed_ref.R(codes[sl]), 5)) < TOL


def test_band_width(tmp_path):
    n = 40
    codes = bed_ref.draw_codes(n, 64, seed=5)
    panel = read_bed(_panel(tmp_path, codes))
    for W, bw in ((1, 1), (64, n - 1), (n - 1, n - 1), (n + 5, n - 1), (20, 20)):
        assert BedLD(panel, [n], window=W).band_width(0) == bw
    L = BedLD(panel, [30, 10], window=12)
    assert [L.band_width(b) for b in range(2)] == [12, 9]
    plain = BedLD(panel, [n])                                  # no window: a dense source, as before
    assert plain.window is None and plain.band_width(0) is None and not plain.symmetric(0)
    for bad in (0, -3, 2.5, "x"):
        with pytest.raises(ValueError, match="positive number of markers"):
            BedLD(panel, [n], window=bad)


@pytest.fixture(scope="module")
def cut_case(tmp_path_factory):
    """n = 2,500, W = 200: the panel, the windowed source and its uncut host block."""
    n, N, W = 2500, 64, 200
    codes = bed_ref.draw_codes(n, N, miss=0.03, seed=6)
    d = tmp_path_factory.mktemp("cut")
    L = BedLD(read_bed(_panel(d, codes)), [n], window=W)
    R = L.block(0)
    R.setflags(write=False)
    return codes, L, R, W


def test_band_cut_and_pieces(cut_case):
    codes, L, R, W = cut_case
    n = codes.shape[0]
    cuts = band_cuts([L], [n], piece=1024)
    assert cuts == [[1024, 1476]]
    assert band_cuts([L], [n], piece=0) == [[n]]
    P, cps = L.pieces(cuts)
    assert isinstance(P, BedLD) and P.block_sizes == [1024, 1476] and P.window == W
    assert P.panel is L.panel and [P.band_width(b) for b in range(2)] == [W, W]
    assert list(cps) == [0] and isinstance(cps[0], GenoCoupling)
    cp = cps[0]
    assert (cp.nr, cp.nc) == (200, 200)
    np.testing.assert_array_equal(cp.index, np.arange(1024 - 200, 1024 + 200))
    np.testing.assert_array_equal(cp.rows(), bed_ref.pack(codes[824:1224]))
    # the pieces are the diagonal blocks of the uncut matrix, the coupling its corner
    np.testing.assert_array_equal(P.rows(1), bed_ref.pack(codes[1024:]))
    C = cp.host()
    assert C.shape == (200, 200)
    assert maxrel(C, R[824:1024, 1024:1224]) < TOL
    np.testing.assert_array_equal(C == 0.0, R[824:1024, 1024:1224] == 0.0)
    assert maxrel(P.block(0), R[:1024, :1024]) < TOL
    assert not R[:824, 1024:].any() and not R[:1024, 1224:].any()   # nothing else crosses the cut
    # the same partition: the object itself, no couplings
    same, none = L.pieces([[n]])
    assert same is L and none == {}
    with pytest.raises(ValueError, match="without a window"):
        BedLD(L.panel, [n]).pieces(cuts)


def test_short_pieces_clip_the_coupling(tmp_path):
    """A piece shorter than the window: nr / nc are the piece lengths."""
    codes = bed_ref.draw_codes(70, 64, seed=8)
    L = BedLD(read_bed(_panel(tmp_path, codes)), [70], window=30)
    P, cps = L.pieces([[20, 25, 25]])
    assert P.block_sizes == [20, 25, 25]
    assert [(cps[g].nr, cps[g].nc) for g in (0, 1)] == [(20, 25), (25, 25)]
    R = L.block(0)
    assert maxrel(cps[0].host(), R[0:20, 20:45]) < TOL
    assert maxrel(cps[1].host(), R[20:45, 45:70]) < TOL


def test_select_applies_the_window_in_the_merged_order(tmp_path):
    codes = bed_ref.draw_codes(60, 130, miss=0.03, seed=9)
    panel = read_bed(_panel(tmp_path, codes))
    perm = np.random.RandomState(1).permutation(60)[:48]
    L = BedLD(panel, [48], select=perm, window=6)
    assert maxrel(L.block(0), masked(bed_ref.R(codes[perm]), 6)) < TOL
    P, cps = L.pieces([[24, 24]])
    np.testing.assert_array_equal(cps[0].index, perm[18:30])
    assert cps[0].variant_ids() == ["rs%d" % i for i in perm[18:30]]
    np.testing.assert_array_equal(P.rows(1), bed_ref.pack(codes[perm[24:]]))
    ids = ["rs%d" % i for i in perm]
    L2 = load_bed_ld(panel.prefix, 0.0, block_size=48, variants=ids, window=6)
    np.testing.assert_array_equal(L2.block(0), L.block(0))


def test_regroup(tmp_path):
    codes = bed_ref.draw_codes(60, 64, seed=10)
    L = BedLD(read_bed(_panel(tmp_path, codes)), [25, 35], window=4)
    assert L.regroup([25, 35]) is L
    G = L.regroup([60])
    assert type(G) is BlockLD and G.band_width(0) is None
    ref = np.zeros((60, 60))
    ref[:25, :25] = masked(bed_ref.R(codes[:25]), 4)
    ref[25:, 25:] = masked(bed_ref.R(codes[25:]), 4)
    assert maxrel(G.block(0), ref) < TOL
    np.testing.assert_array_equal(G.block(0) == 0.0, ref == 0.0)


def test_regroup_is_subject_to_the_dense_guard(tmp_path, monkeypatch):
    import sgvamp

    codes = bed_ref.draw_codes(60, 64, seed=10)
    L = BedLD(read_bed(_panel(tmp_path, codes)), [25, 35], window=4)
    monkeypatch.setattr(sgvamp, "DENSE_BLOCK_LIMIT", 8 * 59 * 59)
    with pytest.raises(ValueError, match="dense-block limit"):
        L.regroup([60]).block(0)


def test_marker_without_ld_in_a_halo_is_named(tmp_path):
    codes = np.array(bed_ref.draw_codes(70, 64, seed=11))
    codes[33] = 3
    L = BedLD(read_bed(_panel(tmp_path, codes)), [70], window=10)
    _, cps = L.pieces([[30, 40]])
    with pytest.raises(ValueError, match=r"1 marker\(s\) of the coupling between LD band pieces 0 "
                                         r"and 1 have no LD.*rs33"):
        cps[0].host()


def test_upload_refuses_packing_off(tmp_path):
    codes = bed_ref.draw_codes(20, 64, seed=12)
    L = BedLD(read_bed(_panel(tmp_path, codes)), [20], window=3)
    with pytest.raises(ValueError, match="needs LD packing on"):
        L.upload(None, 0, 0, packed=False)        # refused before the engine is touched


def test_parser_errors(tmp_path, capsys):
    import main

    base = ["--r-files", "r.npy", "--N", "10", "--M", "10", "--out-dir", str(tmp_path),
            "--out-name", "x"]
    bed = ["--ld-files", "p.bed", "--ld-block-size", "5"]
    for extra, msg in (
            (["--ld-files", "R.npz", "--ld-window", "5"], "--ld-window applies to a .bed LD source only"),
            (bed + ["--ld-window", "0"], "--ld-window must be a positive integer"),
            (bed + ["--ld-window", "-4"], "--ld-window must be a positive integer"),
            (bed + ["--ld-window", "2.5"], "--ld-window must be a positive integer"),
            (bed + ["--ld-window", "wide"], "--ld-window must be a positive integer"),
            (bed + ["--ld-window", "5", "--ld-packing", "off"], "cannot be combined with --ld-packing off"),
            (["--ld-files", "p.bed", "--ld-window", "5"], "needs its LD blocks")):
        with pytest.raises(SystemExit) as e:
            main.main(base + extra)
        assert e.value.code == 2
        assert msg in capsys.readouterr().err
