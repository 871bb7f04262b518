"""PLINK .bed panels as an LD source, host side (no GPU): the file format, the
panel reader and writer, variant selection, BedLD's host evaluation against the
NumPy restatement (tests/bed_ref.py), the errors."""
import numpy as np
import pytest

from tests import bed_ref

import ldio
from ldio import BedLD, load_bed_ld, read_bed, write_bed


def _panel(tmp_path, codes, name="p", ids=None):
    M, N = codes.shape
    bim, fam = bed_ref.bim_fam(M, N)
    if ids is not None:
        bim = [(b[0], i) + b[2:] for b, i in zip(bim, ids)]
    return write_bed(str(tmp_path / name), codes, bim, fam)


def test_hand_decoded_bytes(tmp_path):
    """dc 0f, N = 6: dc = 11 01 11 00 -> samples 0..3 = 0, 3, 1, 3; 0f = 00 00 11 11
    -> samples 4, 5 = 3, 3 (and two padding positions reading 0)."""
    rows = np.array([[0xDC, 0x0F]], dtype=np.uint8)
    assert bed_ref.decode(rows, 6).tolist() == [[0, 3, 1, 3, 3, 3]]
    assert ldio.bed_codes(rows, 6).tolist() == [[0, 3, 1, 3, 3, 3]]
    x = ldio.BED_A1_COUNT[ldio.bed_codes(rows, 6)][0]
    assert x[[0, 1, 3, 4, 5]].tolist() == [2.0, 0.0, 0.0, 0.0, 0.0] and np.isnan(x[2])
    # the same row through a file: the padding bits are not samples
    p = tmp_path / "h"
    with open(str(p) + ".bed", "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x01, 0xDC, 0x0F]))
    with open(str(p) + ".bim", "w") as f:
        f.write("1\trs0\t0\t1\tA\tG\n")
    with open(str(p) + ".fam", "w") as f:
        f.writelines("f%d i%d 0 0 0 -9\n" % (s, s) for s in range(6))
    panel = read_bed(str(p))
    assert (panel.N, panel.M, panel.ids) == (6, 1, ["rs0"])
    L = BedLD(panel, [1])
    _, counts = L.standardised(0)
    assert counts.tolist() == [[1, 1, 0, 4]]      # 6 samples, not 8
    assert bed_ref.counts(bed_ref.decode(panel.rows, 6)).tolist() == [[1, 1, 0, 4]]


@pytest.mark.parametrize("N", [5, 6, 130, 1027])
def test_write_read_round_trip(tmp_path, N):
    rs = np.random.RandomState(N)
    codes = rs.randint(0, 4, size=(37, N))
    prefix = _panel(tmp_path, codes)
    for path in (prefix, prefix + ".bed"):
        panel = read_bed(path)
        assert panel.N == N and panel.M == 37 and panel.rows.shape == (37, (N + 3) // 4)
        assert panel.ids == ["rs%d" % i for i in range(37)]
        np.testing.assert_array_equal(bed_ref.decode(panel.rows, N), codes)
        np.testing.assert_array_equal(ldio.bed_codes(panel.rows, N), codes)
    np.testing.assert_array_equal(np.asarray(panel.rows), bed_ref.pack(codes))
    raw = open(prefix + ".bed", "rb").read()
    assert raw[:3] == b"\x6c\x1b\x01" and len(raw) == 3 + 37 * ((N + 3) // 4)


def test_rejects_bad_files(tmp_path):
    codes = np.random.RandomState(0).randint(0, 4, size=(9, 10))
    prefix = _panel(tmp_path, codes)
    raw = open(prefix + ".bed", "rb").read()

    def rewrite(data):
        with open(prefix + ".bed", "wb") as f:
            f.write(data)

    rewrite(b"\x6c\x1c" + raw[2:])
    with pytest.raises(ValueError, match="magic"):
        read_bed(prefix)
    rewrite(raw[:2] + b"\x00" + raw[3:])
    with pytest.raises(ValueError, match="sample-major"):
        read_bed(prefix)
    rewrite(raw + b"\x00")
    with pytest.raises(ValueError, match=r"expected 3 \+ 9 variants x 3 bytes = 30"):
        read_bed(prefix)
    rewrite(raw[:-1])
    with pytest.raises(ValueError, match="29 bytes"):
        read_bed(prefix)
    rewrite(raw)
    assert read_bed(prefix).M == 9
    with pytest.raises(ValueError):
        write_bed(str(tmp_path / "q"), codes + 3, *bed_ref.bim_fam(9, 10))
    with pytest.raises(ValueError):
        write_bed(str(tmp_path / "q"), codes, *bed_ref.bim_fam(8, 10))


def test_variant_selection_and_order(tmp_path):
    """Rows follow the merged .bim's order (sorted by coordinate over cohorts),
    matched on variant ids; the panel may hold more variants, in any order."""
    N, M = 64, 40
    codes = bed_ref.draw_codes(M, N, miss=0.03, seed=3)
    ids = ["rs%d" % i for i in range(M)]
    perm = np.random.RandomState(1).permutation(M)
    prefix = _panel(tmp_path, codes[perm], ids=[ids[i] for i in perm])
    # two cohorts' .bim files: coordinates give the merged order rs39 .. rs10
    want = [ids[i] for i in range(M - 1, 9, -1)]
    for k, part in enumerate((want[::-1], want[1::2])):   # cohort 0 holds them all, unsorted
        with open(tmp_path / ("c%d.bim" % k), "w") as f:
            for v in part:
                f.write("1\t%s\t0\t%d\tA\tG\n" % (v, 1000 - int(v[2:])))
    ref, _ = ldio.merge_bims([str(tmp_path / "c0.bim"), str(tmp_path / "c1.bim")])
    merged = list(ref["Variant"])
    assert merged == want
    L = load_bed_ld(prefix + ".bed", 0.0, block_size=12, variants=merged)
    assert L.block_sizes == [12, 12, 6] and L.M == 30
    sel = codes[[int(v[2:]) for v in merged]]
    o = 0
    for b, n in enumerate(L.block_sizes):
        np.testing.assert_array_equal(bed_ref.decode(L.rows(b), N), sel[o:o + n])
        assert L.variant_ids(b) == merged[o:o + n]
        o += n
    # the panel's own order without a selection
    L0 = load_bed_ld(prefix, 0.0, block_size=40)
    np.testing.assert_array_equal(bed_ref.decode(L0.rows(0), N), codes[perm])


def test_missing_variant_error(tmp_path):
    codes = bed_ref.draw_codes(10, 20, seed=1)
    prefix = _panel(tmp_path, codes)
    with pytest.raises(ValueError, match=r"3 of 5 variant\(s\) are absent.*rsX, rsY, rsZ"):
        load_bed_ld(prefix, 0.0, block_size=5, variants=["rs1", "rsX", "rs3", "rsY", "rsZ"])


def test_block_lists(tmp_path):
    codes = bed_ref.draw_codes(10, 20, seed=1)
    prefix = _panel(tmp_path, codes)
    (tmp_path / "sizes.txt").write_text("3\n5\n2\n")
    assert load_bed_ld(prefix, 0.0, blocks_file=str(tmp_path / "sizes.txt")).block_sizes == [3, 5, 2]
    (tmp_path / "bad.txt").write_text("3\n5\n")
    with pytest.raises(ValueError, match="8 markers in all, the LD has 10"):
        load_bed_ld(prefix, 0.0, blocks_file=str(tmp_path / "bad.txt"))
    assert ldio.equal_blocks(10, 4) == [4, 4, 2] and ldio.equal_blocks(8, 4) == [4, 4]


@pytest.mark.parametrize("N,miss", [(5, 0.0), (130, 0.03), (500, 0.0), (1027, 0.03)])
def test_bedld_block_matches_ref(tmp_path, N, miss):
    sizes = [50, 130, 77]
    codes = bed_ref.draw_codes(sum(sizes), N, miss=miss, seed=N)
    prefix = _panel(tmp_path, codes)
    L = BedLD(read_bed(prefix), sizes, s=0.25)
    assert L.s == 0.25 and L.M == sum(sizes)
    o = 0
    for b, n in enumerate(sizes):
        ref = bed_ref.R(codes[o:o + n])
        got = L.block(b)
        assert np.max(np.abs(got - ref)) / np.max(np.abs(ref)) < 1e-12
        nobs = bed_ref.moments(codes[o:o + n])[0]
        np.testing.assert_allclose(np.diag(got), nobs / N, rtol=0, atol=1e-12)
        assert L.block_csr(b) is None and L.band_width(b) is None
        o += n
    assert L.regroup(sizes) is L
    # a coarser partition: host-assembled blocks, block-diagonal inside
    C = L.regroup([180, 77])
    assert type(C).__name__ == "BlockLD" and C.block_sizes == [180, 77]
    B = C.block(0)
    assert np.array_equal(B[:50, :50], L.block(0)) and not B[:50, 50:].any()
    with pytest.raises(ValueError):
        L.regroup([100, 157])


def test_unusable_markers_raise(tmp_path):
    N = 40
    codes = bed_ref.draw_codes(30, N, miss=0.03, seed=5)
    codes[4] = 3                       # monomorphic
    codes[7] = 1                       # all missing
    codes[11, :] = 2
    codes[11, :3] = 1                  # one value among the observed samples
    for i in (20, 21, 22, 23):
        codes[i] = 0
    prefix = _panel(tmp_path, codes)
    L = BedLD(read_bed(prefix), [30])
    with pytest.raises(ValueError, match=r"7 marker\(s\) of LD block 0 have no LD.*"
                                         r"rs4, rs7, rs11, rs20, rs21, \.\.\."):
        L.block(0)
    assert bed_ref.unusable(codes).sum() == 7
    L2 = BedLD(read_bed(prefix), [4, 26])
    assert L2.block(0).shape == (4, 4)
    with pytest.raises(ValueError, match=r"7 marker\(s\) of LD block 1"):
        L2.block(1)


def test_parser_errors(tmp_path, capsys):
    import main

    base = ["--r-files", "r.npy", "--N", "10", "--M", "10", "--out-dir", str(tmp_path),
            "--out-name", "x"]
    for extra, msg in (
            (["--ld-files", "p.bed"], "needs its LD blocks"),
            (["--ld-files", "p.bed", "--ld-block-size", "5", "--ld-blocks", "s.txt"],
             "exclude each other"),
            (["--ld-files", "R.npy", "--ld-block-size", "5"], "apply to a .bed LD source only"),
            (["--ld-files", "p.bed", "--ld-block-size", "0"], "positive integer")):
        with pytest.raises(SystemExit) as e:
            main.main(base + extra)
        assert e.value.code == 2
        assert msg in capsys.readouterr().err
