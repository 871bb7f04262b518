"""Host side of score.py (no device): effect-file readers, variant matching and
the allele rules, phenotype parsing, the chunk-length rule, the statistics."""
import math

import numpy as np
import pytest

import score

from tests import score_ref as sr


def test_effect_readers(tmp_path):
    b = np.random.RandomState(0).normal(size=37)
    pb, p1, p2 = (str(tmp_path / n) for n in ("x_xhat_it_12.bin", "a_bet.npy", "b.npy"))
    b.tofile(pb)
    np.save(p1, b.reshape(-1, 1))
    np.save(p2, b.astype(np.float32))
    assert np.array_equal(score.read_effects(pb), b)
    assert np.array_equal(score.read_effects(pb, 37), b)
    assert np.array_equal(score.read_effects(p1, 37), b)
    got = score.read_effects(p2)
    assert got.dtype == np.float64 and np.array_equal(got, b.astype(np.float32).astype(np.float64))
    for p in (pb, p1, p2):
        with pytest.raises(ValueError, match="expected 36"):
            score.read_effects(p, 36)
    bad = str(tmp_path / "m.npy")
    np.save(bad, np.zeros((4, 2)))
    with pytest.raises(ValueError, match="shape"):
        score.read_effects(bad)
    odd = str(tmp_path / "odd.bin")
    open(odd, "wb").write(b"\0" * 13)
    with pytest.raises(ValueError, match="whole number"):
        score.read_effects(odd)
    assert score.effect_iteration(pb) == 12
    assert score.effect_iteration(p1) is None
    assert score.effect_iteration("/x/run_it_3/name_xhat_it_50.bin") == 50
    assert score.parse_iterations("1-3,7,10-11") == [1, 2, 3, 7, 10, 11]


def test_match_variants_and_alleles():
    eff = ["rs%d" % i for i in range(8)]
    e1, e2 = ["A"] * 8, ["G"] * 8
    tgt = ["rs5", "rs0", "rsX", "rs3", "rs2", "rs7", "rs6"]          # rs1, rs4 absent
    t1 = ["A", "a", "C", "G", "A", "T", "G"]
    t2 = ["G", "g", "T", "A", "C", "C", "a"]
    m = score.match_variants(eff, e1, e2, tgt, t1, t2)
    #                           rs0 rs1 rs2 rs3 rs4 rs5 rs6 rs7
    assert m["row"].tolist() == [1, -1, -1, 3, -1, 0, 6, -1]
    assert m["sign"].tolist() == [1, 0, 0, -1, 0, 1, -1, 0]
    assert (m["m_used"], m["m_absent"], m["m_flipped"], m["m_allele_mismatch"]) == (4, 2, 2, 2)
    # without alleles on either side nothing is checked
    for args in ((eff, None, None, tgt, t1, t2), (eff, e1, e2, tgt, None, None)):
        m = score.match_variants(*args)
        assert m["row"].tolist() == [1, -1, 4, 3, -1, 0, 6, 5]
        assert m["sign"].tolist() == [1, 0, 1, 1, 0, 1, 1, 1]
        assert (m["m_used"], m["m_absent"], m["m_flipped"], m["m_allele_mismatch"]) == (6, 2, 0, 0)
    with pytest.raises(ValueError, match="no variant"):
        score.match_variants(["a", "b"], None, None, ["c"], None, None)
    with pytest.raises(ValueError, match="no variant"):
        score.match_variants(["a"], ["A"], ["G"], ["a"], ["A"], ["C"])


def test_bim_readers(tmp_path):
    p = str(tmp_path / "t.bim")
    open(p, "w").write("1 rs1 0 10 A G\n1 rs2 0 20 C T\n\n")
    assert score.read_bim(p) == (["rs1", "rs2"], ["A", "C"], ["G", "T"])
    q = str(tmp_path / "short.bim")
    open(q, "w").write("1 rs1 0 10\n1 rs2 0 20\n")
    assert score.read_bim(q) == (["rs1", "rs2"], None, None)
    assert score.merged_bim([p]) == score.read_bim(p)


def test_merged_bim_order(tmp_path):
    a, b = str(tmp_path / "a.bim"), str(tmp_path / "b.bim")
    open(a, "w").write("1 rs1 0 10 A G\n1 rs3 0 30 C T\n")
    open(b, "w").write("1 rs2 0 20 G C\n1 rs3 0 30 T C\n")
    ids, a1, a2 = score.merged_bim([a, b])
    from ldio import merge_bims

    assert ids == [str(v) for v in merge_bims([a, b])[0]["Variant"]]
    assert sorted(ids) == ["rs1", "rs2", "rs3"]
    al = dict(zip(ids, zip(a1, a2)))
    assert al == {"rs1": ("A", "G"), "rs2": ("G", "C"), "rs3": ("C", "T")}


def test_phenotypes(tmp_path):
    fam = str(tmp_path / "t.fam")
    open(fam, "w").write("f0 i0 0 0 1 1.5\nf1 i1 0 0 2 -9\nf2 i2 0 0 0 NA\nf3 i3 0 0 0 nan\n"
                         "f4 i4 0 0 0 -2e-1\nf5 i5\n")
    ids, ph = score.read_fam(fam)
    assert ids == [("f%d" % i, "i%d" % i) for i in range(6)]
    assert ph[0] == 1.5 and ph[4] == -0.2 and np.isnan(ph[[1, 2, 3, 5]]).all()
    p = str(tmp_path / "p.txt")
    open(p, "w").write("FID IID y\nf4 i4 3.25\nf0 i0 -9\nf1 i1 Na\nf2 i2 7\nzz zz 1\nf3 i3 inf\n")
    got = score.read_pheno(p, ids)
    assert got[4] == 3.25 and got[2] == 7.0 and np.isnan(got[[0, 1, 3, 5]]).all()
    open(p, "w").write("f4 i4\n")
    with pytest.raises(ValueError, match="FID IID value"):
        score.read_pheno(p, ids)
    for t in ("-9", "NA", "na", "NaN", "nan", " -9 ", "x"):
        assert math.isnan(score.parse_value(t))
    assert score.parse_value("-9.0") == -9.0 and score.parse_value("0") == 0.0


@pytest.mark.parametrize("N", [1, 5, 300, 2000, 10000, 50000, 487409, 3000000])
def test_chunk_rule(N):
    m = score.chunk_markers(N)
    assert m >= 1024 and m % 1024 == 0
    slabs = m // 1024
    part = slabs * N * 16 * 8
    assert part <= 256 << 20 or slabs == 1          # one slab at least, whatever N
    assert (slabs + 1) * N * 16 * 8 > 256 << 20      # and no shorter than it has to be
    assert score.chunk_markers(N, cap_bytes=N * 128 * 3) == 3 * 1024


def test_corr_r2():
    rs = np.random.RandomState(1)
    x = rs.normal(size=200)
    y = 0.4 * x + rs.normal(size=200)
    y[[3, 50, 199]] = np.nan
    n, c, r2 = score.corr_r2(x, y)
    ok = ~np.isnan(y)
    want = np.corrcoef(x[ok], y[ok])[0, 1]
    assert n == 197 and abs(c - want) < 1e-12 and abs(r2 - want * want) < 1e-12
    assert (c, n) == sr.pearson(x, y)
    with np.errstate(all="raise"):                   # a constant side: nan, no crash, no warning
        n, c, r2 = score.corr_r2(x, np.full(200, 2.5))
        assert n == 200 and math.isnan(c) and math.isnan(r2)
        n, c, r2 = score.corr_r2(np.zeros(200), y)
        assert n == 197 and math.isnan(c) and math.isnan(r2)
        assert score.corr_r2(x, np.full(200, np.nan)) [0] == 0
        n, c, r2 = score.corr_r2(x[:1], y[:1])
        assert n == 1 and math.isnan(c)
    assert score.fmt(float("nan")) == "" and score.fmt(0.5) == "0.5"
