"""score.py through the process seam: a 600-marker x 300-sample panel written with
ldio.write_bed, three effect files and a phenotype (reference score + noise);
then a target whose markers are dropped, swapped, mismatched and reordered
against --effects-bim; no phenotype; no matching variant."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest

from ldio import write_bed

from tests import bed_ref
from tests import score_ref as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORE = os.path.join(ROOT, "sgvamp-py_amd", "score.py")
M, N = 600, 300
ITS = (3, 7, 12)
DROP, SWAP, MISMATCH = 40, 30, 5
COLS = ["it", "m_used", "m_absent", "m_flipped", "m_allele_mismatch", "m_monomorphic", "n_pheno",
        "corr", "r2"]


def run(*argv):
    return subprocess.run([sys.executable, SCORE] + [str(a) for a in argv], capture_output=True,
                          text=True, timeout=120)


def read_csv(path):
    with open(path) as f:
        rows = list(csv.reader(f))
    assert rows[0] == COLS
    return [dict(zip(COLS, r)) for r in rows[1:]]


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("score_cli")
    rs = np.random.RandomState(41)
    codes = bed_ref._draw(rs, M, N, 0.02)
    codes[17] = 3                                    # monomorphic in the target
    codes[333] = 1                                   # unobserved
    bim, fam = bed_ref.bim_fam(M, N)
    write_bed(str(d / "target"), codes, bim, fam)
    beta = rs.normal(size=(3, M)) / np.sqrt(M)
    paths = []
    for k, it in enumerate(ITS):
        p = d / ("run_xhat_it_%d.bin" % it)
        beta[k].tofile(p)
        paths.append(str(p))
    X = sr.x_target(codes)
    ref = sr.scores(X, beta)
    y = np.asarray(ref[2], dtype=np.float64) + rs.normal(size=N) * 0.5
    y[[4, 77]] = np.nan
    with open(d / "pheno.txt", "w") as f:
        for s, (fid, iid) in enumerate((r[0], r[1]) for r in fam):
            f.write("%s %s %s\n" % (fid, iid, "NA" if np.isnan(y[s]) else repr(float(y[s]))))
    return dict(d=d, codes=codes, bim=bim, fam=fam, beta=beta, paths=paths, X=X, ref=ref, y=y)


def test_scores_files_and_statistics(data):
    d = data["d"]
    out = d / "o1" / "s"
    r = run("--bed", d / "target", "--effects", ",".join(data["paths"]), "--pheno", d / "pheno.txt",
            "--out", out)
    assert r.returncode == 0, r.stderr
    ids = [line.split() for line in open(str(out) + "_ids.txt")]
    assert ids == [[f[0], f[1]] for f in data["fam"]]
    rows = read_csv(str(out) + "_score.csv")
    assert [int(x["it"]) for x in rows] == list(ITS)
    bnd = sr.bound(data["X"], data["beta"])
    for k, it in enumerate(ITS):
        pgs = np.fromfile("%s_pgs_it_%d.bin" % (out, it))
        assert pgs.shape == (N,)
        assert np.all(np.abs(pgs.astype(np.longdouble) - data["ref"][k]) <= bnd[k])
        c, n = sr.pearson(pgs, data["y"])
        x = rows[k]
        assert (int(x["m_used"]), int(x["m_absent"]), int(x["m_flipped"]),
                int(x["m_allele_mismatch"]), int(x["m_monomorphic"])) == (M, 0, 0, 0, 2)
        assert int(x["n_pheno"]) == n == N - 2
        assert abs(float(x["corr"]) - c) <= 1e-12 and abs(float(x["r2"]) - c * c) <= 1e-12
        assert abs(float(x["corr"]) - np.corrcoef(pgs[np.isfinite(data["y"])],
                                                  data["y"][np.isfinite(data["y"])])[0, 1]) <= 1e-12
    assert float(rows[2]["r2"]) > 0.3                # the phenotype was built on the third score


def test_effect_file_without_iteration_and_npy(data):
    d = data["d"]
    p = d / "plain_bet.npy"
    np.save(p, data["beta"][1].reshape(-1, 1))
    out = d / "o2" / "s"
    r = run("--bed", d / "target", "--effects", "%s,%s" % (p, data["paths"][0]), "--out", out,
            "--standardise", "raw")
    assert r.returncode == 0, r.stderr
    Xr = sr.x_raw(data["codes"])
    b = data["beta"][[1, 0]]
    ref, bnd = sr.scores(Xr, b), sr.bound(Xr, b)
    for k, name in enumerate(("%s_pgs_0.bin" % out, "%s_pgs_it_%d.bin" % (out, ITS[0]))):
        pgs = np.fromfile(name)
        assert np.all(np.abs(pgs.astype(np.longdouble) - ref[k]) <= bnd[k])
    rows = read_csv(str(out) + "_score.csv")
    assert [x["it"] for x in rows] == ["0", str(ITS[0])]
    # no phenotype (.fam column 6 is -9 throughout): empty columns, exit status 0
    assert all(x["n_pheno"] == "0" and x["corr"] == "" and x["r2"] == "" for x in rows)


def test_reordered_target(data):
    """The effects stay in the order of the training .bim; the target drops 40 of
    its markers, has 30 recoded with A1 / A2 swapped and 5 with another allele
    pair, and lists its markers in another order."""
    d = data["d"]
    rs = np.random.RandomState(9)
    codes, bim = data["codes"], data["bim"]
    write_train = d / "train.bim"
    with open(write_train, "w") as f:
        for row in bim:
            f.write("\t".join(row) + "\n")
    pick = rs.permutation(M)
    dropped, swapped, mism = pick[:DROP], pick[DROP:DROP + SWAP], pick[DROP + SWAP:DROP + SWAP + MISMATCH]
    keep = rs.permutation(np.setdiff1d(np.arange(M), dropped))       # the target's own order
    tcodes = codes.copy()
    tbim = [list(r) for r in bim]
    for i in swapped:
        tcodes[i] = np.array([3, 1, 2, 0])[codes[i]]
        tbim[i][4], tbim[i][5] = bim[i][5], bim[i][4]
    for i in mism:
        tbim[i][4], tbim[i][5] = "C", "T"
    write_bed(str(d / "target2"), tcodes[keep], [tbim[i] for i in keep], data["fam"])
    out = d / "o3" / "s"
    r = run("--bed", d / "target2", "--effects", data["paths"][1], "--effects-bim", write_train,
            "--pheno", d / "pheno.txt", "--out", out)
    assert r.returncode == 0, r.stderr
    (x,) = read_csv(str(out) + "_score.csv")
    assert (int(x["m_absent"]), int(x["m_flipped"]), int(x["m_allele_mismatch"])) == (DROP, SWAP,
                                                                                      MISMATCH)
    assert int(x["m_used"]) == M - DROP - MISMATCH
    # the reference by the same rules, from the TARGET's codes
    use = np.setdiff1d(np.arange(M), np.concatenate([dropped, mism]))
    sign = np.ones(M)
    sign[swapped] = -1.0
    Xt = sr.x_target(tcodes[use])
    b = (data["beta"][1] * sign)[use][None, :]
    pgs = np.fromfile("%s_pgs_it_%d.bin" % (out, ITS[1]))
    assert np.all(np.abs(pgs.astype(np.longdouble) - sr.scores(Xt, b)[0]) <= sr.bound(Xt, b)[0])
    # swapping the coding and negating the effect is the same standardised score
    ok = ~np.isin(np.arange(M), np.concatenate([dropped, mism]))
    same = sr.scores(data["X"][ok], data["beta"][1][ok][None, :])[0]
    assert np.all(np.abs(pgs.astype(np.longdouble) - same) <= 2 * sr.bound(Xt, b)[0])
    c, n = sr.pearson(pgs, data["y"])
    assert int(x["n_pheno"]) == n and abs(float(x["corr"]) - c) <= 1e-12


def test_no_matching_variant(data):
    d = data["d"]
    other = d / "other.bim"
    with open(other, "w") as f:
        for i in range(M):
            f.write("1\tzz%d\t0\t%d\tA\tG\n" % (i, i + 1))
    r = run("--bed", d / "target", "--effects", data["paths"][0], "--effects-bim", other, "--out",
            d / "o4" / "s")
    assert r.returncode != 0
    assert "no variant" in r.stderr and "target" in r.stderr
    assert not os.path.exists(str(d / "o4" / "s") + "_score.csv")
    # and a length that does not fit the target without --effects-bim
    short = d / "short_xhat_it_1.bin"
    np.zeros(M - 1).tofile(short)
    r = run("--bed", d / "target", "--effects", short, "--out", d / "o4" / "s")
    assert r.returncode != 0 and "--effects-bim" in r.stderr
