"""The posterior outputs through the process seam (main.py --posterior): the
files of one rank against the reference recomputed from the run's own r1 files,
cohort CSV and fixed prior; `last` and the default; two ranks byte-equal to one."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import posterior_ref as pr

pytestmark = pytest.mark.gpu

M, NSAMP, BLK, ITS = 2000, 1500, 250, 3
CAUSAL = 100
PRIOR_VAR = 0.8 / CAUSAL
PRIOR_PROBS = (0.95, 0.05)
GAM1_0 = 1e-6                      # the command line's default --gam1
THR = 0.9
BOUND = 1e-9                       # r1 went through a scale and back
KINDS = ("pip", "lodds", "postvar")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """K = 1, M = 2,000 in 8 LD blocks of 250, as tests/test_gpu_cli.py draws them."""
    import scipy.sparse

    d = tmp_path_factory.mktemp("posterior_cli")
    rs = np.random.RandomState(23)
    X = rs.normal(size=(NSAMP, M))
    for b in range(0, M, BLK):
        X[:, b + 1:b + BLK] += 0.6 * X[:, b:b + 1]
    X = (X - X.mean(0)) / X.std(0) / np.sqrt(NSAMP)
    C = X.T @ X
    mask = np.zeros((M, M), dtype=bool)
    for b in range(0, M, BLK):
        mask[b:b + BLK, b:b + BLK] = True
    scipy.sparse.save_npz(d / "R.npz", scipy.sparse.csr_matrix(np.where(mask, C, 0.0)))
    beta = np.zeros(M)
    beta[rs.choice(M, CAUSAL, replace=False)] = rs.normal(0, np.sqrt(PRIOR_VAR), CAUSAL)
    y = X @ beta * np.sqrt(NSAMP) + rs.normal(0, np.sqrt(0.2), NSAMP)
    np.save(d / "r.npy", X.T @ y)
    return d


def _argv(inputs, out, *extra):
    return ["--ld-files", str(inputs / "R.npz"), "--r-files", str(inputs / "r.npy"),
            "--out-dir", str(out), "--out-name", "t", "--N", str(NSAMP), "--M", str(M), "--K", "1",
            "--iterations", str(ITS), "--prior-vars", "0,%r" % PRIOR_VAR,
            "--prior-probs", "%r,%r" % PRIOR_PROBS, "--seed", "4", "--s", "0.02",
            "--prior-update", "none"] + list(extra)


def _run(inputs, name, *extra):
    import main

    out = inputs / name
    out.mkdir()
    main.main(_argv(inputs, out, *extra))
    return out


@pytest.fixture(scope="module")
def run_all(inputs):
    return _run(inputs, "all", "--posterior", "all", "--pip-threshold", str(THR))


def _csv(path):
    with open(path) as fh:
        lines = fh.read().splitlines()
    return lines[0].split("\t"), [ln.split("\t") for ln in lines[1:]]


def test_one_rank_files_match_the_reference(run_all):
    """Three files of M * 8 bytes per iteration; each equals the reference at that
    run's own r1 file (x sqrt(Nt)), the cohort CSV's gam1 (row it - 1; the initial
    value at 0) and the fixed prior, within 1e-9 on posterior_ref's scales;
    posterior.csv matches the sums of the files."""
    out = run_all
    Nt = float(NSAMP)
    _, cohort = _csv(out / "t_cohort_1.csv")
    head, rows = _csv(out / "t_posterior.csv")
    assert head == ["it", "sum_pip", "sum_postvar", "n_pip_ge_thr"]
    assert [int(r[0]) for r in rows] == list(range(ITS))
    for it in range(ITS):
        f = {k: out / ("t_%s_it_%d.bin" % (k, it)) for k in KINDS}
        for k in KINDS:
            assert os.path.getsize(f[k]) == M * 8, (k, it)
        pip, lodds, postvar = (np.fromfile(f[k]) for k in KINDS)
        r1 = np.fromfile(out / ("t_r1_cohort_1_it_%d.bin" % it)) * np.sqrt(Nt)
        gam1 = GAM1_0 if it == 0 else float(cohort[it - 1][2])
        ref = pr.reference(r1[None, :], [gam1], [1.0], 1.0 - PRIOR_PROBS[0], [1.0],
                           [PRIOR_VAR * Nt], thr=THR)
        e = (pr.dist_pip(pip, ref), pr.dist_lodds(lodds, ref), pr.dist_var(postvar * Nt, ref))
        print("it %d: pip %.3e lodds %.3e var %.3e" % ((it,) + e))
        assert max(e) <= BOUND, (it, e)
        assert np.isfinite(lodds).all() and (pip >= 0).all() and (pip <= 1).all()
        assert float(rows[it][1]) == pytest.approx(pip.sum(), rel=1e-12)
        assert float(rows[it][2]) == pytest.approx(postvar.sum(), rel=1e-12)
        assert int(rows[it][3]) == int((pip >= THR).sum())
    # the posterior moves between iterations, and it is not the xhat file's: xhat
    # is the damped mean
    assert not np.array_equal(np.fromfile(out / "t_pip_it_1.bin"), np.fromfile(out / "t_pip_it_2.bin"))


def test_last_and_default(inputs, run_all):
    """--posterior last writes only the last iteration's files (bytes of the `all`
    run's); the default writes no new file: its listing is that of a run with
    --posterior none, and every file of it is bytewise the `all` run's."""
    last = _run(inputs, "last", "--posterior", "last", "--pip-threshold", str(THR))
    new = sorted(f for f in os.listdir(last) if f.split("_")[1] in KINDS + ("posterior.csv",))
    assert new == sorted(["t_%s_it_%d.bin" % (k, ITS - 1) for k in KINDS] + ["t_posterior.csv"])
    for k in KINDS:
        name = "t_%s_it_%d.bin" % (k, ITS - 1)
        assert (last / name).read_bytes() == (run_all / name).read_bytes(), name
    head, rows = _csv(last / "t_posterior.csv")
    assert len(rows) == 1 and rows[0] == _csv(run_all / "t_posterior.csv")[1][ITS - 1]
    default = _run(inputs, "default")
    none = _run(inputs, "none", "--posterior", "none")
    assert sorted(os.listdir(default)) == sorted(os.listdir(none))
    assert len(os.listdir(default)) == 2 * ITS + 2      # xhat, r1 per iteration; two CSVs
    assert sorted(os.listdir(run_all)) == sorted(
        os.listdir(default) + ["t_%s_it_%d.bin" % (k, it) for k in KINDS for it in range(ITS)]
        + ["t_posterior.csv"])
    for f in os.listdir(default):
        assert (default / f).read_bytes() == (run_all / f).read_bytes(), f


def test_phases_path_writes_the_same_files(inputs, run_all, monkeypatch):
    """The one-host-call-per-phase step path (SGV_AB=1 SGV_STEP=phases), which calls
    Engine.posterior behind the denoiser: the same listing, every posterior file
    and the posterior CSV bytewise the chained sgv_step path's."""
    monkeypatch.setenv("SGV_AB", "1")
    monkeypatch.setenv("SGV_STEP", "phases")
    out = _run(inputs, "phases", "--posterior", "all", "--pip-threshold", str(THR))
    assert sorted(os.listdir(out)) == sorted(os.listdir(run_all))
    for f in os.listdir(out):
        if f.split("_")[1] in KINDS + ("posterior.csv",):
            assert (out / f).read_bytes() == (run_all / f).read_bytes(), f
    assert (out / "t_xhat_it_2.bin").read_bytes() == (run_all / "t_xhat_it_2.bin").read_bytes()


def test_two_ranks_byte_equal_one_rank(inputs, run_all):
    """The same run as `main.py --gpus 2` (LD blocks sharded; both ranks on device 0
    with the host exchange, as tests/test_gpu_cli.py launches it): every posterior
    .bin and the posterior CSV byte-equal to the one-rank run's, as every other
    output file."""
    two = inputs / "two"
    two.mkdir()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["SGV_EXCHANGE"] = "host"
    p = subprocess.run([sys.executable, os.path.join(root, "sgvamp-py_amd", "main.py")]
                       + _argv(inputs, two, "--posterior", "all", "--pip-threshold", str(THR))
                       + ["--gpus", "2", "--device", "0"], env=env, capture_output=True, text=True,
                       timeout=240)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    files = sorted(os.listdir(run_all))
    assert files == sorted(os.listdir(two))
    assert len([f for f in files if f.split("_")[1] in KINDS]) == 3 * ITS
    for f in files:
        assert (run_all / f).read_bytes() == (two / f).read_bytes(), f
