"""bench.py's roofline bookkeeping (CPU): the PMC traffic attached to a bench
line must come from a summary of the same workload."""
import json
import os
import sys

import numpy as np

from tests.conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _summaries():
    out = {}
    for f in sorted(os.listdir(os.path.join(ROOT, "profiles"))):
        if "pmc" in f and f.endswith(".json"):
            out[f] = json.load(open(os.path.join(ROOT, "profiles", f)))
    return out


def test_traffic_matches_workload_bytes():
    sums = _summaries()
    assert sums, "no PMC summaries committed under profiles/"
    for name, d in sums.items():
        alg = d.get("algorithmic_bytes_per_launch")
        if not alg:
            continue
        kern = "k_sym_mfma" if "k_sym_mfma" in d["kernel"] else d["kernel"].split("<")[0]
        traffic, src = bench.read_traffic(kern, alg, d["K"], d["M"])
        assert src is not None
        got = sums[src]
        assert abs(got["algorithmic_bytes_per_launch"] - alg) <= 0.01 * alg
        assert (got["K"], got["M"]) == (d["K"], d["M"])
        assert traffic == got["hbm_bytes_per_launch"]


def test_traffic_none_for_unprofiled_workload():
    # the C2 pass bytes at ten times the size: no summary, so no traffic claimed
    assert bench.read_traffic("k_sym_pass", 2.0e11, 1, 200000) == (None, None)
    assert bench.read_traffic("k_no_such_kernel", 20210140245.0, 1, 200000) == (None, None)
    # C5 and the north star store the same LD (bytes within 0.2 %): K tells them apart
    src = bench.read_traffic("k_sym_mfma", 63779430912.0, 8, 1000000)[1]
    assert src.startswith("pmc_sym_mfma_") and src.endswith("_c5.json"), src
    src = bench.read_traffic("k_sym_mfma", 63651430912.0, 4, 1000000)[1]
    assert src.startswith("pmc_sym_mfma_") and src.endswith("_northstar.json"), src


def test_northstar_and_c2_summaries_present():
    sums = _summaries()
    kinds = {(d["kernel"].split("<")[0], round(d.get("algorithmic_bytes_per_launch") or 0, -9))
             for d in sums.values()}
    assert ("k_sym_pass", 2.0e10) in kinds          # C2, K = 1
    assert ("k_sym_mfma", 6.4e10) in kinds          # north star, M = 1e6, K = 4


def test_plain_run_is_the_default(monkeypatch):
    """The legs that take runs of their own (CPU baseline, read probe) are behind
    --full; --steps and --warmup set the loops' counts."""
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and (a.steps, a.warmup) == (7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"
    assert a.cpu_baseline == "auto" and a.read_bw == 1      # --full runs both by default


class _OneRank:
    def Get_size(self):
        return 1

    def Get_rank(self):
        return 0


class _Vectors:
    """get_vector of a stand-in engine: xhat1 and K cohorts' r1 of M markers."""

    def __init__(self, K, M):
        import hip_backend as hb

        rs = np.random.RandomState(5)
        self.K, self.M = K, M
        self.v = {(hb.VEC_XHAT1, 0): rs.normal(size=M)}
        for k in range(K):
            self.v[(hb.VEC_R1, k)] = rs.normal(size=M)

    def get_vector(self, which, k=0):
        return self.v[(which, k)].copy()


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    import hip_backend as hb

    K, M = 3, 5000
    eng = _Vectors(K, M)
    rec = dict(gamw=[1.0, 2.0, 3.0], gam1=[4.0, 5.0, 6.0], gam2=np.array([7.0, 8.0, 9.0]),
               alpha1=[0.1, 0.2, 0.3], alpha2=[0.4, 0.5, 0.6], lam=0.25,
               cg_iters=[[3, 4], [5, 6], [7, 8]])
    bench.dump_outputs(str(tmp_path / "a"), eng, _OneRank(), rec)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sorted(got) == ["cg_iters", "lam", "r1", "scalars", "xhat1"]
    assert all(a.dtype == np.float64 for a in got.values())
    np.testing.assert_array_equal(got["xhat1"], eng.v[(hb.VEC_XHAT1, 0)])
    np.testing.assert_array_equal(got["r1"], np.stack([eng.v[(hb.VEC_R1, k)] for k in range(K)]))
    assert got["scalars"].shape == (5, K) and got["scalars"][2].tolist() == [7.0, 8.0, 9.0]
    assert got["lam"].tolist() == [0.25] and got["cg_iters"].tolist() == rec["cg_iters"]
    # over the budget: the same seeded sample of the long arrays in every run
    whole = sum(a.nbytes for a in got.values())
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", whole // 2)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), eng, _OneRank(), rec)
    b = {f[:-4]: np.load(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")}
    assert sum(a.nbytes for a in b.values()) <= whole // 2 + 8 * 64
    assert b["r1"].ndim == 1 and b["r1"].size == int(K * M * ((whole // 2) / float(whole)))
    assert np.isin(b["r1"], got["r1"]).all() and b["scalars"].shape == (5, K)
    for n in b:
        np.testing.assert_array_equal(b[n], np.load(tmp_path / "c" / (n + ".npy")))


def test_workload_label_names_non_default_flags():
    """the bench line's workload names every reference CLI
    flag (src/main.py:27-50) it sets away from the CLI default, instead of
    claiming the defaults."""
    import argparse

    def args(**kw):
        d = dict(band=None, prior="matched", ridge=0.0, lmmse_damp=0)
        d.update(kw)
        return argparse.Namespace(**d)

    matched = dict(prior_vars=[0.0, 3.2e-6], prior_probs=[0.5, 0.5])
    lab = bench.flags_label(args(), matched)
    assert "--prior-vars 0,3.2e-06 --prior-probs 0.5,0.5" in lab and "except" in lab
    assert "default flags" not in lab
    lab = bench.flags_label(args(ridge=0.1, lmmse_damp=1), matched)
    assert "--s 0.1" in lab and "--lmmse-damp 1" in lab
    cli = dict(prior_vars=[0.0, 1.0], prior_probs=[0.99, 0.01])
    assert bench.flags_label(args(prior="cli"), cli) == \
        "reference CLI default flags (src/main.py:27-50)"
