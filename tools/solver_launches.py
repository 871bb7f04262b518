#!/usr/bin/env python3
"""The kernel launches of one VAMP step, in order: K = 2 cohorts on the mixed9
partition of tests/marker_ref.py, one outer iteration (EM prior loop, denoiser,
LMMSE with three CG iterations and gamw learning) through the library at --lib.
Run it under a kernel trace in a fresh process per library,

  rocprofv3 --kernel-trace -d DIR -o step --output-format csv -- \\
      python tools/solver_launches.py --lib sgvamp-py_amd/libsgvamp_hip.so

then --list DIR/.../step_kernel_trace.csv prints the kernel names in dispatch order:
two builds that enqueue the same launches print the same list
(profiles/solver_one/launches_*.txt)."""
import argparse
import csv
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sgvamp-py_amd"))
sys.path.insert(0, ROOT)


def listing(path):
    rows = list(csv.DictReader(open(path)))
    key = "Dispatch_Id" if rows and "Dispatch_Id" in rows[0] else "Start_Timestamp"
    rows.sort(key=lambda r: int(r[key]))   # the order they were enqueued in
    for r in rows:
        print(r["Kernel_Name"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--list", default=None, metavar="TRACE.csv")
    a = ap.parse_args()
    if a.list:
        return listing(a.list)
    import hip_backend
    hip_backend.load(a.lib, strict=False) if a.lib else hip_backend.load()
    from engine import Engine
    from sgvamp import VAMP
    from tests import marker_ref as mr

    sizes, K, N = mr.PARTS["mixed9"], 2, 250
    M = sum(sizes)
    rs = np.random.RandomState(9)
    beta = np.zeros(M)
    beta[rs.choice(M, M // 10, replace=False)] = rs.normal(0, 0.01, M // 10)
    eng = Engine(sizes, K=K)
    g = eng.synth_ld_g(0, 5, N, beta).sum(axis=0)
    for k in range(K):
        eng.synth_r(k, 5, N, g + np.random.RandomState(k).normal(0, 0.4, N))
    with tempfile.TemporaryDirectory() as d:
        v = VAMP(N=[float(N)] * K, Nt=float(N) * K, M=M, K=K, rho=0.5, gamw=5.0, gam1=1e-6,
                 a=[1.0 / K] * K, prior_vars=[0.0, 0.8 / (M // 10) / K], prior_probs=[0.9, 0.1],
                 out_dir=d, out_name="launches", seed=3, write_files=False)
        v.attach_engine(eng, x0=beta * np.sqrt(float(N)))
        v.infer(None, None, 1, x0=beta * np.sqrt(float(N)), cg_maxit=3, lmmse_damp=True,
                learn_gamw=True, prior_update="em", update_prior_from=0)
        print("cg iterations", [r["cg_iters"] for r in v.history])
    eng.close()


if __name__ == "__main__":
    main()
