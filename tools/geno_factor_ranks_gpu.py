#!/usr/bin/env python3
"""The factor LD form over N ranks on ONE GPU (host exchange, as
tools/geno_ranks_gpu.py): every rank stages only its own blocks' rows of a .bed
panel and hands them over as factor blocks; rank 0 then reruns on one rank and
requires every output file (xhat, r1, the csv files) to be bitwise identical.
The solve runs the pipelined CG, both CG solves of an iteration and the gamw
pass, 4 iterations.

  RANK=r WORLD_SIZE=2 MASTER_ADDR=127.0.0.1 MASTER_PORT=29533 SGV_EXCHANGE=host \
      python tools/geno_factor_ranks_gpu.py
Exit code 0 iff they are."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sgvamp-py_amd"))

from comm import SingleComm, world_from_env  # noqa: E402
from ldio import BedLD, read_bed, write_bed  # noqa: E402
from sgvamp import VAMP  # noqa: E402
from tests import bed_ref  # noqa: E402

SIZES = [50, 130, 257, 700, 1100]   # 1100: two slabs of the first product
N, K, ITERS = 500, 2, 4


def run(comm, prefix, r, out):
    L = BedLD(read_bed(prefix), SIZES, form="factor")
    v = VAMP(N=[N] * K, Nt=N * K, M=sum(SIZES), K=K, rho=0.5, gamw=5.0, gam1=1e-6,
             a=np.full(K, 1.0 / K), prior_vars=[0.0, 1.0], prior_probs=[0.9, 0.1], out_dir=out,
             out_name="g", seed=7, comm=comm, device=0)
    v.infer(L, np.stack([r] * K), ITERS, x0=None, cg_maxit=50, em_prior_maxit=20,
            prior_update="em", learn_gamw=True)
    eng = v.engine
    fmts = [eng.ld_block_format(0, b) for b in range(eng.b0, eng.b1)]
    kind = eng.ld_pass_form(0, 2 * K).kind
    cg = [rec["cg_iters"] for rec in v.history if "cg_iters" in rec]
    owned = (eng.b0, eng.b1)
    comm.barrier()
    eng.close()
    return fmts, kind, cg, owned


def main():
    comm = world_from_env()
    rank = comm.Get_rank()
    M = sum(SIZES)
    work = comm.bcast(tempfile.mkdtemp(prefix="geno_factor_ranks_") if rank == 0 else None)
    prefix = os.path.join(work, "p")
    codes = bed_ref.draw_codes(M, N, miss=0.03, seed=21)
    if rank == 0:
        write_bed(prefix, codes, *bed_ref.bim_fam(M, N))
        os.mkdir(os.path.join(work, "many"))
        os.mkdir(os.path.join(work, "one"))
    comm.barrier()
    rs = np.random.RandomState(5)
    beta = np.zeros(M)
    beta[rs.choice(M, 60, replace=False)] = rs.normal(0, np.sqrt(0.8 / 60), 60)
    y = bed_ref.g(codes, beta) + rs.normal(0, np.sqrt(0.2), N)
    r = bed_ref.r(codes, y)
    fmts, kind, cg, owned = run(comm, prefix, r, os.path.join(work, "many"))
    parts = comm.allgather((fmts, kind, owned))
    ok = True
    if rank == 0:
        solo_fmts, solo_kind, solo_cg, _ = run(SingleComm(), prefix, r, os.path.join(work, "one"))
        factor = all(f == 3 for p in parts for f in p[0]) and all(p[1] == "factor" for p in parts) \
            and solo_fmts == [3] * len(SIZES) and solo_kind == "factor"
        names = sorted(os.listdir(os.path.join(work, "one")))
        same_files = names == sorted(os.listdir(os.path.join(work, "many"))) \
            and sum(f.endswith(".bin") for f in names) == ITERS * (K + 1)
        for fn in names:
            with open(os.path.join(work, "one", fn), "rb") as fa, \
                    open(os.path.join(work, "many", fn), "rb") as fb:
                same_files &= fa.read() == fb.read()
        x = np.fromfile(os.path.join(work, "one", "g_xhat_it_%d.bin" % (ITERS - 1)))
        iterated = len(solo_cg) >= 3 and solo_cg == cg
        ok = bool(factor and same_files and iterated and np.isfinite(x).all() and x.any())
        print("[geno_factor_ranks] ranks=%d owned=%s factor=%s files_equal=%s (%d files) cg=%s -> %s"
              % (comm.Get_size(), [p[2] for p in parts], factor, same_files, len(names), solo_cg,
                 "bitwise equal -> OK" if ok else "FAIL"), flush=True)
    ok = comm.bcast(ok)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
