#!/usr/bin/env python3
"""Distance-windowed genotype LD over N ranks on ONE GPU (host exchange, as
tools/geno_band_ranks_gpu.py): a 2,500-marker .bed panel whose .bim positions are
clustered (ties, gaps up to 400 bp) at --ld-window-kb 4 is one band of width 132,
cut into pieces [1024, 1476] (SGV_BAND_PIECE=1024); every rank reads only its own
piece's rows and the halo rows of the coupling it owns, and forms both on the
device from the reach.  Rank 0 then reruns on one rank and requires the stored
pieces and every xhat / r1 file to be bitwise identical.

  RANK=r WORLD_SIZE=2 MASTER_ADDR=127.0.0.1 MASTER_PORT=29533 SGV_EXCHANGE=host \
      SGV_BAND_PIECE=1024 python tools/geno_reach_ranks_gpu.py [f64|f32] [none|triangle]
Exit code 0 iff they are.  With the taper the solve runs at s = 0 (the tapered
band is positive semi-definite), without at s = 0.3."""
import hashlib
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

M, KB, PIECES = 2500, 4.0, [1024, 1476]
N, K, ITERS = 500, 2, 5


def positions():
    return np.cumsum(np.random.RandomState(3).choice([0, 1, 5, 50, 400], M, p=[.1, .3, .3, .2, .1]))


def run(comm, prefix, r, out, precision, taper):
    L = BedLD(read_bed(prefix), [M], window_kb=KB, taper=taper, s=0.0 if taper != "none" else 0.3)
    v = VAMP(N=[N] * K, Nt=N * K, M=M, K=K, rho=0.5, gamw=5.0, gam1=1e-6,
             a=np.full(K, 1.0 / K), prior_vars=[0.0, 1.0], prior_probs=[0.9, 0.1], out_dir=out,
             out_name="g", seed=7, comm=comm, device=0, ld_precision=precision)
    v.infer(L, np.stack([r] * K), ITERS, x0=None, cg_maxit=50, em_prior_maxit=20,
            prior_update="em")
    eng = v.engine
    sizes = list(eng.block_sizes)
    blocks = {b: hashlib.sha256(eng.get_ld_block(0, b).tobytes()).hexdigest()
              for b in range(eng.b0, eng.b1)}
    fmts = [eng.ld_block_format(0, b) for b in range(eng.b0, eng.b1)]
    owned = (eng.b0, eng.b1)
    comm.barrier()
    eng.close()
    return blocks, owned, sizes, fmts


def main():
    precision = sys.argv[1] if len(sys.argv) > 1 else "f64"
    taper = sys.argv[2] if len(sys.argv) > 2 else "none"
    comm = world_from_env()
    rank = comm.Get_rank()
    work = comm.bcast(tempfile.mkdtemp(prefix="geno_reach_ranks_") if rank == 0 else None)
    prefix = os.path.join(work, "p")
    codes = bed_ref.draw_codes(M, N, miss=0.03, seed=23)
    if rank == 0:
        bim = [("1", "rs%d" % i, "0", str(int(p)), "A", "G") for i, p in enumerate(positions())]
        write_bed(prefix, codes, bim, bed_ref.bim_fam(M, N)[1])
        os.mkdir(os.path.join(work, "many"))
        os.mkdir(os.path.join(work, "one"))
    comm.barrier()
    rs = np.random.RandomState(5)
    beta = np.zeros(M)
    beta[rs.choice(M, 100, replace=False)] = rs.normal(0, np.sqrt(0.8 / 100), 100)
    y = bed_ref.g(codes, beta) + rs.normal(0, np.sqrt(0.2), N)
    r = bed_ref.r(codes, y)
    blocks, owned, sizes, fmts = run(comm, prefix, r, os.path.join(work, "many"), precision, taper)
    parts = comm.allgather((blocks, owned, sizes, fmts))
    ok = True
    if rank == 0:
        merged = {}
        for bl, _, _, _ in parts:
            merged.update(bl)
        solo, _, solo_sizes, solo_fmts = run(SingleComm(), prefix, r, os.path.join(work, "one"),
                                             precision, taper)
        cut = all(p[2] == PIECES for p in parts) and solo_sizes == PIECES
        # one piece per rank: the coupling spans the two ranks
        spans = comm.Get_size() != 2 or [tuple(p[1]) for p in parts] == [(0, 1), (1, 2)]
        bands = all(f == 2 for p in parts for f in p[3]) and solo_fmts == [2, 2]
        same_blocks = merged == solo and len(solo) == len(PIECES)
        names = sorted(f for f in os.listdir(os.path.join(work, "one")) if f.endswith(".bin"))
        same_files = len(names) == ITERS * (K + 1)
        for fn in names:
            with open(os.path.join(work, "one", fn), "rb") as fa, \
                    open(os.path.join(work, "many", fn), "rb") as fb:
                same_files &= fa.read() == fb.read()
        x = np.fromfile(os.path.join(work, "one", "g_xhat_it_%d.bin" % (ITERS - 1)))
        ok = bool(cut and spans and bands and same_blocks and same_files
                  and np.isfinite(x).all() and x.any())
        print("[geno_reach_ranks] %s taper=%s ranks=%d pieces=%s owned=%s bands=%s blocks_equal=%s "
              "files_equal=%s (%d files) -> %s"
              % (precision, taper, comm.Get_size(), solo_sizes, [p[1] for p in parts], bands,
                 same_blocks, same_files, len(names), "bitwise equal -> OK" if ok else "FAIL"),
              flush=True)
    ok = comm.bcast(ok)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
