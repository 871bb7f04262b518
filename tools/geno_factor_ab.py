#!/usr/bin/env python3
"""LD pass time of the factor form (sgv_geno_ld_factor: G (G^T p) from the 2-bit
rows) against the stored f64 packed form (sgv_geno_ld) on the SAME panel, on one
device, at 1, 2, 4, 8 and 16 columns; also the memory each form holds and the
time to build it.  One shape per call:

  north   8 blocks of 15,625 markers, N = 10,000 (the north star's block)
  n500    the same blocks at N = 500
  chrom   one unwindowed block of 131,072 markers, N = 2,000 -- the stored form
          cannot hold it (68.7 GB packed), so the factor arm only

  timeout -k 10 600 python tools/geno_factor_ab.py --shape north --out profiles/geno_factor/ldpass_ab.jsonl && \
  timeout -k 10 300 python tools/geno_factor_ab.py --shape n500 --out profiles/geno_factor/ldpass_ab.jsonl && \
  timeout -k 10 300 python tools/geno_factor_ab.py --shape chrom --out profiles/geno_factor/ldpass_ab.jsonl

(each step under its own time limit, chained, so a fault ends the sequence; a
call appends its lines).  Pass time is the library's own: HIP events around every
LD pass on the context's stream (sgv_timers), over windows of --inner passes
after a warm-up of each arm at each column count, the arms alternating within a
column count, --reps windows each.  One JSON line per window, one summary line
per column count (medians, the factor / stored ratio, the factor form's f64 rate
from 4 N n_b nc flops per block), one line for memory and build time.  The panel
is one block's rows drawn at allele frequencies in [0.05, 0.5] with 1 % missing
and used for every block: both arms read the same rows.  Needs a GPU; there is
no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sgvamp-py_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from engine import Engine  # noqa: E402
from geno_ld_ab import draw_rows, free_bytes  # noqa: E402

SHAPES = {"north": (8, 15625, 10000, True), "n500": (8, 15625, 500, True),
          "chrom": (1, 131072, 2000, False)}
GF_SLAB = 1024                 # csrc/common.h
GF_SCRATCH_MAX = 32 << 20      # csrc/ldplan.hip: doubles per launch at 16 columns


def scratch_bytes(nblk, n, N):
    """The factor form's scratch as ensure_plan sizes it: t and the slab partials of
    the blocks of the largest launch, 16 columns."""
    per = (-(-n // GF_SLAB) + 1) * N * 16            # doubles per block
    fit = max(1, min(nblk, GF_SCRATCH_MAX // per))
    return 8 * per * fit


def window(eng, V, inner):
    eng.timers(reset=True)
    for _ in range(inner):
        eng.ld_matvec(0, V)
    t = eng.timers()
    assert t["ld_launches"] == inner
    return t["ld_ms"] / inner, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--shape", choices=sorted(SHAPES), required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--cols", default="1,2,4,8,16")
    a = ap.parse_args()
    nblk, n, N, both = SHAPES[a.shape]
    base = draw_rows(min(n, 4096), N, 1)
    rows = np.ascontiguousarray(np.tile(base, (-(-n // base.shape[0]), 1))[:n])
    sizes = [n] * nblk
    recs = []

    def emit(**kw):
        recs.append(kw)
        print(json.dumps(kw), flush=True)

    engs = {}
    mem = dict(shape=a.shape, nblk=nblk, n=n, N=N, memory=True)
    try:
        for arm in ("factor", "stored") if both else ("factor",):
            eng = engs[arm] = Engine(sizes, K=1)
            eng.sync()
            f0 = free_bytes()
            stage_s = build_s = 0.0
            for b in range(nblk):
                t0 = time.perf_counter()
                eng.geno_set_block(b, rows, N)
                t1 = time.perf_counter()
                (eng.geno_ld_factor if arm == "factor" else eng.geno_ld)(0, b)
                t2 = time.perf_counter()
                stage_s += t1 - t0
                build_s += t2 - t1
            eng.geno_clear()
            eng.ld_matvec(0, np.zeros((16, n * nblk)))      # the plan and its scratch
            eng.sync()
            mem.update({arm + "_stored_bytes": eng.stored_bytes(0),
                        arm + "_device_bytes": int(f0 - free_bytes()),
                        arm + "_stage_s": stage_s, arm + "_build_s": build_s})
        mem["factor_scratch_bytes"] = scratch_bytes(nblk, n, N)
        emit(**mem)
        rs = np.random.RandomState(2)
        for nc in [int(c) for c in a.cols.split(",")]:
            V = rs.normal(size=(nc, n * nblk))
            Y = {}
            for arm, eng in engs.items():                     # warm-up of this column count
                Y[arm] = eng.ld_matvec(0, V)
                window(eng, V, 2)
            diff = None
            if both:
                diff = float(np.max(np.abs(Y["factor"] - Y["stored"])) / np.max(np.abs(Y["stored"])))
            ms = {arm: [] for arm in engs}
            for rep in range(a.reps):
                for arm, eng in engs.items():
                    m, t = window(eng, V, a.inner)
                    ms[arm].append(m)
                    emit(shape=a.shape, nc=nc, arm=arm, rep=rep, ms_per_pass=m, inner=a.inner,
                         ld_bytes_per_pass=t["ld_bytes"] / a.inner,
                         ld_flops_per_pass=t["ld_flops"] / a.inner,
                         aux_bytes_per_pass=t["aux_bytes"] / a.inner)
            fm = float(np.median(ms["factor"]))
            s = dict(shape=a.shape, summary=True, nc=nc, factor_ms=fm,
                     factor_ms_min=float(min(ms["factor"])), factor_ms_max=float(max(ms["factor"])),
                     factor_tflops=4.0 * N * n * nblk * nc / (fm * 1e-3) / 1e12,
                     form=engs["factor"].ld_pass_form(0, nc).kind)
            if both:
                sm = float(np.median(ms["stored"]))
                s.update(stored_ms=sm, stored_ms_min=float(min(ms["stored"])),
                         stored_ms_max=float(max(ms["stored"])), factor_over_stored=fm / sm,
                         stored_form=engs["stored"].ld_pass_form(0, nc).kind,
                         maxrel_factor_vs_stored=diff)
            emit(**s)
    finally:
        for eng in engs.values():
            eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
