#!/usr/bin/env python3
"""Scoring on the f64 matrix cores (sgv_score_*: csrc/score.hip) against the only
other route to the same numbers, one sgv_geno_g call per column on the same
panel staged as one block.  One 65,536-marker chunk per call:

  timeout -k 10 300 python tools/score_ab.py --N 2000 --out profiles/score/score_ab.jsonl && \\
  timeout -k 10 300 python tools/score_ab.py --N 10000 --out profiles/score/score_ab.jsonl && \\
  timeout -k 10 420 python tools/score_ab.py --N 50000 --out profiles/score/score_ab.jsonl && \\
  timeout -k 10 420 python tools/score_ab.py --e2e --out profiles/score/score_ab.jsonl

(each step under its own time limit, chained, so a fault ends the sequence; a call
appends its lines).  Arm A, `mfma`, at 1, 4, 16 and 64 columns: the library's own
HIP events around the stream's kernels (sgv_score_timers: pack, MFMA, slab sums)
and the call's wall time, which also holds the chunk's staging (repacking the
rows, the upload, the counts).  Arm B, `geno_g`: wall time of 16 sgv_geno_g calls
(each uploads M effects, runs one kernel over the staged block and downloads N
sums; the panel is staged once, outside the timing).  After a warm-up of both,
the arms alternate within a repetition; medians of --reps.  TF/s counts 2 N M
ncol flops over the kernel time.  --e2e: one score.py run (score_panel) at N =
10,000, M = 200,000, 50 columns from a .bed written to a temporary directory,
split into file-read and device time.  --lib PATH --tag NAME --skip-b: arm A on a
timing variant of the library (a kernel with a part taken out computes wrong
sums: its times are the point).  The panel is 2,048 drawn rows (allele
frequencies in [0.05, 0.5], 1 % missing) tiled.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sgvamp-py_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import hip_backend as hb  # noqa: E402
from engine import Engine  # noqa: E402
from geno_ld_ab import draw_rows  # noqa: E402

M_CHUNK = 65536
MFMA_PROBE_TFLOPS = 47.0      # tools/mfma_probe.hip: v_mfma_f64_16x16x4_f64, whole device


def tiled(M, N, base=2048):
    b = draw_rows(min(M, base), N, 1)
    return np.ascontiguousarray(np.tile(b, (-(-M // b.shape[0]), 1))[:M])


def arm_a(eng, rows, N, beta):
    eng.score_timers(reset=True)
    t0 = time.perf_counter()
    eng.score_begin(N, beta.shape[0])
    eng.score_chunk(rows, beta, mode=hb.SCORE_TARGET)
    S = eng.score_end()
    wall = (time.perf_counter() - t0) * 1e3
    t = eng.score_timers()
    return S, wall, t["kernel_ms"], t["stage_ms"]


def arm_b(eng, N, beta):
    t0 = time.perf_counter()
    g = np.stack([eng.geno_g(b, N)[0] for b in beta])
    return g, (time.perf_counter() - t0) * 1e3


def ab(a, emit):
    N, M = a.N, M_CHUNK
    rows = tiled(M, N)
    rs = np.random.RandomState(2)
    eng = Engine([M], K=1)
    try:
        if not a.skip_b:
            eng.geno_set_block(0, rows, N)
        beta16 = rs.normal(size=(16, M)) / np.sqrt(M)
        S, _, _, _ = arm_a(eng, rows, N, beta16)            # warm-up, and the arms agree
        ka, wa, wb = [], [], []
        if not a.skip_b:
            g, _ = arm_b(eng, N, beta16)
            diff = float(np.max(np.abs(S - g))) / float(np.max(np.abs(g)))
        for rep in range(a.reps):
            _, wall, kms, stage = arm_a(eng, rows, N, beta16)
            ka.append(kms), wa.append(wall)
            emit(N=N, M=M, rep=rep, arm="mfma", ncol=16, kernel_ms=kms, wall_ms=wall, stage_ms=stage)
            if not a.skip_b:
                _, bms = arm_b(eng, N, beta16)
                wb.append(bms)
                emit(N=N, M=M, rep=rep, arm="geno_g", ncol=16, wall_ms=bms)
        km = float(np.median(ka))
        s = dict(N=N, M=M, summary=True, ncol=16, mfma_kernel_ms=km, mfma_kernel_ms_min=float(min(ka)),
                 mfma_kernel_ms_max=float(max(ka)), mfma_wall_ms=float(np.median(wa)),
                 mfma_tflops=2.0 * N * M * 16 / (km * 1e-3) / 1e12, probe_tflops=MFMA_PROBE_TFLOPS)
        if not a.skip_b:
            bm = float(np.median(wb))
            s.update(geno_g_wall_ms=bm, geno_g_wall_ms_min=float(min(wb)),
                     geno_g_wall_ms_max=float(max(wb)), geno_g_over_mfma_kernel=bm / km,
                     geno_g_over_mfma_wall=bm / float(np.median(wa)), maxrel_mfma_vs_geno_g=diff)
        emit(**s)
        for nc in (1, 4, 64):
            beta = rs.normal(size=(nc, M)) / np.sqrt(M)
            arm_a(eng, rows, N, beta)
            ks = [arm_a(eng, rows, N, beta)[2] for _ in range(a.reps)]
            km = float(np.median(ks))
            emit(N=N, M=M, summary=True, ncol=nc, mfma_kernel_ms=km, mfma_kernel_ms_min=float(min(ks)),
                 mfma_kernel_ms_max=float(max(ks)),
                 mfma_tflops=2.0 * N * M * nc / (km * 1e-3) / 1e12)
    finally:
        eng.close()


def e2e(a, emit):
    import score

    N, M, ncol = 10000, 200000, 50
    rows = tiled(M, N)
    with tempfile.TemporaryDirectory() as d:
        prefix = os.path.join(d, "target")
        with open(prefix + ".bed", "wb") as f:
            f.write(b"\x6c\x1b\x01")
            f.write(rows.tobytes())
        with open(prefix + ".bim", "w") as f:
            for i in range(M):
                f.write("1\trs%d\t0\t%d\tA\tG\n" % (i, i + 1))
        with open(prefix + ".fam", "w") as f:
            for s in range(N):
                f.write("f%d\ti%d\t0\t0\t0\t-9\n" % (s, s))
        del rows
        beta = np.random.RandomState(3).normal(size=(ncol, M)) / np.sqrt(M)
        t0 = time.perf_counter()
        res = score.score_panel(prefix, beta)
        total = time.perf_counter() - t0
    emit(e2e=True, N=N, M=M, ncol=ncol, chunk=res["chunk"], total_s=total, read_s=res["read_s"],
         device_s=res["device_s"], m_monomorphic=res["m_monomorphic"],
         pgs_absmax=float(np.max(np.abs(res["pgs"]))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--N", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--lib", help="a timing variant of the library to load instead of the in-tree one")
    ap.add_argument("--tag", help="label of the variant, written into every line")
    ap.add_argument("--skip-b", action="store_true", help="arm A only (variants)")
    a = ap.parse_args()
    if a.lib:
        hb.load(a.lib)
    recs = []

    def emit(**kw):
        if a.tag:
            kw["tag"] = a.tag
        recs.append(kw)
        print(json.dumps(kw), flush=True)

    try:
        (e2e if a.e2e else ab)(a, emit)
    finally:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
