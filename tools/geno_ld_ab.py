#!/usr/bin/env python3
"""Build time of one north-star-shaped LD block (n = 15,625 markers, N = 10,000
samples) from .bed bits (geno_set_block + geno_ld) against the synthetic
generator's build of the same shape (synth_ld_g: hash, materialise G, k_syrk_nt),
on one device in alternating arms; then the wall time of all 64 such blocks from
bits and the device memory the staged genotypes take.

  python tools/geno_ld_ab.py --out profiles/geno_ld/build_ab.jsonl [--n 15625 --N 10000 --reps 5]

Times are host clocks around calls that end in a stream wait.  One JSON line per
timed call, then a summary line.  Needs a GPU; there is no fallback."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sgvamp-py_amd"))

from engine import Engine  # noqa: E402


def free_bytes():
    hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    if hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) != 0:
        raise RuntimeError("hipMemGetInfo failed")
    return int(free.value)


def draw_rows(n, N, seed):
    """Packed .bed rows of A1 counts at allele frequencies in [0.05, 0.5], 1 % missing."""
    rs = np.random.RandomState(seed)
    nb = (N + 3) // 4
    rows = np.zeros((n, nb), dtype=np.uint8)
    lut = np.array([3, 2, 0], dtype=np.uint8)
    for i0 in range(0, n, 1024):                      # in slabs: 10 MB of codes at a time
        m = min(1024, n - i0)
        p = rs.uniform(0.05, 0.5, size=(m, 1))
        codes = lut[rs.binomial(2, p, size=(m, N))]
        codes[rs.uniform(size=(m, N)) < 0.01] = 1
        pad = np.zeros((m, nb * 4), dtype=np.uint8)
        pad[:, :N] = codes
        q = pad.reshape(m, nb, 4)
        rows[i0:i0 + m] = q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--n", type=int, default=15625)
    ap.add_argument("--N", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=64)
    a = ap.parse_args()
    n, N = a.n, a.N
    rows = draw_rows(n, N, 1)
    zeros = np.zeros(n)
    recs = []

    def emit(**kw):
        recs.append(kw)
        print(json.dumps(kw), flush=True)

    eng = Engine([n], K=1)
    try:
        eng.sync()
        f0 = free_bytes()
        eng.geno_set_block(0, rows, N)
        f1 = free_bytes()
        eng.geno_ld(0, 0)                              # warm-up of both arms
        f2 = free_bytes()
        R_bed = eng.get_ld_block(0, 0)
        eng.synth_ld_g(0, 5, N, zeros)
        for rep in range(a.reps):
            t0 = time.perf_counter()
            eng.geno_set_block(0, rows, N)
            t1 = time.perf_counter()
            eng.geno_ld(0, 0)
            t2 = time.perf_counter()
            emit(arm="bed", rep=rep, n=n, N=N, stage_stats_ms=(t1 - t0) * 1e3,
                 syrk_ms=(t2 - t1) * 1e3, total_ms=(t2 - t0) * 1e3)
            t0 = time.perf_counter()
            eng.synth_ld_g(0, 5, N, zeros)
            t1 = time.perf_counter()
            emit(arm="synth", rep=rep, n=n, N=N, total_ms=(t1 - t0) * 1e3)
        t0 = time.perf_counter()
        for _ in range(a.blocks):                      # every block of an M = blocks * n job
            eng.geno_set_block(0, rows, N)
            eng.geno_ld(0, 0)
        all_s = time.perf_counter() - t0
    finally:
        eng.close()
    d = np.diag(R_bed)
    bed = np.array([r["total_ms"] for r in recs if r["arm"] == "bed"])
    syrk = np.array([r["syrk_ms"] for r in recs if r["arm"] == "bed"])
    syn = np.array([r["total_ms"] for r in recs if r["arm"] == "synth"])
    macs = n * (n + 64) / 2.0 * (-(-N // 16) * 16)     # upper tiles, padded K
    emit(summary=True, n=n, N=N, reps=a.reps,
         bed_ms_median=float(np.median(bed)), bed_ms_min=float(bed.min()),
         bed_ms_max=float(bed.max()), bed_syrk_ms_median=float(np.median(syrk)),
         synth_ms_median=float(np.median(syn)), synth_ms_min=float(syn.min()),
         synth_ms_max=float(syn.max()),
         bed_syrk_tflops=float(2 * macs / (np.median(syrk) * 1e-3) / 1e12),
         bed_rows_bytes=int(rows.nbytes),
         bed_device_scratch_bytes=int(f0 - f1),        # staged rows + per-marker tables
         bed_scratch_formula_bytes=int(n * (-(-N // 16)) * 4 + n * 48),
         synth_G_scratch_bytes=int(n * (-(-N // 16) * 16) * 8),
         ld_block_bytes=int(f1 - f2),
         all_blocks=a.blocks, all_blocks_wall_s=float(all_s),
         diag_min=float(d.min()), diag_max=float(d.max()),
         symmetric=bool(np.array_equal(R_bed, R_bed.T)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
