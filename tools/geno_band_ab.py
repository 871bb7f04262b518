#!/usr/bin/env python3
"""Build time of one band piece (n = 65,536 markers, N = 10,000 samples) from .bed
bits as a windowed packed band (geno_ld_band, W = 1,000: arm B) against the
dense-triangle build of the same rows (geno_ld: arm A), on one device in
alternating arms; then the build of one whole chromosome (M = 1e6 markers in
BAND_PIECE pieces, couplings included) and its stored bytes.

  python tools/geno_band_ab.py --out profiles/geno_band/build_ab.jsonl \
      [--n 65536 --N 10000 --window 1000 --reps 5 --M 1000000 --piece 65536]

The two arms fill two LD matrices of one engine, so after the warm-up no arm
allocates.  Times are host clocks around calls that end in a stream wait.  A
kernel's rate is fma per second per stored in-window entry's sample: entries x
padded N / time.  One JSON line per timed call, then a summary line.  Needs a
GPU; there is no fallback."""
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


def draw_rows(n, N, seed, distinct=2048):
    """Packed .bed rows of A1 counts at allele frequencies in [0.05, 0.5], 1 %
    missing: `distinct` drawn rows repeated to n (the kernels' time does not depend
    on the codes; every row has LD)."""
    rs = np.random.RandomState(seed)
    nb = (N + 3) // 4
    m = min(distinct, n)
    lut = np.array([3, 2, 0], dtype=np.uint8)
    p = rs.uniform(0.05, 0.5, size=(m, 1))
    codes = lut[rs.binomial(2, p, size=(m, N))]
    codes[rs.uniform(size=(m, N)) < 0.01] = 1
    pad = np.zeros((m, nb * 4), dtype=np.uint8)
    pad[:, :N] = codes
    q = pad.reshape(m, nb, 4)
    base = q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)
    return np.ascontiguousarray(np.tile(base, (-(-n // m), 1))[:n])


def band_entries(n, W):
    """Stored in-window entries of the upper triangle, diagonal included."""
    W = min(W, n - 1)
    return n * (W + 1) - W * (W + 1) // 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--N", type=int, default=10000)
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--M", type=int, default=1000000)
    ap.add_argument("--piece", type=int, default=65536)
    a = ap.parse_args()
    n, N, W = a.n, a.N, a.window
    npad = -(-N // 16) * 16
    recs = []

    def emit(**kw):
        recs.append(kw)
        print(json.dumps(kw), flush=True)

    # ---- one piece: arm A (ld 0) against arm B (ld 1) ---------------------------
    rows = draw_rows(n, N, 1)
    eng = Engine([n], K=2, ld_of=[0, 1])
    try:
        eng.sync()
        f0 = free_bytes()
        eng.geno_set_block(0, rows, N)
        f1 = free_bytes()
        eng.geno_ld(0, 0)                              # warm-up of both arms
        f2 = free_bytes()
        eng.geno_ld_band(1, 0, W)
        f3 = free_bytes()
        tri_bytes, band_bytes = eng.stored_bytes(0), eng.stored_bytes(1)
        for rep in range(a.reps):
            t0 = time.perf_counter()
            eng.geno_ld(0, 0)
            t1 = time.perf_counter()
            emit(arm="A_triangle", rep=rep, n=n, N=N, ms=(t1 - t0) * 1e3)
            t0 = time.perf_counter()
            eng.geno_ld_band(1, 0, W)
            t1 = time.perf_counter()
            emit(arm="B_band", rep=rep, n=n, N=N, window=W, ms=(t1 - t0) * 1e3)
    finally:
        eng.close()
    ta = np.array([r["ms"] for r in recs if r["arm"] == "A_triangle"])
    tb = np.array([r["ms"] for r in recs if r["arm"] == "B_band"])
    ea, eb = n * (n + 1) // 2, band_entries(n, W)
    rate_a = ea * npad / (np.median(ta) * 1e-3)
    rate_b = eb * npad / (np.median(tb) * 1e-3)

    # ---- one chromosome: M markers in pieces, couplings included -----------------
    k = a.M // a.piece
    pieces = [a.piece] * (k - 1) + [a.M - a.piece * (k - 1)] if k >= 2 else [a.M]
    src = draw_rows(max(pieces), N, 2)
    bw = min(W, min(pieces))
    eng = Engine(pieces, K=1)
    try:
        eng.sync()
        t0 = time.perf_counter()
        for b, nb in enumerate(pieces):
            eng.geno_set_block(b, src[:nb], N)
            eng.geno_ld_band(0, b, W)
        t1 = time.perf_counter()
        for gb in range(len(pieces) - 1):
            halo = np.concatenate([src[pieces[gb] - bw:pieces[gb]], src[:bw]])
            eng.geno_coupling(0, gb, bw, bw, halo, N, W)
        t2 = time.perf_counter()
        eng.geno_clear()
        chrom_bytes = eng.stored_bytes(0)
        fmts = sorted({eng.ld_block_format(0, b) for b in range(len(pieces))})
    finally:
        eng.close()
    nnz = sum(band_entries(p, W) for p in pieces)
    emit(summary=True, n=n, N=N, window=W, reps=a.reps,
         A_ms_median=float(np.median(ta)), A_ms_min=float(ta.min()), A_ms_max=float(ta.max()),
         B_ms_median=float(np.median(tb)), B_ms_min=float(tb.min()), B_ms_max=float(tb.max()),
         A_entries=int(ea), B_entries=int(eb),
         A_gfma_per_s_per_entry=float(rate_a / 1e9), B_gfma_per_s_per_entry=float(rate_b / 1e9),
         B_over_A_rate=float(rate_b / rate_a), expected_at_least=0.75,
         rate_ok=bool(rate_b / rate_a >= 0.75),
         staged_rows_and_tables_bytes=int(f0 - f1),
         staged_formula_bytes=int(n * (npad // 16) * 4 + n * 48),
         A_block_device_bytes=int(f1 - f2), B_block_device_bytes=int(f2 - f3),
         A_stored_bytes=float(tri_bytes), B_stored_bytes=float(band_bytes),
         chrom_M=a.M, chrom_pieces=len(pieces), chrom_last_piece=int(pieces[-1]),
         chrom_blocks_wall_s=float(t1 - t0), chrom_couplings_wall_s=float(t2 - t1),
         chrom_wall_s=float(t2 - t0), chrom_formats=fmts,
         chrom_stored_bytes=float(chrom_bytes),
         chrom_coupling_bytes=int((len(pieces) - 1) * 2 * bw * bw * 8),
         chrom_csr_route_device_bytes=float(chrom_bytes),     # the same layout (tested bitwise)
         chrom_csr_route_host_bytes=int(nnz * 16 + (a.M + len(pieces)) * 8))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
