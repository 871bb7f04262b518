#!/usr/bin/env python3
"""Build time of one band piece (n = 65,536 markers, N = 10,000 samples, W = 1,000)
from .bed bits by k_bed_band with the reach read per row against the same kernel
with the marker window formed in registers, on one device in alternating arms:

  A  geno_ld_band(W)                          the window policy, the reference arm
  B  geno_ld_band_reach(hi = min(i + W, n-1))  the row policy, the same entries
  C  B with the triangular taper (pos = the index, D = W + 1)
  R  a ragged reach of the same MAXIMUM W: gaps between positions swing from 1 to
     4 and back along the piece, so the reach runs from W down to about W / 4

  python tools/geno_reach_ab.py --out profiles/geno_reach/build_ab.jsonl \
      [--n 65536 --N 10000 --window 1000 --reps 5]

The arms fill four LD matrices of one engine, so after the warm-up no arm
allocates.  Times are host clocks around calls that end in a stream wait.  One
JSON line per timed call, then a summary line: medians, min-max spreads, whether B
and C stay within A's own spread plus 2 %, and what the per-piece extent costs the
ragged piece (its stored bytes are the uniform window's, its entries fewer).
Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sgvamp-py_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from engine import Engine  # noqa: E402
from geno_band_ab import draw_rows  # noqa: E402


def ragged_positions(n, W):
    """Positions whose gaps swing 1 -> 4 -> 1 along the piece, and the span at which
    the widest reach is W (in the gap-1 stretches)."""
    gap = 1.0 + 3.0 * (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n))
    return np.cumsum(np.round(gap * 8.0) / 8.0), float(W)


def reach_of(pos, D):
    hi = np.searchsorted(pos, pos + D, side="right") - 1     # exact: multiples of 1/8
    return np.clip(hi, np.arange(len(pos)), len(pos) - 1).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--N", type=int, default=10000)
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n, N, W = a.n, a.N, a.window
    recs = []

    def emit(**kw):
        recs.append(kw)
        print(json.dumps(kw), flush=True)

    idx = np.arange(n)
    uni = np.minimum(idx + W, n - 1).astype(np.int32)
    ipos = idx.astype(np.float64)
    rpos, rspan = ragged_positions(n, W)
    rag = reach_of(rpos, rspan)
    width = rag - idx
    arms = {
        "A_band": lambda eng: eng.geno_ld_band(0, 0, W),
        "B_reach": lambda eng: eng.geno_ld_band_reach(1, 0, uni),
        "C_reach_taper": lambda eng: eng.geno_ld_band_reach(2, 0, uni, ipos, W + 1.0),
        "R_ragged": lambda eng: eng.geno_ld_band_reach(3, 0, rag),
    }
    rows = draw_rows(n, N, 1)
    eng = Engine([n], K=4, ld_of=[0, 1, 2, 3])
    try:
        eng.geno_set_block(0, rows, N)
        for call in arms.values():                     # warm-up: every arm allocates here
            call(eng)
        stored = {name: eng.stored_bytes(l) for l, name in enumerate(arms)}
        fmts = {name: eng.ld_block_format(l, 0) for l, name in enumerate(arms)}
        for rep in range(a.reps):
            for name, call in arms.items():
                t0 = time.perf_counter()
                call(eng)
                t1 = time.perf_counter()
                emit(arm=name, rep=rep, n=n, N=N, window=W, ms=(t1 - t0) * 1e3)
    finally:
        eng.close()
    t = {name: np.array([r["ms"] for r in recs if r["arm"] == name]) for name in arms}
    med = {k: float(np.median(v)) for k, v in t.items()}
    spread = float(t["A_band"].max() - t["A_band"].min())
    bar = med["A_band"] + spread + 0.02 * med["A_band"]
    entries = {"A_band": int(np.sum(uni - idx + 1)), "R_ragged": int(np.sum(width + 1))}
    emit(summary=True, n=n, N=N, window=W, reps=a.reps,
         **{k + "_ms_median": med[k] for k in arms},
         **{k + "_ms_min": float(t[k].min()) for k in arms},
         **{k + "_ms_max": float(t[k].max()) for k in arms},
         A_spread_ms=spread, bar_ms=bar,
         B_within_bar=bool(med["B_reach"] <= bar), C_within_bar=bool(med["C_reach_taper"] <= bar),
         ragged_reach_max=int(width.max()), ragged_reach_min_inner=int(width[:n - W].min()),
         ragged_entries=entries["R_ragged"], uniform_entries=entries["A_band"],
         ragged_over_uniform_entries=entries["R_ragged"] / entries["A_band"],
         ragged_over_uniform_ms=med["R_ragged"] / med["A_band"],
         stored_bytes=stored, formats=fmts)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
