#!/usr/bin/env python3
"""What every LD pass form reports, beside what a kernel trace sees.

For each A/B arm of the pass switches (none, then the arms of
profiles/pass_form/) this builds the triangle, band and mixed engines of
tests/test_gpu_pass_exact.py at their present sizes, f64 and f32-stored, runs
one pass at 2, 4, 8 and 16 columns and prints the form Engine.ld_pass_form
reports for it with the kernels that form names.  Run under a kernel trace,

  rocprofv3 --kernel-trace --stats -- python tools/pass_form_sweep.py --lib LIB

the kernel names in the stats must be the ones printed here.  --lib may be a
build from before sgv_ld_pass_form (the A/B's parent): the passes run, the
form column reads "-", and its trace must show the same names.
--names STATS.csv prints the distinct LD-pass kernel names of a rocprofv3
kernel_stats file, template arguments kept."""
import argparse
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sgvamp-py_amd"))
sys.path.insert(0, ROOT)

ARMS = [{}, {"SGV_MF_WIDE": "0", "SGV_MF_PAIR": "0"}, {"SGV_MF_PAIR": "1"}, {"SGV_MF_WIDE": "1"},
        {"SGV_MF_WIDE_IDLE": "0"}, {"SGV_BAND_WALK": "0"}, {"SGV_F32_WALK": "1"},
        {"SGV_F32_FORM": "1"}, {"SGV_FIN_FORM": "1"}, {"SGV_FIN_FORM": "4"}]
SWITCHES = ("SGV_AB", "SGV_BAND_WALK", "SGV_F32_WALK", "SGV_MF_WIDE", "SGV_MF_PAIR",
            "SGV_MF_WIDE_IDLE", "SGV_F32_FORM", "SGV_FIN_FORM")
NCOLS = (2, 4, 8, 16)
STRIP = {"strip4": "k_sym_mfma<", "pair": "k_sym_mfma_pair<", "strip16": "k_sym_mfma16<"}
PASS_KERNELS = ("k_ld_pass", "k_sym_pass", "k_sym_finalize", "k_pack", "k_sym_mfma", "k_band_walk",
                "k_walk_fin")


def kernels(f):
    """The kernels a reported form names, in launch order."""
    k = ["k_ld_pass"] if f.dense else []
    if f.kind == "valu":
        return k + ["k_sym_pass<class %d>" % f.valu_class, "k_sym_finalize"]
    if f.kind == "none":
        return k
    k.append("k_pack<%d%s>" % (f.pk_width, ", paired" if f.pk_paired else ""))
    fin = {1: "k_sym_finalize_strip1", 4: "k_sym_finalize_strip", 0: None}[f.fin_form]
    if f.kind == "walk":
        return k + ["k_band_walk<load form %d>" % f.load_form, "k_walk_fin"]
    if f.kind == "wide":
        k += ["k_sym_mfma_wide<idle exit %d>" % f.idle_exit, "k_sym_finalize_wide"]
        if f.rest_kind != "none":
            k += [STRIP[f.rest_kind] + "load form %d>" % f.load_form, fin]
        return k
    return k + [STRIP[f.kind] + "load form %d>" % f.load_form, fin]


def names(path):
    seen = set()
    for row in csv.DictReader(open(path)):
        n = row.get("Name") or row.get("Kernel_Name") or ""
        if any(p in n for p in PASS_KERNELS):
            seen.add(n.split("(")[0])
    for n in sorted(seen):
        print(n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--names", default=None)
    a = ap.parse_args()
    if a.names:
        return names(a.names)
    import hip_backend as hb
    lib = hb.load(a.lib, strict=False) if a.lib else hb.load()
    reports = hasattr(lib, "sgv_ld_pass_form")
    from engine import Engine
    from tests import exact_ld as xl

    bits = xl.NARROW["bits"]
    plans = {
        "tri": [xl.exact_block(n, bits, 11) for n in xl.TRI_SIZES],
        "mixed": [xl.Band(1537, bits, 16, 300), xl.exact_block(1281, bits, 11),
                  xl.Band(2305, bits, 16, 40), xl.exact_block(513, bits, 11)],
    }
    for bw in xl.WALK_BWS:
        plans["band%d" % bw] = [xl.Band(n, bits, 13, bw) for n in xl.walk_sizes(bw)]
    for arm in ARMS:
        for k in SWITCHES:
            os.environ.pop(k, None)
        if arm:
            os.environ.update(dict(arm, SGV_AB="1"))
        tag = " ".join("%s=%s" % kv for kv in arm.items()) or "default"
        for name, blocks in plans.items():
            sizes = [xl.block_size(B) for B in blocks]
            V = np.ones((16, sum(sizes)))
            for prec in (64, 32):
                eng = Engine(sizes, K=1)
                eng.set_ld_precision(prec)
                for b, B in enumerate(blocks):
                    (eng.set_ld_block_csr if isinstance(B, xl.Band) else eng.set_ld_block)(0, b, B)
                for nc in NCOLS:
                    f = eng.ld_pass_form(0, nc) if reports else None
                    eng.ld_matvec(0, V[:nc])
                    print("%-28s %-8s f%d nc=%-2d %s" % (
                        tag, name, prec, nc, " ".join(x for x in kernels(f) if x) if f else "-"))
                eng.close()


if __name__ == "__main__":
    main()
