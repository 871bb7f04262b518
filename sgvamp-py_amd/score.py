#!/usr/bin/env python3
"""Score a target PLINK 1 .bed panel with saved effects: a polygenic score per
individual and, against a phenotype, its correlation and R^2, per effect file --
gVAMP's `test` run mode.  The products run on the device from the 2-bit rows
(sgv_score_*: csrc/score.hip); nothing of size N x M exists on the host or the
device.

  python sgvamp-py_amd/score.py --bed target --effects out/name_xhat_it_50.bin[,...] \\
     [--effects-dir DIR --out-name NAME --iterations 1-50] [--effects-bim train.bim] \\
     [--pheno FILE] [--standardise target|raw] --out PREFIX [--device D]

Effects: a raw f64 .bin of M values (what the solver writes: already divided by
sqrt(Nt), so on the standardised-genotype scale) or a .npy of M or (M, 1) (a
_bet.npy).  They are in the order of --effects-bim (several files: the merged
order of ldio.merge_bims); without it, in the target's own .bim order.  Target
rows are found by variant id.  A variant absent from the target contributes 0 and
is counted.  Where both .bim files give alleles: the same pair with A1 / A2
swapped negates the marker's effect; any other pair skips the marker, counted.
Strand flips and ambiguous (A/T, C/G) pairs are NOT resolved.

--standardise target (default): each marker standardised with the TARGET panel's
own mean and sd (missing -> 0); a marker monomorphic or unobserved in the target
scores 0 and is counted.  raw: A1 dosages 2 / 1 / 0, missing -> the marker's mean
(a swapped marker's dosage counts the other allele there, so negating its effect
shifts every individual's score by the same -2 beta: correlations are unaffected).

Outputs: PREFIX_pgs_it_<it>.bin (N f64; PREFIX_pgs_<k>.bin for the k-th effect
file without an iteration number), PREFIX_score.csv (it, m_used, m_absent,
m_flipped, m_allele_mismatch, m_monomorphic, n_pheno, corr, r2) and PREFIX_ids.txt
(FID IID in score order).  The phenotype is --pheno's `FID IID value` rows, else
.fam column 6; -9, NA and nan mean missing.  corr is the Pearson correlation over
the individuals with a phenotype, r2 its square, both f64 on the host.
"""
import argparse
import os
import re
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

SLAB = 1024                    # csrc/score.h: markers per slab partial
PART_BYTES_MAX = 256 << 20     # the slab partials of one chunk
MAXCOL = 64                    # SGV_SCORE_MAXCOL: columns per stream
MISSING = ("-9", "na", "nan")


# ---- inputs ------------------------------------------------------------------------
def read_effects(path, M=None):
    """(M,) f64 effects of a .bin (raw f64) or a .npy of M or (M, 1); M given: the
    length it must have."""
    if path.endswith(".npy"):
        a = np.load(path)
        if a.ndim == 2 and a.shape[1] == 1:
            a = a[:, 0]
        if a.ndim != 1:
            raise ValueError("%s: effects of shape %s, expected (M,) or (M, 1)" % (path, a.shape))
        a = np.ascontiguousarray(a, dtype=np.float64)
    else:
        size = os.path.getsize(path)
        if size % 8:
            raise ValueError("%s: %d bytes is not a whole number of f64 values" % (path, size))
        a = np.fromfile(path, dtype=np.float64)
    if M is not None and a.shape[0] != M:
        raise ValueError("%s holds %d effects, expected %d" % (path, a.shape[0], M))
    return a


def effect_iteration(path):
    """The iteration number of name_xhat_it_<it>.bin, or None."""
    m = re.search(r"_it_(\d+)\.[A-Za-z]+$", os.path.basename(path))
    return int(m.group(1)) if m else None


def parse_iterations(text):
    """'1-50', '5', '1,4,10-12' -> the iterations in order."""
    out = []
    for part in text.split(","):
        lo, _, hi = part.partition("-")
        out.extend(range(int(lo), int(hi or lo) + 1))
    return out


def read_bim(path):
    """(ids, a1, a2) of a .bim; a1 / a2 None where the file has no allele columns."""
    with open(path) as f:
        rows = [line.split() for line in f if line.strip()]
    if any(len(t) < 2 for t in rows):
        raise ValueError("%s: a line has no variant id" % path)
    ids = [t[1] for t in rows]
    if all(len(t) >= 6 for t in rows):
        return ids, [t[4] for t in rows], [t[5] for t in rows]
    return ids, None, None


def merged_bim(paths):
    """(ids, a1, a2) in the order the effects are in: one file as written, several
    in ldio.merge_bims' merged order (a variant's alleles from the first file that
    has it)."""
    if len(paths) == 1:
        return read_bim(paths[0])
    from ldio import merge_bims

    df, _ = merge_bims(paths)
    ids = [str(v) for v in df["Variant"]]
    first = {}
    for p in paths:
        pid, p1, p2 = read_bim(p)
        if p1 is None:
            continue
        for v, x, y in zip(pid, p1, p2):
            first.setdefault(v, (x, y))
    if not first:
        return ids, None, None
    a1 = [first.get(v, (None, None))[0] for v in ids]
    a2 = [first.get(v, (None, None))[1] for v in ids]
    return ids, a1, a2


def match_variants(eff_ids, eff_a1, eff_a2, tgt_ids, tgt_a1, tgt_a2):
    """Where each effect lands in the target: row[j] (target row, -1 unused) and
    sign[j] (+1, -1 for swapped alleles, 0 unused), with the counts m_used,
    m_absent, m_flipped (among the used), m_allele_mismatch.  Alleles are compared
    as written, case aside, where both sides give them."""
    index = {}
    for i, v in enumerate(tgt_ids):
        index.setdefault(v, i)
    n = len(eff_ids)
    row = np.full(n, -1, dtype=np.int64)
    sign = np.zeros(n, dtype=np.float64)
    absent = flipped = mismatch = 0
    check = eff_a1 is not None and tgt_a1 is not None
    for j, v in enumerate(eff_ids):
        i = index.get(v)
        if i is None:
            absent += 1
            continue
        s = 1.0
        if check and eff_a1[j] is not None and eff_a2[j] is not None:
            e = (eff_a1[j].upper(), eff_a2[j].upper())
            t = (tgt_a1[i].upper(), tgt_a2[i].upper())
            if e == t:
                s = 1.0
            elif e == (t[1], t[0]):
                s = -1.0
                flipped += 1
            else:
                mismatch += 1
                continue
        row[j], sign[j] = i, s
    used = int((row >= 0).sum())
    if used == 0:
        raise ValueError("no variant of the effects matches the target panel (%d effect "
                         "variants: %d absent from the target, %d with other alleles)"
                         % (n, absent, mismatch))
    return dict(row=row, sign=sign, m_used=used, m_absent=absent, m_flipped=flipped,
                m_allele_mismatch=mismatch)


def parse_value(text):
    """A phenotype field: nan for -9, NA, nan (any case) and anything not a number."""
    if text.strip().lower() in MISSING:
        return float("nan")
    try:
        v = float(text)
    except ValueError:
        return float("nan")
    return v if np.isfinite(v) else float("nan")


def read_fam(path):
    """[(FID, IID)] and the column-6 phenotype (nan: missing) of a .fam."""
    ids, ph = [], []
    with open(path) as f:
        for line in f:
            t = line.split()
            if not t:
                continue
            if len(t) < 2:
                raise ValueError("%s: a line has no IID" % path)
            ids.append((t[0], t[1]))
            ph.append(parse_value(t[5]) if len(t) > 5 else float("nan"))
    return ids, np.array(ph, dtype=np.float64)


def read_pheno(path, ids):
    """The phenotype of the individuals `ids` [(FID, IID)] from `FID IID value`
    rows (nan where absent or missing); a header line is skipped."""
    table = {}
    with open(path) as f:
        for k, line in enumerate(f):
            t = line.split()
            if not t:
                continue
            if len(t) < 3:
                raise ValueError("%s line %d: expected FID IID value" % (path, k + 1))
            if k == 0 and t[0].upper() in ("FID", "#FID"):
                continue
            table[(t[0], t[1])] = parse_value(t[2])
    return np.array([table.get(i, float("nan")) for i in ids], dtype=np.float64)


# ---- the pieces of a run -----------------------------------------------------------
def chunk_markers(N, cap_bytes=PART_BYTES_MAX):
    """Markers per chunk: the largest multiple of 1,024 whose slab partials
    (slabs x N x 16 doubles) stay under cap_bytes; one slab at least.  The chunk
    length changes no bit of a score (the order contract of csrc/score.hip)."""
    slabs = cap_bytes // (int(N) * 16 * 8)
    return SLAB * max(1, int(slabs))


def corr_r2(pgs, pheno):
    """(n_pheno, corr, r2): Pearson correlation over the individuals whose
    phenotype is not nan, in f64; nan for fewer than two of them or a constant
    side."""
    pgs, pheno = np.asarray(pgs, dtype=np.float64), np.asarray(pheno, dtype=np.float64)
    m = ~np.isnan(pheno)
    n = int(m.sum())
    if n < 2:
        return n, float("nan"), float("nan")
    dx, dy = pgs[m] - pgs[m].mean(), pheno[m] - pheno[m].mean()
    den = float(np.sqrt((dx * dx).sum() * (dy * dy).sum()))
    if not den > 0.0:
        return n, float("nan"), float("nan")
    c = float((dx * dy).sum() / den)
    return n, c, c * c


def score_panel(bed, effects, eff_bim=None, standardise="target", device=None, engine=None,
                chunk=None):
    """Score the panel `bed` (prefix) with effects (ncol, M_eff), which are in the
    order of eff_bim = (ids, a1, a2) or, without it, of the target's own .bim.
    Returns dict(pgs (ncol, N), ids [(FID, IID)], fam_pheno, m_used, m_absent,
    m_flipped, m_allele_mismatch, m_monomorphic, read_s, device_s, chunk)."""
    import hip_backend as hb
    from engine import Engine
    from ldio import read_bed

    if standardise not in ("target", "raw"):
        raise ValueError("standardise must be target or raw")
    panel = read_bed(bed)
    t_ids, t_a1, t_a2 = read_bim(panel.prefix + ".bim")
    effects = np.atleast_2d(np.asarray(effects, dtype=np.float64))
    if eff_bim is None:
        if effects.shape[1] != panel.M:
            raise ValueError("%d effects for the %d variants of %s.bim: give --effects-bim"
                             % (effects.shape[1], panel.M, panel.prefix))
        eff_bim = (t_ids, None, None)
    e_ids, e_a1, e_a2 = eff_bim
    if effects.shape[1] != len(e_ids):
        raise ValueError("%d effects for the %d variants of the effects' .bim"
                         % (effects.shape[1], len(e_ids)))
    mt = match_variants(e_ids, e_a1, e_a2, t_ids, t_a1, t_a2)
    used = np.nonzero(mt["row"] >= 0)[0]
    used = used[np.argsort(mt["row"][used], kind="stable")]     # the .bed is read front to back
    rows_sel = mt["row"][used]
    beta = np.ascontiguousarray(effects[:, used] * mt["sign"][used][None, :])
    N, ncol, Mu = panel.N, effects.shape[0], len(used)
    step = chunk_markers(N) if chunk is None else int(chunk)
    if step < SLAB or step % SLAB:
        raise ValueError("the chunk length must be a multiple of %d" % SLAB)
    mode = hb.SCORE_TARGET if standardise == "target" else hb.SCORE_RAW
    own = engine is None
    eng = Engine([64], K=1, device=device) if own else engine
    pgs = np.empty((ncol, N), dtype=np.float64)
    read_s = device_s = 0.0
    mono = 0
    try:
        for c0 in range(0, ncol, MAXCOL):            # each batch re-streams the panel
            c1 = min(ncol, c0 + MAXCOL)
            eng.score_begin(N, c1 - c0)
            for i in range(0, Mu, step):
                j = min(Mu, i + step)
                t0 = time.perf_counter()
                rows = np.ascontiguousarray(panel.rows[rows_sel[i:j]])
                t1 = time.perf_counter()
                cnt = eng.score_chunk(rows, beta[c0:c1, i:j], mode=mode)
                device_s += time.perf_counter() - t1
                read_s += t1 - t0
                if c0 == 0:
                    nobs = cnt[:, 0] + cnt[:, 2] + cnt[:, 3]
                    s1, s2 = 2 * cnt[:, 0] + cnt[:, 2], 4 * cnt[:, 0] + cnt[:, 2]
                    mono += int(((nobs == 0) | (nobs * s2 - s1 * s1 == 0)).sum())
            t1 = time.perf_counter()
            pgs[c0:c1] = eng.score_end()
            device_s += time.perf_counter() - t1
    finally:
        if own:
            eng.close()
    ids, fam_ph = read_fam(panel.prefix + ".fam")
    out = {k: mt[k] for k in ("m_used", "m_absent", "m_flipped", "m_allele_mismatch")}
    out.update(pgs=pgs, ids=ids, fam_pheno=fam_ph, m_monomorphic=mono, read_s=read_s,
               device_s=device_s, chunk=step)
    return out


def fmt(v):
    return "" if v is None or (isinstance(v, float) and np.isnan(v)) else repr(v)


# ---- CLI ---------------------------------------------------------------------------
def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--bed", required=True, help="target panel prefix (.bed/.bim/.fam)")
    ap.add_argument("--effects", help="effect files, comma separated (.bin f64 or .npy)")
    ap.add_argument("--effects-dir", help="with --out-name and --iterations: DIR/NAME_xhat_it_<it>.bin")
    ap.add_argument("--out-name")
    ap.add_argument("--iterations", help="e.g. 1-50 or 5,10,20-25")
    ap.add_argument("--effects-bim", help=".bim file(s) the effects are ordered by, comma separated")
    ap.add_argument("--pheno", help="FID IID value rows (default: .fam column 6)")
    ap.add_argument("--standardise", choices=("target", "raw"), default="target")
    ap.add_argument("--out", required=True, help="output prefix")
    ap.add_argument("--device", type=int, default=None)
    a = ap.parse_args(argv)

    files = [p for p in (a.effects or "").split(",") if p]
    if a.effects_dir or a.out_name or a.iterations:
        if not (a.effects_dir and a.out_name and a.iterations):
            ap.error("--effects-dir, --out-name and --iterations go together")
        files += [os.path.join(a.effects_dir, "%s_xhat_it_%d.bin" % (a.out_name, it))
                  for it in parse_iterations(a.iterations)]
    if not files:
        ap.error("no effect file: give --effects or --effects-dir/--out-name/--iterations")
    try:
        eff_bim = merged_bim(a.effects_bim.split(",")) if a.effects_bim else None
        M = len(eff_bim[0]) if eff_bim else None
        cols = [read_effects(p, M) for p in files]
        if len({c.shape[0] for c in cols}) != 1:
            raise ValueError("the effect files differ in length: %s"
                             % ", ".join("%s: %d" % (p, c.shape[0]) for p, c in zip(files, cols)))
        res = score_panel(a.bed, np.stack(cols), eff_bim, a.standardise, a.device)
        pheno = read_pheno(a.pheno, res["ids"]) if a.pheno else res["fam_pheno"]
    except (ValueError, OSError) as e:
        print("score.py: error: %s" % e, file=sys.stderr)
        return 1
    d = os.path.dirname(os.path.abspath(a.out))
    os.makedirs(d, exist_ok=True)
    with open(a.out + "_ids.txt", "w") as f:
        for fid, iid in res["ids"]:
            f.write("%s\t%s\n" % (fid, iid))
    with open(a.out + "_score.csv", "w") as f:
        f.write("it,m_used,m_absent,m_flipped,m_allele_mismatch,m_monomorphic,n_pheno,corr,r2\n")
        for k, p in enumerate(files):
            it = effect_iteration(p)
            name = "%s_pgs_it_%d.bin" % (a.out, it) if it is not None else "%s_pgs_%d.bin" % (a.out, k)
            res["pgs"][k].tofile(name)
            n, c, r2 = corr_r2(res["pgs"][k], pheno)
            f.write(",".join([str(it if it is not None else k)]
                             + [str(res[x]) for x in ("m_used", "m_absent", "m_flipped",
                                                      "m_allele_mismatch", "m_monomorphic")]
                             + [str(n), fmt(c), fmt(r2)]) + "\n")
    print("scored %d individuals x %d effect file(s): %d markers used, %d absent, %d flipped, "
          "%d allele mismatches, %d monomorphic in the target; chunks of %d markers; file read "
          "%.3f s, device %.3f s"
          % (len(res["ids"]), len(files), res["m_used"], res["m_absent"], res["m_flipped"],
             res["m_allele_mismatch"], res["m_monomorphic"], res["chunk"], res["read_s"],
             res["device_s"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
