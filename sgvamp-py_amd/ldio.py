"""Input loaders of the CLI (src/main.py:126-285), host side.

* .bim files: union of variants over cohorts, sorted by Coordinate (main.py:132-143)
* r vectors:  .txt / .npy / PLINK .linear (BETA, NaN -> 0, x sqrt(N)) (main.py:176-191)
* LD:         .npy dense (block structure detected), .npz CSR (block-diagonal
              detected from indptr/indices), or the build's block manifest
              ``*.blocks.json`` = {"block_sizes": [...], "files": [one .npy per
              block]} for LD that cannot exist as one dense array (M = 1e6).
* PLINK .ld text LD (main.py:203-257): per cohort a CSR matrix with a unit
              diagonal and every listed pair in both triangles (duplicates summed, as
              scipy's COO -> CSR does); markers a cohort lacks are filled from another
              cohort (the reference's MPI point-to-point exchange, emulated here in one
              process: load_plink_ld_all)
* true signal: .bin (f64) / .npy, multiplied by sqrt(N) (main.py:268-285)
* genotypes:  a PLINK 1 .bed/.bim/.fam panel (read_bed) as an LD source: BedLD
              forms each LD block on the device from the block's 2-bit rows
              (simulation/sim_phen.py:33-37 reads such a panel with bed_reader;
              here NumPy only); windowed by markers, by the .bim's kb or cM, with
              an optional triangular taper; one block per chromosome
              (chromosome_blocks)
"""
import json
import os
import struct

import numpy as np

from sgvamp import BlockLD


def merge_bims(bim_paths):
    """Returns (bim_ref DataFrame, per-cohort variant lists).  src/main.py:132-143."""
    import pandas as pd

    bim_list, bim_ref_df = [], None
    for k, path in enumerate(bim_paths):
        df = pd.read_table(path, sep=r"\s+", header=None,
                           names=["Chromosome", "Variant", "Position", "Coordinate", "Allele1",
                                  "Allele2"])
        bim_list.append(list(df["Variant"]))
        if k == 0:
            bim_ref_df = df
        else:
            bim_ref_df = pd.merge(bim_ref_df, df, on=["Variant"], how="outer", suffixes=("", "_y"))
    bim_ref_df = bim_ref_df.sort_values(by=["Coordinate"])
    return bim_ref_df, bim_list


def load_r(path, M_k, N_k, i_map, M):
    """One cohort's r in the merged marker order (src/main.py:176-191)."""
    if path.endswith(".txt"):
        r_k = np.loadtxt(path).reshape((M_k,))
    elif path.endswith(".npy"):
        r_k = np.load(path).reshape((M_k,))
    elif path.endswith(".linear"):
        import pandas as pd

        df = pd.read_table(path, sep=r"\s+")
        r_k = np.array(df["BETA"], dtype=np.float64).reshape((M_k,))
        r_k[np.isnan(r_k)] = 0
        r_k *= np.sqrt(N_k)
    else:
        raise Exception("Unsupported r vector format!")
    r = np.zeros(M)
    r[np.asarray(i_map, dtype=np.int64)] = r_k
    return r


def load_ld(path, s):
    """One cohort's LD matrix as a BlockLD with ridge s (src/main.py:199-265)."""
    if path.endswith(".npz"):
        import scipy.sparse

        return BlockLD.from_csr(scipy.sparse.load_npz(path), s=s)
    if path.endswith(".npy"):
        R = np.load(path, mmap_mode="r")
        return BlockLD.from_dense(R, s=s)
    if path.endswith(".blocks.json"):
        man = json.load(open(path))
        base = os.path.dirname(os.path.abspath(path))
        files = [f if os.path.isabs(f) else os.path.join(base, f) for f in man["files"]]
        sizes = [int(b) for b in man["block_sizes"]]
        return BlockLD(block_sizes=sizes, loader=lambda b: np.load(files[b], mmap_mode="r"), s=s)
    if path.endswith(".ld"):
        raise Exception("PLINK .ld LD needs every cohort's .ld and .bim: use load_plink_ld_all")
    raise Exception("Unsupported R matrix format!")


def plink_ld_sources(bim_ref, bim_list, N_list):
    """src/main.py:151-162: for cohort k and reference marker i, the cohort k asks
    for marker i (== k: k holds it).  Reproduced as the reference computes it:
    kx = argmax of N over the OTHER cohorts holding the marker is a position in
    that list, used as a cohort id (main.py:161-162), so a marker may be asked of
    a cohort that lacks it (then nothing arrives and r stays 0), or of k itself
    (never requested)."""
    M = len(bim_ref)
    K = len(bim_list)
    idx = {rs: i for i, rs in enumerate(bim_ref)}
    sets = [set(b) for b in bim_list]
    out = []
    for k in range(K):
        source = np.ones(M) * k
        for rs in list(set(bim_ref) - sets[k]):
            idx_rs = [j for j in range(K) if j != k and rs in sets[j]]
            kx = np.argmax(np.array(N_list)[idx_rs])
            source[idx[rs]] = kx
        out.append(source)
    return out


def read_plink_ld(path, idx):
    """One PLINK --r table (columns SNP_A, SNP_B, R): reference-indexed pairs."""
    import pandas as pd

    df = pd.read_table(path, sep=r"\s+")
    indA = [idx[rs] for rs in list(df["SNP_A"])]
    indB = [idx[rs] for rs in list(df["SNP_B"])]
    return indA, indB, list(df["R"])


def load_plink_ld_all(ld_paths, r, bim_ref, bim_list, N_list):
    """All cohorts' .ld files -> (per-cohort scipy CSR R, updated r (K, M)).

    src/main.py:203-257 with the exchange between cohort ranks done in one
    process, in the reference's order: cohort k asks cohort j (j != k) for the
    markers with source[k] == j; j answers with every entry of ITS OWN .ld that
    touches a requested marker -- once per requested endpoint, so a pair whose
    two markers were both requested arrives twice and, summed, doubles -- and
    with its r at those markers; k appends the answers of j = 0..K-1 to its own
    entries and overwrites r[source == j].  R = I + pairs + transposed pairs.

    The reference scans j's whole table once per requested marker
    (O(requests x pairs), main.py:221-225); here one vectorised pass per (k, j)
    selects the same entries in the same order (requested marker ascending,
    then table order; oracle/ldio_oracle.py keeps the loop, tests compare)."""
    import scipy.sparse

    K = len(ld_paths)
    M = len(bim_ref)
    idx = {rs: i for i, rs in enumerate(bim_ref)}
    own = [tuple(np.asarray(a) for a in read_plink_ld(p, idx)) for p in ld_paths]
    own = [(A.astype(np.int64), B.astype(np.int64), C.astype(np.float64)) for A, B, C in own]
    sources = plink_ld_sources(bim_ref, bim_list, N_list)
    r_in = np.asarray(r, dtype=np.float64)
    r_out = r_in.copy()
    mats = []
    for k in range(K):
        parts_a, parts_b, parts_c = [own[k][0]], [own[k][1]], [own[k][2]]
        source = sources[k]
        for j in range(K):
            if j == k or j not in source:
                continue
            req = np.flatnonzero(source == j)
            jA, jB, jC = own[j]
            want = np.zeros(M, dtype=bool)
            want[req] = True
            inA, inB = want[jA], want[jB] & (jB != jA)    # a self pair answers once
            e = np.concatenate([np.flatnonzero(inA), np.flatnonzero(inB)])
            key = np.concatenate([jA[inA], jB[inB]])          # the requested endpoint
            order = np.lexsort((e, key))                      # by marker, then table order
            e = e[order]
            parts_a.append(jA[e])
            parts_b.append(jB[e])
            parts_c.append(jC[e])
            r_out[k][source == j] = r_in[j][req]
        indA, indB, R_col = (np.concatenate(x) for x in (parts_a, parts_b, parts_c))
        ar = np.arange(M)
        ind_r = np.concatenate([ar, indA, indB])
        ind_c = np.concatenate([ar, indB, indA])
        v = np.concatenate([np.ones(M), R_col, R_col])
        mats.append(scipy.sparse.csr_matrix((v, (ind_r, ind_c)), shape=(M, M)))
    return mats, r_out


def load_true_signal(path, M, N):
    if path.endswith(".bin"):
        with open(path, "rb") as f:
            buf = f.read(M * 8)
        x0 = np.array(struct.unpack(str(M) + "d", buf)).reshape((M, 1))
        return x0 * np.sqrt(N)
    if path.endswith(".npy"):
        return np.load(path) * np.sqrt(N)
    raise Exception("Unsupported true signal format!")


# ---------------------------------------------------------------------------
# PLINK 1 .bed panels as an LD source
# ---------------------------------------------------------------------------
BED_MAGIC = b"\x6c\x1b"
BED_A1_COUNT = np.array([2.0, np.nan, 1.0, 0.0])   # value of a 2-bit code (1 = missing)


def _bed_prefix(path):
    return path[:-4] if path.endswith(".bed") else path


class BedPanel:
    """A PLINK 1 .bed/.bim/.fam panel: ``rows`` is a read-only memmap (M,
    ceil(N / 4)) of the SNP-major 2-bit codes, ``N`` the .fam sample count,
    ``ids`` the .bim variant ids (row order).  ``chrom``, ``cm``, ``bp``: the
    .bim's chromosome, genetic-position and base-pair columns as written (row
    order; None where the panel was made without them), read as numbers only by
    positions()."""

    def __init__(self, prefix, rows, N, ids, chrom=None, cm=None, bp=None):
        self.prefix, self.rows, self.N, self.ids = prefix, rows, int(N), list(ids)
        self.chrom, self.cm, self.bp = (None if c is None else list(c) for c in (chrom, cm, bp))
        for name, col in (("chrom", self.chrom), ("cm", self.cm), ("bp", self.bp)):
            if col is not None and len(col) != len(self.ids):
                raise ValueError("%d %s entries for %d variants" % (len(col), name, len(self.ids)))
        self._index = None

    @property
    def M(self):
        return len(self.ids)

    def positions(self, unit, select=None):
        """The ``bp`` or ``cm`` column of the given panel rows (default: all) as
        f64; a value that is not a finite number is a ValueError naming its variant."""
        col = {"bp": self.bp, "cm": self.cm}[unit]
        name = {"bp": "base-pair", "cm": "cM"}[unit]
        if col is None:
            raise ValueError("the panel %s carries no %s positions" % (self.prefix, name))
        rows = range(len(col)) if select is None else [int(i) for i in select]
        out = np.empty(len(rows), dtype=np.float64)
        for k, i in enumerate(rows):
            try:
                out[k] = float(col[i])
                ok = np.isfinite(out[k])
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError("%s.bim: the %s position %r of variant %s is not a number"
                                 % (self.prefix, name, col[i], self.ids[i]))
        return out

    def index_of(self, variants):
        """Panel rows of the given variant ids, in their order; a variant the
        panel lacks is an error that gives the count."""
        if self._index is None:
            self._index = {v: i for i, v in enumerate(self.ids)}
        ix = self._index
        missing = [v for v in variants if v not in ix]
        if missing:
            raise ValueError("%d of %d variant(s) are absent from the panel %s.bim (first: %s)"
                             % (len(missing), len(variants), self.prefix,
                                ", ".join(str(v) for v in missing[:5])))
        return np.array([ix[v] for v in variants], dtype=np.int64)


def read_bed(prefix):
    """Open the panel prefix.bed / .bim / .fam (a path ending in .bed is accepted).
    Only the SNP-major layout is read: magic 6c 1b 01, then per variant ceil(N / 4)
    bytes, sample n in bits 2 (n % 4) of byte n // 4."""
    prefix = _bed_prefix(prefix)
    with open(prefix + ".fam") as f:
        N = sum(1 for line in f if line.strip())
    with open(prefix + ".bim") as f:
        bim = [line.split() for line in f if line.strip()]
    ids = [t[1] for t in bim]
    # chromosome, id, cM, bp: kept as written (a .bim of fewer columns has none)
    chrom, cm, bp = ([t[c] for t in bim] if all(len(t) > c for t in bim) else None
                     for c in (0, 2, 3))
    bed = prefix + ".bed"
    with open(bed, "rb") as f:
        head = f.read(3)
    if len(head) < 3 or head[:2] != BED_MAGIC:
        raise ValueError("%s is not a PLINK 1 .bed file (magic bytes %s, expected 6c 1b)"
                         % (bed, head[:2].hex(" ")))
    if head[2] != 1:
        raise ValueError("%s is in sample-major mode (third byte %02x): only SNP-major .bed "
                         "files (01) are read; convert it with plink --make-bed" % (bed, head[2]))
    if N < 1:
        raise ValueError("%s.fam lists no sample" % prefix)
    M, nb = len(ids), (N + 3) // 4
    size = os.path.getsize(bed)
    if size != 3 + M * nb:
        raise ValueError("%s has %d bytes, expected 3 + %d variants x %d bytes = %d for the %d "
                         "samples of its .fam" % (bed, size, M, nb, 3 + M * nb, N))
    rows = np.memmap(bed, dtype=np.uint8, mode="r", offset=3, shape=(M, nb)) if M else \
        np.zeros((0, nb), dtype=np.uint8)
    return BedPanel(prefix, rows, N, ids, chrom=chrom, cm=cm, bp=bp)


def write_bed(prefix, codes, bim_rows, fam_rows):
    """Write prefix.bed / .bim / .fam.  codes: (M, N) 2-bit PLINK codes (0 hom A1,
    1 missing, 2 het, 3 hom A2); bim_rows / fam_rows: one sequence of the six
    columns (or one ready line) per variant / sample."""
    prefix = _bed_prefix(prefix)
    codes = np.asarray(codes)
    if codes.ndim != 2 or len(bim_rows) != codes.shape[0] or len(fam_rows) != codes.shape[1]:
        raise ValueError("codes must be (len(bim_rows), len(fam_rows))")
    if codes.size and (codes.min() < 0 or codes.max() > 3):
        raise ValueError("codes must be in 0..3")
    M, N = codes.shape
    nb = (N + 3) // 4
    pad = np.zeros((M, nb * 4), dtype=np.uint8)
    pad[:, :N] = codes
    q = pad.reshape(M, nb, 4)
    rows = q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)
    with open(prefix + ".bed", "wb") as f:
        f.write(BED_MAGIC + b"\x01")
        f.write(np.ascontiguousarray(rows, dtype=np.uint8).tobytes())
    for ext, table in ((".bim", bim_rows), (".fam", fam_rows)):
        with open(prefix + ext, "w") as f:
            for row in table:
                f.write((row if isinstance(row, str) else "\t".join(str(x) for x in row)) + "\n")
    return prefix


def bed_codes(rows, N):
    """(n, N) uint8 codes of packed .bed rows (the padding bits dropped)."""
    rows = np.asarray(rows, dtype=np.uint8)
    sh = np.array([0, 2, 4, 6], dtype=np.uint8)
    return ((rows[:, :, None] >> sh) & 3).reshape(rows.shape[0], -1)[:, :N]


def equal_blocks(M, n):
    """M markers in blocks of n, the last one shorter."""
    n = int(n)
    if n < 1:
        raise ValueError("LD block size must be >= 1")
    return [n] * (M // n) + ([M % n] if M % n else [])


class BedLD(BlockLD):
    """Block-diagonal LD whose blocks are marker ranges of a genotype panel:
    R_b = G_b G_b^T with G the per-marker standardised A1 counts / sqrt(N),
    missing genotypes mean-imputed (include/sgvamp_hip.h, "genotype LD source").

    upload() sends only the block's 2-bit rows; the device forms R_b in the
    engine's packing and precision, so a rank reads only its own part of the
    .bed and no matrix exists on the host or on disk.  block() is the same
    definition evaluated on the host in NumPy (n x N doubles and an f64
    product: slow, for checks and for regroup(), which on the same partition
    returns this object and on a coarser one a plain BlockLD whose blocks are
    assembled on the host from block() -- the slow path).  ``select``: panel rows in marker
    order (default: the panel's own order).

    ``window`` (markers of that order, >= 1; None: none): inside each block only
    the entries with |i - j| <= window are kept, everything else is exactly 0
    (include/sgvamp_hip.h, "windowed genotype LD").  The block is then a symmetric
    band of width min(window, n_b - 1): upload() forms it on the device as a
    packed band (the engine's packing must be on), band_cuts() may cut it into
    pieces, and pieces() gives those pieces' couplings as GenoCoupling objects,
    formed on the device from the 2 * window rows next to each cut.  Truncating
    LD to a window does not preserve positive semi-definiteness; the ridge ``s``
    is the remedy -- or ``taper``.

    ``window_kb`` / ``window_cm`` (positive floats): a window by distance, the
    .bim's base-pair column with span D = 1000 window_kb, or its cM column with D =
    window_cm (include/sgvamp_hip.h, "distance-windowed genotype LD").  Marker i
    then reaches hi[i] = max{j >= i : pos[j] - pos[i] <= D} (reach(b), from the
    .bim alone), cut to i + window where ``window`` is given as well; entry (i, j),
    j >= i, is kept iff j <= hi[i].  Positions must not decrease inside a block.
    ``taper`` = "triangle" multiplies every kept entry by 1 - (pos[j] - pos[i]) /
    D, which keeps the windowed block positive semi-definite (the Schur product
    with a positive-definite function), so it needs no ridge.  A taper needs
    exactly one of the three windows; with ``window`` alone the positions are the
    markers' indices in the block and D = window + 1.  The band's width is the
    widest reach, max(hi - i), per block and per piece.

    ``form`` = "stored" (default) forms and stores R_b as above.  "factor" keeps
    the block as its 2-bit rows on the device and every LD pass applies R_b p as
    G_b (G_b^T p) (include/sgvamp_hip.h, "factor LD blocks"): exactly positive
    semi-definite, 2 bits per genotype instead of 8 bytes per pair of markers, so
    an unwindowed block as long as a chromosome fits one GPU.  A factor source has
    no window and no taper (ValueError), no pieces() and no regroup() onto another
    partition (ValueError), and band_width() is None; block() stays the host's
    dense G_b G_b^T, for checks."""

    uses_geno = True
    FORMS = ("stored", "factor")

    def __init__(self, panel, block_sizes, select=None, s=0.0, window=None, window_kb=None,
                 window_cm=None, taper=None, _pos=None, form="stored"):
        if form not in self.FORMS:
            raise ValueError("LD form must be 'stored' or 'factor', not %r" % (form,))
        self.form = form
        if form == "factor":
            given = [n for n, v in (("window", window), ("window_kb", window_kb),
                                    ("window_cm", window_cm), ("taper", check_ld_taper(taper)))
                     if v is not None]
            if given:
                raise ValueError("the factor LD form applies the whole block G_b G_b^T: it takes "
                                 "no %s" % " / ".join(given))
        sizes = [int(b) for b in block_sizes]
        super().__init__(block_sizes=sizes, loader=self._host_block, s=s)
        self.panel = panel
        self.select = None if select is None else np.asarray(select, dtype=np.int64)
        m = panel.M if self.select is None else len(self.select)
        if sum(sizes) != m or any(b < 1 for b in sizes):
            raise ValueError("LD block sizes sum to %d, the panel selection has %d markers"
                             % (sum(sizes), m))
        self._offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.window = check_ld_window(window)
        self.window_kb = check_ld_distance(window_kb, "kb")
        self.window_cm = check_ld_distance(window_cm, "cM")
        self.taper = check_ld_taper(taper)
        given = sum(w is not None for w in (self.window, self.window_kb, self.window_cm))
        if self.taper is not None and given != 1:
            raise ValueError("an LD taper needs exactly one of the windows (markers, kb, cM) as "
                             "its distance: %d given" % given)
        if self.window_kb is not None and self.window_cm is not None:
            raise ValueError("an LD window in kb and one in cM exclude each other")
        # a reach per row (distance window and / or taper); a marker window alone
        # stays on the uniform-window path
        self.by_reach = any(x is not None for x in (self.taper, self.window_kb, self.window_cm))
        self._pos, self._span, self._hi = None, None, {}
        if self.by_reach:
            self._set_positions(_pos)

    def _set_positions(self, pos):
        """Every selected marker's position and the span D; the checks of each
        block's positions (a piece partition takes its parent's, checked there)."""
        if self.window_kb is not None:
            unit, self._span = "bp", 1000.0 * self.window_kb
        elif self.window_cm is not None:
            unit, self._span = "cm", self.window_cm
        else:
            unit, self._span = None, float(self.window + 1)
        if pos is not None:
            self._pos = pos
            return
        if unit is None:    # a tapered marker window: the index in the block
            self._pos = np.concatenate([np.arange(n, dtype=np.float64) for n in self.block_sizes])
            return
        self._pos = self.panel.positions(unit, self.select)
        name = {"bp": "base-pair", "cm": "cM"}[unit]
        for b in range(len(self.block_sizes)):
            p = self._pos[int(self._offs[b]):int(self._offs[b + 1])]
            down = np.flatnonzero(np.diff(p) < 0)
            if len(down):
                ids, k = self.variant_ids(b), int(down[0])
                raise ValueError("LD block %d: the %s positions decrease from %s (%s) to %s (%s); "
                                 "a distance window needs them in order inside every block"
                                 % (b, name, ids[k], repr(float(p[k])), ids[k + 1],
                                    repr(float(p[k + 1]))))
            if unit == "cm" and len(p) > 1 and p[0] == p[-1]:
                raise ValueError("LD block %d: every marker has the cM position %s: %s.bim "
                                 "carries no genetic map, so a window in cM keeps everything"
                                 % (b, repr(float(p[0])), self.panel.prefix))

    def positions(self, b):
        """Block b's positions (by_reach only)."""
        return self._pos[int(self._offs[b]):int(self._offs[b + 1])]

    def reach(self, b):
        """hi (n_b,) int32: hi[i] = max{j : i <= j < n_b, pos[j] - pos[i] <= D}, cut
        to i + window where a marker window is given too.  The predicate is that
        f64 subtraction and comparison: searchsorted on pos + D is a first guess,
        fixed up by testing it at hi and hi + 1."""
        if b not in self._hi:
            p, D = self.positions(b), self._span
            n = len(p)
            i = np.arange(n)
            hi = np.clip(np.searchsorted(p, p + D, side="right") - 1, i, n - 1)
            while True:
                far = (p[hi] - p[i] > D) & (hi > i)
                if not far.any():
                    break
                hi = hi - far
            while True:
                nxt = np.minimum(hi + 1, n - 1)
                near = (hi + 1 < n) & (p[nxt] - p[i] <= D)
                if not near.any():
                    break
                hi = hi + near
            if self.window is not None:
                hi = np.minimum(hi, i + self.window)
            self._hi[b] = hi.astype(np.int32)
        return self._hi[b]

    def _index(self, b):
        o0, o1 = int(self._offs[b]), int(self._offs[b + 1])
        return np.arange(o0, o1) if self.select is None else self.select[o0:o1]

    def _read(self, ix):
        if len(ix) and np.all(np.diff(ix) == 1):   # one contiguous read of the file
            return np.ascontiguousarray(self.panel.rows[int(ix[0]):int(ix[-1]) + 1])
        return np.ascontiguousarray(self.panel.rows[ix])

    def rows(self, b):
        """The block's packed rows, (n_b, ceil(N / 4)) uint8."""
        return self._read(self._index(b))

    def variant_ids(self, b):
        return [self.panel.ids[i] for i in self._index(b)]

    def check_counts(self, b, counts, ids=None, what=None):
        """ValueError naming the block's markers that have no LD (no observed
        sample, or one value among them), from their code counts."""
        c = np.asarray(counts, dtype=np.int64)
        nobs = c[:, 0] + c[:, 2] + c[:, 3]
        s1 = 2 * c[:, 0] + c[:, 2]
        s2 = 4 * c[:, 0] + c[:, 2]
        bad = np.flatnonzero((nobs == 0) | (nobs * s2 - s1 * s1 == 0))
        if len(bad):
            ids = self.variant_ids(b) if ids is None else ids
            raise ValueError("%d marker(s) of %s have no LD (monomorphic among their "
                             "observed samples, or all missing): %s%s"
                             % (len(bad), what or "LD block %d" % b,
                                ", ".join(str(ids[i]) for i in bad[:5]),
                                ", ..." if len(bad) > 5 else ""))

    def _standardise(self, rows, check):
        N = self.panel.N
        codes = bed_codes(rows, N)
        counts = np.stack([(codes == k).sum(axis=1) for k in range(4)], axis=1).astype(np.int64)
        check(counts)
        nobs = counts[:, 0] + counts[:, 2] + counts[:, 3]
        s1 = 2 * counts[:, 0] + counts[:, 2]
        s2 = 4 * counts[:, 0] + counts[:, 2]
        mean = s1.astype(np.float64) / nobs.astype(np.float64)
        sd = np.sqrt((nobs * s2 - s1 * s1).astype(np.float64)
                     / (nobs.astype(np.float64) * nobs.astype(np.float64)))
        x = BED_A1_COUNT[codes]
        G = ((x - mean[:, None]) / sd[:, None]) / np.sqrt(float(N))
        G[codes == 1] = 0.0
        return G, counts

    def standardised(self, b):
        """G_b (n_b, N) on the host, and the code counts."""
        return self._standardise(self.rows(b), lambda counts: self.check_counts(b, counts))

    def _host_block(self, b):
        G, _ = self.standardised(b)
        R = G @ G.T
        if self.by_reach:
            return reach_masked(R, self.reach(b), self.positions(b) if self.taper else None,
                                self._span)
        if self.window is not None:
            i = np.arange(R.shape[0])
            R[np.abs(i[:, None] - i[None, :]) > self.window] = 0.0
        return R

    def block_csr(self, b):
        return None

    def band_width(self, b):
        """min(window, n_b - 1) of a windowed source, the widest reach max(hi - i) of
        a distance-windowed one (from the .bim alone: no genotype is read); None (a
        dense block) without a window."""
        if self.by_reach:
            hi = self.reach(b)
            return int(np.max(hi - np.arange(len(hi))))
        return None if self.window is None else min(self.window, self.block_sizes[b] - 1)

    def symmetric(self, b, A=None):
        return True if self.window is not None or self.by_reach else super().symmetric(b, A)

    def upload(self, eng, ld, b, packed=True):
        """Stage block b's rows on the engine and form R_b there (this rank's
        blocks only; `packed` is the engine's own setting)."""
        if self.form == "factor":     # the staged rows and tables become the block
            if eng.b0 <= b < eng.b1:
                counts = eng.geno_set_block(b, self.rows(b), self.panel.N)
                self.check_counts(b, counts)
                eng.geno_ld_factor(ld, b)
            return
        if self.by_reach and not packed:
            raise ValueError("distance-windowed genotype LD is stored as a packed band: it needs "
                             "LD packing on")
        if self.window is not None and not packed:
            raise ValueError("windowed genotype LD (window %d) is stored as a packed band: "
                             "it needs LD packing on" % self.window)
        if not (eng.b0 <= b < eng.b1):
            return
        counts = eng.geno_set_block(b, self.rows(b), self.panel.N)
        self.check_counts(b, counts)
        if self.by_reach:
            eng.geno_ld_band_reach(ld, b, self.reach(b),
                                   self.positions(b) if self.taper else None, self._span)
        elif self.window is not None:
            eng.geno_ld_band(ld, b, self.window)
        else:
            eng.geno_ld(ld, b)

    def pieces(self, cuts):
        """The same windowed matrix on a finer partition that cuts blocks into
        pieces (sgvamp.BlockLD.pieces): a BedLD of the same panel, order and window
        on the piece partition -- so a rank reads only its own pieces' rows -- and
        {gb: GenoCoupling} between consecutive pieces of one block, nr = min(bw,
        n_gb), nc = min(bw, n_gb+1), bw the block's band width.  A coupling holds
        the panel rows of its halo, not a matrix."""
        sizes = [int(n) for ps in cuts for n in ps]
        if len(sizes) == len(self.block_sizes):
            return self, {}
        if self.form == "factor":
            raise ValueError("a factor LD source has no pieces: its blocks are applied whole")
        if self.window is None and not self.by_reach:
            raise ValueError("a genotype LD source without a window has dense blocks: no pieces")
        # by reach: the pieces keep the original blocks' positions (a tapered marker
        # window's are indices in the original block, so a cut changes no weight) and
        # a piece's reach is the block's, cut at the piece's end
        L = BedLD(self.panel, sizes, select=self.select, s=self.s, window=self.window,
                  window_kb=self.window_kb, window_cm=self.window_cm, taper=self.taper,
                  _pos=self._pos)
        couplings = {}
        k = 0
        for b, ps in enumerate(cuts):
            if len(ps) > 1:
                bw = max(1, self.band_width(b))
                b0 = o = int(self._offs[b])
                for i in range(len(ps) - 1):
                    cut = o + int(ps[i])
                    nr, nc = min(bw, int(ps[i])), min(bw, int(ps[i + 1]))
                    m = np.arange(cut - nr, cut + nc)
                    keep = pos = None
                    if self.by_reach:   # head columns tail row a keeps: up to hi, from the cut on
                        hi = self.reach(b).astype(np.int64) + b0
                        keep = np.clip(hi[cut - nr - b0:cut - b0] - cut + 1, 0, nc)
                        pos = self._pos[m] if self.taper else None
                    couplings[k + i] = GenoCoupling(
                        L, nr, nc, m if self.select is None else self.select[m], keep=keep,
                        pos=pos)
                    o = cut
            k += len(ps)
        return L, couplings

    def regroup(self, sizes):
        """On the same partition this object.  On a coarser one the slow path: a
        plain BlockLD whose blocks are assembled on the host from block() (masked to
        the window inside each original block), each refused where it exceeds the
        dense-block limit."""
        if list(sizes) == list(self.block_sizes):
            return self
        if self.form == "factor":
            raise ValueError("a factor LD source cannot be regrouped onto another partition "
                             "(%d blocks -> %d): no R exists to assemble; give every LD matrix "
                             "of the run the same blocks" % (len(self.block_sizes), len(sizes)))
        L = super().regroup(sizes)
        if self.window is not None or self.by_reach:
            from sgvamp import _dense_guard

            assemble = L._loader

            def load(b):
                _dense_guard(L.block_sizes[b], "genotype LD blocks regrouped on the host")
                return assemble(b)

            L._loader = load
        return L


class GenoCoupling:
    """Coupling between band pieces gb and gb + 1 of a windowed BedLD, kept as the
    panel rows of its halo: ``index`` = the panel rows of gb's last nr markers,
    then of gb + 1's first nc.  C = G_tail G_head^T masked to the window is formed
    on the device (upload); host() is the same in NumPy, for checks.  Of a
    distance-windowed BedLD: ``keep`` (nr,) = the head columns each tail row keeps
    (entry (a, c) iff c < keep[a]) and, with a taper, ``pos`` = the halo rows'
    positions (the weight of (a, c) is 1 - (pos[nr + c] - pos[a]) / D)."""

    def __init__(self, ld, nr, nc, index, keep=None, pos=None):
        self.ld, self.nr, self.nc = ld, int(nr), int(nc)
        self.index = np.asarray(index, dtype=np.int64)
        if len(self.index) != self.nr + self.nc:
            raise ValueError("a %d x %d coupling needs %d halo rows, not %d"
                             % (self.nr, self.nc, self.nr + self.nc, len(self.index)))
        self.keep = None if keep is None else np.asarray(keep, dtype=np.int32)
        self.pos = None if pos is None else np.asarray(pos, dtype=np.float64)
        if self.keep is not None and len(self.keep) != self.nr:
            raise ValueError("a %d x %d coupling needs %d kept-column counts, not %d"
                             % (self.nr, self.nc, self.nr, len(self.keep)))
        if self.pos is not None and (self.keep is None or len(self.pos) != self.nr + self.nc):
            raise ValueError("a tapered %d x %d coupling needs its kept-column counts and %d halo "
                             "positions" % (self.nr, self.nc, self.nr + self.nc))

    def rows(self):
        """The halo's packed rows, (nr + nc, ceil(N / 4)) uint8."""
        return self.ld._read(self.index)

    def variant_ids(self):
        return [self.ld.panel.ids[i] for i in self.index]

    def _check(self, gb, counts):
        self.ld.check_counts(None, counts, ids=self.variant_ids(),
                             what="the coupling between LD band pieces %d and %d" % (gb, gb + 1))

    def host(self, gb=0):
        G, _ = self.ld._standardise(self.rows(), lambda counts: self._check(gb, counts))
        C = G[:self.nr] @ G[self.nr:].T
        a, c = np.arange(self.nr)[:, None], np.arange(self.nc)[None, :]
        if self.keep is not None:
            if self.pos is not None:
                w = 1.0 - (self.pos[self.nr:][None, :] - self.pos[:self.nr][:, None]) / self.ld._span
                C = C * w
            return np.where(c < self.keep[:, None], C, 0.0)
        C[c + self.nr - a > self.ld.window] = 0.0
        return C

    def upload(self, eng, ld, gb):
        """Register the coupling on the engine (every rank, every coupling: the
        rows are read only where the rank owns one of the two pieces)."""
        if self.keep is not None:
            eng.geno_coupling_reach(ld, gb, self.nr, self.nc, self.rows, self.ld.panel.N,
                                    self.keep, self.pos, self.ld._span,
                                    check=lambda counts: self._check(gb, counts))
            return
        eng.geno_coupling(ld, gb, self.nr, self.nc, self.rows, self.ld.panel.N, self.ld.window,
                          check=lambda counts: self._check(gb, counts))


def check_ld_window(window):
    """An LD window as a positive int (None: no window); ValueError otherwise."""
    if window is None:
        return None
    try:
        w = int(window)
        ok = w >= 1 and w == window
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("the LD window must be a positive number of markers, not %r" % (window,))
    return w


def check_ld_distance(x, unit):
    """An LD window by distance as a positive finite float (None: none)."""
    if x is None:
        return None
    try:
        v = float(x)
        ok = np.isfinite(v) and v > 0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("the LD window in %s must be a positive number, not %r" % (unit, x))
    return v


LD_TAPERS = ("none", "triangle")


def check_ld_taper(taper):
    """"triangle" or None (given as None or "none"); ValueError otherwise."""
    if taper is None or taper == "none":
        return None
    if taper not in LD_TAPERS:
        raise ValueError("the LD taper must be one of %s, not %r" % (", ".join(LD_TAPERS), taper))
    return taper


def reach_masked(R, hi, pos=None, span=None):
    """The distance-windowed block of a symmetric R (include/sgvamp_hip.h): for j
    >= i the entry (i, j) where j <= hi[i], times 1.0 - (pos[j] - pos[i]) / span
    where pos is given, exactly 0.0 elsewhere; the lower triangle its mirror."""
    n = R.shape[0]
    i = np.arange(n)
    up = (i[None, :] >= i[:, None]) & (i[None, :] <= np.asarray(hi)[:, None])
    U = np.asarray(R, dtype=np.float64)
    if pos is not None:
        p = np.asarray(pos, dtype=np.float64)
        U = U * (1.0 - (p[None, :] - p[:, None]) / float(span))
    U = np.where(up, U, 0.0)
    return U + np.triu(U, 1).T


def chromosome_blocks(panel, select=None):
    """LD block sizes, one block per run of equal chromosome code in the run's
    marker order (``select``: panel rows in that order; default the panel's own)."""
    if panel.chrom is None:
        raise ValueError("the panel %s carries no chromosome column" % panel.prefix)
    chrom = panel.chrom if select is None else [panel.chrom[int(i)] for i in select]
    sizes = []
    for k, c in enumerate(chrom):
        if k and c == chrom[k - 1]:
            sizes[-1] += 1
        else:
            sizes.append(1)
    return sizes


def load_bed_ld(path, s, block_size=None, blocks_file=None, variants=None, window=None,
                window_kb=None, window_cm=None, taper=None, chr_blocks=False, form="stored"):
    """A .bed panel as a BedLD: blocks of block_size markers (the last shorter),
    the sizes listed one per line in blocks_file, or (chr_blocks) one block per
    run of equal chromosome code; variants: the marker order as variant ids
    (default: the panel's own); window: keep only LD within that many markers of
    the diagonal, as packed bands; window_kb / window_cm: within that distance by
    the .bim's positions; taper: "triangle"; form: "stored" or "factor" (BedLD)."""
    panel = read_bed(path)
    select = None if variants is None else panel.index_of(list(variants))
    M = panel.M if select is None else len(select)
    if chr_blocks:
        sizes = chromosome_blocks(panel, select)
    elif blocks_file is not None:
        with open(blocks_file) as f:
            sizes = [int(t) for t in f.read().split()]
        if sum(sizes) != M:
            raise ValueError("%s lists blocks of %d markers in all, the LD has %d"
                             % (blocks_file, sum(sizes), M))
    else:
        sizes = equal_blocks(M, block_size)
    return BedLD(panel, sizes, select=select, s=s, window=window, window_kb=window_kb,
                 window_cm=window_cm, taper=taper, form=form)
