"""The factor LD form, host side (no GPU): the premise of the exact-arithmetic GPU
test (tests/factor_panels.py, checked here with tests/bed_ref.py), BedLD's and
main.py's refusals, what upload() asks of an engine, the binding, and the rule
that the pass-form model stays as it was."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hip_backend as hb
from ldio import BedLD, load_bed_ld, read_bed, write_bed

from tests import bed_ref
from tests import exact_ld as xl
from tests import factor_panels as fp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the exact panels' premise -----------------------------------------------------
@pytest.mark.parametrize("N", fp.EXACT_NS)
def test_exact_panel_premise(N):
    """sqrt(N) G is exactly {-2, -1, 0, 1, 2}, no marker is unusable, both n_obs and
    both kinds occur, and with integer |p| <= 1023 at n_b = 300 the two-stage product
    G (G^T p), the stored form's R p and the int64 result agree bit for bit, |N q| <
    2**21."""
    n = 300
    codes = fp.exact_codes(n, N, 5)
    assert not bed_ref.unusable(codes).any()
    gi = fp.scaled_G(codes)
    nobs = bed_ref.moments(codes)[0]
    assert set(nobs.tolist()) == {N, N // 2}
    assert (codes == 1).sum(axis=1).tolist() == (N - nobs).tolist()
    assert (np.abs(gi).max(axis=1) == 1).any() and (np.abs(gi).max(axis=1) == 2).any()
    mean, sd = bed_ref.mean_sd(codes)
    assert set(mean.tolist()) == {1.0} and set(sd.tolist()) == {1.0, 0.5}
    V = xl.exact_rhs(16, n, fp.RHS_BITS, 9)
    assert np.abs(V).max() <= 1023
    ref, RA = fp.exact_reference([codes], V)
    G = bed_ref.G(codes)
    np.testing.assert_array_equal((G @ (G.T @ V.T)).T, ref)      # the factor form's two stages
    np.testing.assert_array_equal(V @ bed_ref.R(codes).T, ref)   # the stored form's R p
    assert np.abs(ref * N).max() < 2 ** 21
    # the epilogue's grid: out, yout and the dots of the GPU test are exact in any order
    c1, c2 = xl.narrow_coeffs(16)
    W = xl.exact_weights(16, n, 3, 10)
    xl.check_exact(None, V, c1, c2, N.bit_length() - 1, w=W, ys=(xl.YS1, xl.YS0), RA=RA)


# ---- BedLD ---------------------------------------------------------------------------
def small_panel(tmp_path, M=12, N=20):
    codes = bed_ref.draw_codes(M, N, miss=0.05, seed=4)
    bim = [("1", "rs%d" % i, str(0.1 * i), str(1000 * (i + 1)), "A", "G") for i in range(M)]
    prefix = write_bed(str(tmp_path / "p"), codes, bim, bed_ref.bim_fam(M, N)[1])
    return prefix, codes


def test_bedld_factor_refusals(tmp_path):
    prefix, codes = small_panel(tmp_path)
    panel = read_bed(prefix)
    for kw, word in ((dict(window=3), "window"), (dict(window_kb=2.0), "window_kb"),
                     (dict(window_cm=0.3), "window_cm"),
                     (dict(window=3, taper="triangle"), "window / taper")):
        with pytest.raises(ValueError, match="factor LD form.*no %s" % word):
            BedLD(panel, [5, 7], form="factor", **kw)
    with pytest.raises(ValueError, match="'stored' or 'factor', not 'lowrank'"):
        BedLD(panel, [5, 7], form="lowrank")
    L = BedLD(panel, [5, 7], form="factor", taper="none")      # main.py's "no taper"
    assert L.form == "factor" and L.uses_geno
    assert L.band_width(0) is None and L.band_width(1) is None
    assert L.regroup([5, 7]) is L and L.pieces([[5], [7]]) == (L, {})
    with pytest.raises(ValueError, match="factor LD source cannot be regrouped"):
        L.regroup([12])
    with pytest.raises(ValueError, match="factor LD source has no pieces"):
        L.pieces([[5], [3, 4]])
    # block() stays the definition on the host, for checks
    assert np.max(np.abs(L.block(1) - bed_ref.R(codes[5:]))) < 1e-12


class FakeEngine:
    """Records what upload() asks for; owns blocks [b0, b1)."""

    def __init__(self, codes, sizes, b0, b1):
        self.codes, self.offs = codes, np.concatenate([[0], np.cumsum(sizes)])
        self.b0, self.b1, self.calls = b0, b1, []

    def geno_set_block(self, b, rows, nsamp):
        self.calls.append(("set", b, rows.shape, nsamp))
        return bed_ref.counts(self.codes[self.offs[b]:self.offs[b + 1]])

    def geno_ld(self, ld, b):
        self.calls.append(("ld", ld, b))

    def geno_ld_factor(self, ld, b):
        self.calls.append(("factor", ld, b))


def test_upload_hands_over_and_default_is_the_stored_source(tmp_path):
    """upload() of a factor source stages the block and hands it over, on the
    owning rank only; --ld-form stored builds the BedLD no flag builds, which
    uploads through geno_ld as before."""
    import main

    prefix, codes = small_panel(tmp_path)
    sizes = [5, 7]
    F = load_bed_ld(prefix + ".bed", 0.0, block_size=None, blocks_file=None, form="factor",
                    chr_blocks=True)
    assert F.form == "factor" and F.block_sizes == [12]
    F = BedLD(read_bed(prefix), sizes, form="factor")
    eng = FakeEngine(codes, sizes, 1, 2)
    for b in range(2):
        F.upload(eng, 3, b)
    assert eng.calls == [("set", 1, (7, 5), 20), ("factor", 3, 1)]

    base = ["--ld-files", prefix + ".bed", "--ld-block-size", "5", "--r-files", "r.npy", "--N", "20",
            "--M", "12", "--out-dir", str(tmp_path), "--out-name", "x"]
    parser = main.build_parser()
    made = []
    for extra in ([], ["--ld-form", "stored"]):
        args = parser.parse_args(base + extra)
        main.check_bed_flags(parser, args)
        main.check_ld_form(parser, args)
        assert args.ld_form == "stored"
        L = load_bed_ld(prefix + ".bed", 0.0, block_size=args.ld_block_size,
                        blocks_file=args.ld_blocks, taper=args.ld_taper,
                        chr_blocks=args.ld_chr_blocks, form=args.ld_form)
        eng = FakeEngine(codes, [5, 5, 2], 0, 3)
        for b in range(3):
            L.upload(eng, 0, b)
        made.append((L.form, L.block_sizes, L.window, L.window_kb, L.window_cm, L.taper, L.by_reach,
                     L.s, eng.calls))
    assert made[0] == made[1]
    assert made[0][0] == "stored" and [c[0] for c in made[0][-1]] == ["set", "ld"] * 3
    assert BedLD(read_bed(prefix), sizes).form == "stored"


# ---- main.py -------------------------------------------------------------------------
def test_main_refusals_in_child_processes(tmp_path):
    """Every combination --ld-form factor refuses, each with its message: fresh
    child processes (started together), argparse's exit code 2, before any file
    is opened or any device touched."""
    base = [sys.executable, os.path.join(ROOT, "sgvamp-py_amd", "main.py"), "--r-files", "r.npy",
            "--N", "10", "--M", "10", "--out-dir", str(tmp_path), "--out-name", "x",
            "--ld-form", "factor"]
    bed = ["--ld-files", "p.bed", "--ld-block-size", "5"]
    cases = [
        (["--ld-files", "R.npz"], "needs a .bed LD source for every cohort: R.npz is not one"),
        (["--ld-files", "p.bed,R.blocks.json", "--ld-block-size", "5", "--K", "2"],
         "needs a .bed LD source for every cohort: R.blocks.json is not one"),
        (bed + ["--ld-precision", "f32"], "cannot be combined with --ld-precision f32"),
        (bed + ["--ld-packing", "off"], "cannot be combined with --ld-packing off"),
        (bed + ["--ld-window", "5"], "cannot be combined with --ld-window"),
        (bed + ["--ld-window-kb", "5"], "cannot be combined with --ld-window-kb"),
        (bed + ["--ld-window-cm", "0.5"], "cannot be combined with --ld-window-cm"),
        (bed + ["--ld-window", "5", "--ld-taper", "triangle"], "cannot be combined with --ld-"),
        (["--ld-files", "p.bed", "--ld-block-size", "5", "--ld-form", "lowrank"], "invalid choice"),
    ]
    procs = [subprocess.Popen(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                              text=True, cwd=str(tmp_path)) for extra, _ in cases]
    for p, (extra, msg) in zip(procs, cases):
        _, err = p.communicate(timeout=120)
        assert p.returncode == 2, (extra, p.returncode, err[-2000:])
        assert msg in err and "--ld-form" in err, (extra, err[-2000:])


# ---- the binding, and the model left alone ---------------------------------------
def test_binding_exports_the_call_and_names_the_kind():
    assert "sgv_geno_ld_factor" in hb.EXPORTS
    assert hb.PASS_KINDS.index("factor") == 7
    assert hasattr(hb.load(), "sgv_geno_ld_factor")
    text = open(os.path.join(ROOT, "include", "sgvamp_hip.h")).read()
    assert "#define SGV_KIND_FACTOR 7" in text and "int sgv_geno_ld_factor(" in text


def test_pass_form_model_is_unchanged():
    """sgv_pass_form_model knows nothing of the factor form: one sample shape gives
    what it gave before (recorded from the parent commit), and no input makes it
    answer "factor"."""
    shape = {"packed": 1, "wide": 1, "pair": 1, "ngrp": 4, "wide_ngrp": 2}
    want = {
        1: ("valu", 0, "none", 0, 0, 0, False, False, False, False, False, False),
        2: ("valu", 0, "none", 0, 0, 0, False, False, False, False, False, False),
        4: ("wide", -1, "none", 1, 0, 4, False, False, True, False, False, True),
        8: ("wide", -1, "none", 1, 0, 8, True, False, True, False, False, True),
        12: ("strip16", -1, "none", 1, 4, 16, False, False, True, False, True, False),
    }
    for ncol, w in want.items():
        assert tuple(hb.pass_form_model(shape, {}, 3, ncol)) == w, ncol
    for sh in ({}, {"dense": 1}, {"packed": 1}, {"packed": 1, "walks": 1, "ragged": 1},
               {"packed": 1, "bits": 32}):
        for ncol in range(1, 17):
            f = hb.pass_form_model(sh, {}, 3, ncol)
            assert f.kind != "factor" and f.rest_kind != "factor"
    assert len(hb.PASS_FORM_FIELDS) == 12 and len(hb.PLAN_SHAPE_FIELDS) == 14 \
        and len(hb.PASS_SWITCHES) == 7
