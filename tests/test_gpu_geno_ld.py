"""LD blocks, r and g from PLINK .bed genotypes on the device (geno.hip) against
the NumPy restatement tests/bed_ref.py.

Block sizes [50, 130, 257, 700] cross the 64-row tile and the 256-row panel
edges; N in {5, 130, 500, 1027}: less than one 16-sample word, N % 4 = 2, a
multiple of 4 but not of 16, N % 16 = 3.  Allele frequencies in [0.05, 0.5],
missing rates 0 and 3 %; every marker of a drawn panel has LD (bed_ref.draw_codes;
N = 5 selects the usable markers of an oversampled draw).

Tolerance of R, r, g: maxrel < 1e-12, the bar test_synth_generator_vs_oracle
sets for the same contraction (the NumPy product and a sample-sequential f64 sum
both stay within 2.4e-14 of an extended-precision product at N <= 1027)."""
import functools
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import hip_backend as hb
from engine import Engine
from ldio import BedLD, read_bed, write_bed

from tests import bed_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [50, 130, 257, 700]
OFFS = np.concatenate([[0], np.cumsum(SIZES)])
NS = [5, 130, 500, 1027]
MISS = [0.0, 0.03]
TOL = 1e-12


def maxrel(a, b):
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


def W(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def panel(N, miss):
    """The case's codes per block and their reference R, computed once."""
    codes = bed_ref.draw_codes(sum(SIZES), N, miss=miss, seed=1000 + N)
    assert not bed_ref.unusable(codes).any()
    if miss:
        assert (codes == 1).any()
    blocks = [codes[OFFS[b]:OFFS[b + 1]] for b in range(len(SIZES))]
    for c in blocks:
        c.setflags(write=False)
    R = [bed_ref.R(c) for c in blocks]
    for r in R:
        r.setflags(write=False)
    return blocks, R


def stage(eng, blocks):
    """geno_set_block of every block: the counts."""
    N = blocks[0].shape[1]
    return [eng.geno_set_block(b, bed_ref.pack(c), N) for b, c in enumerate(blocks)]


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "dense"])
@pytest.mark.parametrize("miss", MISS)
@pytest.mark.parametrize("N", NS)
def test_counts_and_ld_blocks(N, miss, packed):
    blocks, Rref = panel(N, miss)
    eng = Engine(SIZES, K=1)
    try:
        eng.set_ld_packing(packed)
        for b, cnt in enumerate(stage(eng, blocks)):
            assert cnt.dtype == np.int64
            np.testing.assert_array_equal(cnt, bed_ref.counts(blocks[b]))
            assert (cnt.sum(axis=1) == N).all()        # padding bits are not samples
        for b in range(len(SIZES)):
            assert eng.ld_block_format(0, b) == -1
            eng.geno_ld(0, b)
            assert eng.ld_block_format(0, b) == (1 if packed else 0)
            assert eng.ld_block_precision(0, b) == 64
        for b in range(len(SIZES)):      # (a block is read back once the matrix is whole)
            R = eng.get_ld_block(0, b)
            err = maxrel(R, Rref[b])
            print("N=%d miss=%g packed=%d block %d: maxrel %.3e" % (N, miss, packed, b, err))
            assert err < TOL, (b, err)
            np.testing.assert_array_equal(R, R.T)
            nobs = bed_ref.moments(blocks[b])[0]
            assert np.max(np.abs(np.diag(R) - nobs / N)) < 1e-12
    finally:
        eng.close()


@pytest.mark.parametrize("N", [5, 130, 1027])
def test_padding_bits_and_row_stride_ignored(N):
    """Rows longer than ceil(N / 4) bytes and padding positions holding every
    code: the same counts, tables and blocks as the clean rows."""
    blocks, _ = panel(N, 0.03)
    got = {}
    for pad in (0, 1, 2, 3):
        eng = Engine(SIZES[:2], K=1)
        try:
            nb = (N + 3) // 4 + (pad % 2) * 3
            cnt = [eng.geno_set_block(b, bed_ref.pack(blocks[b], row_bytes=nb, pad_bits=pad), N)
                   for b in range(2)]
            for b in range(2):
                np.testing.assert_array_equal(cnt[b], bed_ref.counts(blocks[b]))
                eng.geno_ld(0, b)
            got[pad] = [eng.get_ld_block(0, b) for b in range(2)]
        finally:
            eng.close()
    for pad in (1, 2, 3):
        for b in range(2):
            np.testing.assert_array_equal(got[pad][b], got[0][b])


@pytest.mark.parametrize("N,miss", [(500, 0.03), (1027, 0.0)])
def test_f32_storage_rounds_on_store(N, miss):
    """The f32 engine's stored blocks are float32(round) of the f64 engine's, bit
    for bit (as test_f32_generator_rounds_on_store for the synthetic generator)."""
    blocks, _ = panel(N, miss)
    got = {}
    for bits in (64, 32):
        eng = Engine(SIZES, K=1)
        try:
            eng.set_ld_precision(bits)
            stage(eng, blocks)
            for b in range(len(SIZES)):
                eng.geno_ld(0, b)
            assert [eng.ld_block_precision(0, b) for b in range(len(SIZES))] == [bits] * len(SIZES)
            got[bits] = [eng.get_ld_block(0, b) for b in range(len(SIZES))]
        finally:
            eng.close()
    for b in range(len(SIZES)):
        assert not np.array_equal(got[64][b], W(got[64][b]))
        np.testing.assert_array_equal(got[32][b], W(got[64][b]))


@pytest.mark.parametrize("miss", MISS)
@pytest.mark.parametrize("N", NS)
def test_geno_r_and_g(N, miss):
    blocks, _ = panel(N, miss)
    M = sum(SIZES)
    rs = np.random.RandomState(N)
    y = rs.normal(size=N)
    beta = np.zeros(M)
    idx = rs.choice(M, M // 3, replace=False)
    beta[idx] = rs.normal(size=len(idx))
    eng = Engine(SIZES, K=2)
    try:
        stage(eng, blocks)
        eng.geno_r(1, y)
        r = eng.get_vector(hb.VEC_R, 1)
        g = eng.geno_g(beta, N)
    finally:
        eng.close()
    assert g.shape == (len(SIZES), N)
    for b, c in enumerate(blocks):
        sl = slice(OFFS[b], OFFS[b + 1])
        er = maxrel(r[sl], bed_ref.r(c, y))
        eg = maxrel(g[b], bed_ref.g(c, beta[sl]))
        print("N=%d miss=%g block %d: r maxrel %.3e, g maxrel %.3e" % (N, miss, b, er, eg))
        assert er < TOL and eg < TOL, (b, er, eg)


def test_unusable_marker_refused_nothing_stored(tmp_path):
    """A monomorphic marker: geno_set_block reports it in the counts, geno_ld is a
    state error and leaves the block unset; the other block is stored.  BedLD
    raises the ValueError naming the variant before any block is stored."""
    N = 130
    blocks, _ = panel(N, 0.03)
    bad = np.array(blocks[1])
    bad[17] = 3                      # homozygous A2 everywhere
    bad[40, :] = 1                   # and one never observed
    eng = Engine(SIZES[:2], K=1)
    try:
        cnt = [eng.geno_set_block(0, bed_ref.pack(blocks[0]), N),
               eng.geno_set_block(1, bed_ref.pack(bad), N)]
        np.testing.assert_array_equal(cnt[1], bed_ref.counts(bad))
        assert cnt[1][17].tolist() == [0, 0, 0, N] and cnt[1][40].tolist() == [0, N, 0, 0]
        assert eng.ld_block_format(0, 1) == -1
        with pytest.raises(hb.HipError, match=r"\(-4\).*2 marker\(s\) without LD"):
            eng.geno_ld(0, 1)
        assert eng.ld_block_format(0, 1) == -1
        with pytest.raises(hb.HipError, match=r"\(-4\)"):
            eng.geno_r(0, np.zeros(N))
        eng.geno_ld(0, 0)
        assert eng.ld_block_format(0, 0) == 1
        eng.geno_clear()
        with pytest.raises(hb.HipError, match=r"\(-4\)"):
            eng.geno_ld(0, 0)
        with pytest.raises(hb.HipError, match=r"\(-2\)"):
            eng.ctx.sgv_geno_set_block(0, bed_ref.pack(blocks[0]).ctypes.data_as(hb._c_u8_p),
                                       (N + 3) // 4 - 1, N, cnt[0].ctypes.data_as(hb._c_i64_p))
    finally:
        eng.close()
    codes = np.concatenate([blocks[0], bad])
    prefix = write_bed(str(tmp_path / "p"), codes, *bed_ref.bim_fam(codes.shape[0], N))
    L = BedLD(read_bed(prefix), SIZES[:2])
    eng = Engine(SIZES[:2], K=1)
    try:
        L.upload(eng, 0, 0)
        with pytest.raises(ValueError, match=r"2 marker\(s\) of LD block 1 have no LD.*rs67, rs90"):
            L.upload(eng, 0, 1)
        assert [eng.ld_block_format(0, b) for b in range(2)] == [1, -1]
    finally:
        eng.close()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_one_rank_vs_two_ranks_bitwise():
    """tests/test_gpu_multirank.py's harness (ranks on one device, host exchange):
    two ranks, each forming only its own blocks from its own rows of the .bed,
    store the same blocks and write the same 5-iteration xhat / r1 files as one
    rank, bit for bit (tools/geno_ranks_gpu.py)."""
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2",
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), SGV_EXCHANGE="host")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tools", "geno_ranks_gpu.py")],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                      text=True))
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(out)
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, out[-4000:])
    assert "bitwise equal -> OK" in outs[0], outs[0][-3000:]


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_cli_bed_equals_manifest_of_its_blocks(tmp_path, precision):
    """simulate.py --bed on a 900-marker, N = 500 panel, then main.py on the .bed
    (K = 2 cohorts sharing it, blocks [130, 257, 513], 5 iterations) and on a
    *.blocks.json manifest of the same blocks fetched with get_ld_block: every
    output file byte-identical."""
    import main
    import simulate

    M, N, sizes = 900, 500, [130, 257, 513]
    codes = bed_ref.draw_codes(M, N, miss=0.03, seed=77)
    prefix = write_bed(str(tmp_path / "p"), codes, *bed_ref.bim_fam(M, N))
    simulate.main(["--bed", prefix, "--out", str(tmp_path / "sim"), "--h2", "0.8", "--lam", "0.1",
                   "--seed", "3"])
    y = np.load(tmp_path / "sim_phen.npy")
    beta = np.load(tmp_path / "sim_bet.npy")
    r = np.load(tmp_path / "sim_r.npy")
    assert y.shape == (N, 1) and beta.shape == (M, 1) and r.shape == (M, 1)
    assert np.count_nonzero(beta) == int(M * 0.1)
    assert maxrel(r[:, 0], bed_ref.r(codes, y[:, 0])) < TOL
    w = y[:, 0] - bed_ref.g(codes, beta[:, 0])         # the noise the simulator added
    assert abs(np.var(w) - 0.2) < 0.05 and abs(np.mean(w)) < 0.1
    (tmp_path / "sizes.txt").write_text("".join("%d\n" % n for n in sizes))

    def run(ld, out, extra):
        (tmp_path / out).mkdir()
        main.main(["--ld-files", "%s,%s" % (ld, ld), "--r-files",
                   "%s,%s" % (tmp_path / "sim_r.npy", tmp_path / "sim_r.npy"),
                   "--true-signal-file", str(tmp_path / "sim_bet.npy"), "--out-dir",
                   str(tmp_path / out), "--out-name", "run", "--N", "%d,%d" % (N, N), "--M",
                   "%d,%d" % (M, M), "--K", "2", "--iterations", "5", "--seed", "11",
                   "--prior-probs", "0.9,0.1", "--ld-precision", precision] + extra)
        return {fn: open(tmp_path / out / fn, "rb").read()
                for fn in sorted(os.listdir(tmp_path / out))}

    a = run(prefix + ".bed", "bed", ["--ld-blocks", str(tmp_path / "sizes.txt")])
    L = BedLD(read_bed(prefix), sizes)
    eng = Engine(sizes, K=1)
    try:
        eng.set_ld_precision(32 if precision == "f32" else 64)
        files = []
        for b in range(len(sizes)):
            L.upload(eng, 0, b)
        for b in range(len(sizes)):
            np.save(tmp_path / ("blk%d.npy" % b), eng.get_ld_block(0, b))
            files.append("blk%d.npy" % b)
    finally:
        eng.close()
    with open(tmp_path / "R.blocks.json", "w") as f:
        json.dump({"block_sizes": sizes, "files": files}, f)
    b = run(str(tmp_path / "R.blocks.json"), "man", [])
    assert a.keys() == b.keys()
    assert sum(fn.endswith(".bin") for fn in a) == 5 * 3 and "run_metrics.csv" in a
    for fn in a:
        assert a[fn] == b[fn], fn
    x = np.frombuffer(a["run_xhat_it_4.bin"])
    assert np.isfinite(x).all() and x.any()
