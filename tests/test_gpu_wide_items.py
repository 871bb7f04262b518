"""The wide strip form of the MFMA pass (k_sym_mfma_wide, sym_mfma.hip):
1,024-column items on dense-triangle blocks, eight waves of 128 columns per
strip, row sums combined through an LDS hand-off ring.

Its summation order differs from the 512-column forms', so its bits do; what
must hold is the project's bar for every LD kernel (1e-12 relative to numpy),
that a block's sums depend on the block alone, the default selection (3-8
columns wide, 9-16 columns on the 512-column forms) and repeatability.
"""
import contextlib
import os

import numpy as np
import pytest

from engine import Engine
from oracle import vamp_oracle as vo

pytestmark = pytest.mark.gpu

RIDGE = 0.1
# 8500 = 34 panels: two column classes have 9 panels, so their chunks get an
# 8 + 1-panel strip pair; the small blocks put the ragged chunk end on, just
# past and far before wave (128-column) boundaries, with most waves idle
SIZES = [8500, 1281, 1025, 513, 257, 1]
NCOLS = [3, 4, 5, 8]
FORCED = {"SGV_AB": "1", "SGV_MF_WIDE": "1"}


def maxrel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


_blocks = {}


def block(n):
    """Exactly symmetric random n x n block (entries ~ N(0, 1/n)); one per size."""
    if n not in _blocks:
        A = np.random.RandomState(1000 + n).standard_normal((n, n)) / np.sqrt(n)
        U = np.triu(A)
        _blocks[n] = U + np.triu(A, 1).T
    return _blocks[n]


_vecs = {}


def vec(n, ncol):
    """The right-hand sides of block n for an ncol-column product."""
    if (n, ncol) not in _vecs:
        _vecs[(n, ncol)] = np.random.RandomState(7 * n + ncol).normal(size=(ncol, n))
    return _vecs[(n, ncol)]


@contextlib.contextmanager
def environ(env):
    keys = ("SGV_AB", "SGV_MF_WIDE", "SGV_MF_PAIR", "SGV_MF_WIDE_IDLE")
    old = {k: os.environ.get(k) for k in keys}
    try:
        for k in keys:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k in keys:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def products(sizes, ncols, env, repeat=1, kinds=("wide",)):
    """{ncol: [Y, ...]}: `repeat` products per column count on a fresh engine
    holding block(n) for n in sizes, under the A/B switches `env`; every pass
    reports one of the packed `kinds` up to 8 columns, the 16x16x4 strips above."""
    with environ(env):
        eng = Engine(sizes, K=1)
        for b, n in enumerate(sizes):
            eng.set_ld_block(0, b, block(n))
        eng.set_ridge(RIDGE)
        out = {}
        for ncol in ncols:
            V = np.concatenate([vec(n, ncol) for n in sizes], axis=1)
            form = eng.ld_pass_form(0, ncol)
            assert form.kind in (kinds if ncol <= 8 else ("strip16",)), (env, ncol, form)
            assert form.idle_exit == (form.kind == "wide"), form
            out[ncol] = [np.array(eng.ld_matvec(0, V)) for _ in range(repeat)]
        eng.close()
    return out


_forced = {}


def forced_wide():
    """Two forced-wide products per column count on the SIZES engine (shared)."""
    if not _forced:
        _forced.update(products(SIZES, NCOLS, FORCED, repeat=2))
    return _forced


@pytest.mark.parametrize("ncol", NCOLS)
def test_wide_vs_numpy(ncol):
    """Every column of the forced-wide product within 1e-12 relative of numpy."""
    Y = forced_wide()[ncol][0]
    L = vo.BlockLD([block(n) for n in SIZES], s=RIDGE)
    V = np.concatenate([vec(n, ncol) for n in SIZES], axis=1)
    for j in range(ncol):
        err = maxrel(Y[j], L.matvec_Rs(V[j]))
        print("ncol=%d column %d: maxrel %.3e" % (ncol, j, err))
        assert err < 1e-12, (ncol, j, err)


def test_wide_function_of_block_alone():
    """The 1281-marker block's sums are bitwise the same whatever else the
    engine holds and wherever the block sits."""
    alone = products([1281], NCOLS, FORCED)
    for sizes in ([8500, 1281, 513], [513, 1281, 8500]):
        got = products(sizes, NCOLS, FORCED)
        o = sum(sizes[:sizes.index(1281)])
        for ncol in NCOLS:
            np.testing.assert_array_equal(got[ncol][0][:, o:o + 1281], alone[ncol][0])


def test_wide_default_selection():
    """No switches: 8 columns take the wide form, 16 columns the 512-column one.
    The two forms add a row's terms in different orders, so over thousands of
    terms their bits differ: the forced arms are not one kernel twice."""
    sizes = [2600, 1281]
    default = products(sizes, [8, 16], {})
    wide = products(sizes, [8], FORCED)
    narrow = products(sizes, [8, 16], {"SGV_AB": "1", "SGV_MF_WIDE": "0"},
                      kinds=("strip4", "pair"))   # either 512-column kernel: bitwise one product
    np.testing.assert_array_equal(default[8][0], wide[8][0])
    np.testing.assert_array_equal(default[16][0], narrow[16][0])
    assert not np.array_equal(wide[8][0], narrow[8][0])


class UpperCsr:
    """The upper triangle of a dense block as CSR arrays (Engine.set_ld_block_csr)."""

    def __init__(self, B, bw):
        n = B.shape[0]
        self.shape = B.shape
        cols = [np.arange(i, min(n, i + bw + 1)) for i in range(n)]
        self.indptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])])
        self.indices = np.concatenate(cols)
        self.data = np.concatenate([B[i, c] for i, c in enumerate(cols)])


def test_wide_beside_band_block():
    """A plan holding a packed band block and a dense triangle launches each
    table with its own kernel (the band block on the 512-column strips, its
    partials behind the wide ones): both within 1e-12 of numpy, the triangle's
    sums bitwise those of the block alone."""
    nb, bw, ncol = 3000, 300, 8
    i = np.arange(nb)
    band = np.where(np.abs(i[:, None] - i[None, :]) <= bw, block(nb), 0.0)
    V = np.concatenate([vec(nb, ncol), vec(1281, ncol)], axis=1)
    with environ(FORCED):
        eng = Engine([nb, 1281], K=1)
        eng.set_ld_block_csr(0, 0, UpperCsr(band, bw))
        eng.set_ld_block(0, 1, block(1281))
        assert eng.ld_block_format(0, 0) == 2 and eng.ld_block_format(0, 1) == 1
        eng.set_ridge(RIDGE)
        form = eng.ld_pass_form(0, ncol)   # the band's strips are ragged: 4-wave, finalize 1
        assert (form.kind, form.rest_kind, form.fin_form) == ("wide", "strip4", 1), form
        Y = np.array(eng.ld_matvec(0, V))
        eng.close()
    L = vo.BlockLD([band, block(1281)], s=RIDGE)
    for j in range(ncol):
        assert maxrel(Y[j], L.matvec_Rs(V[j])) < 1e-12, j
    alone = products([1281], [ncol], FORCED)
    np.testing.assert_array_equal(Y[:, nb:], alone[ncol][0])


def test_wide_repeatable():
    """Two forced-wide passes on the same inputs are bitwise equal (no
    dependence on dispatch order or on which wave combines first)."""
    for ncol in NCOLS:
        a, b = forced_wide()[ncol]
        np.testing.assert_array_equal(a, b)
