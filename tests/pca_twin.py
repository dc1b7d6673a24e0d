"""numpy twin of ``snpm_panel_gram`` / ``snpm_panel_loadings`` and of ``engine.gram`` / ``engine.loadings`` (test infrastructure): the
class-table values of a panel, the Gram matrix and the loadings in numpy's order of summation, the same two exactly rounded
(``math.fsum`` per cell: the reference of the tolerance tests) and the sums of absolute products their error bounds are made of; and
the planted panel of the command tests (three Balding-Nichols populations)."""
import math

import numpy as np


def values(snps, tab, cols=None, rows=None):
    """fp64 [n_rows, n_cols]: t(s, i) = tab[s][code] of the selected rows and columns of snps int8 [n_snp, n_acc] -- negative =
    missing (value 0), 0 / 1 / 2 the first three entries, anything else the fourth; cols / rows: fancy indices (repeats count as
    listed), a slice / range, or None"""
    v = np.asarray(snps)
    if rows is not None:
        v = v[np.arange(rows.start, rows.stop) if isinstance(rows, range) else np.asarray(rows, dtype=np.int64), :]
    if cols is not None:
        v = v[:, np.asarray(cols, dtype=np.int64).reshape(-1)]
    tab = np.asarray(tab, dtype=np.float64)
    assert tab.shape == (v.shape[0], 4)
    code = np.where(v > 2, 3, np.maximum(v, 0)).astype(np.int64)
    return np.where(v < 0, 0.0, tab[np.arange(v.shape[0])[:, None], code])


def gram(snps, tab, cols=None, rows=None):
    t = values(snps, tab, cols, rows)
    return t.T @ t


def loadings(snps, tab, vec, cols=None, rows=None):
    return values(snps, tab, cols, rows) @ np.asarray(vec, dtype=np.float64)


def gram_abs(snps, tab, cols=None, rows=None):
    """S[i][j] = sum_s |t(s, i)| |t(s, j)|"""
    t = np.abs(values(snps, tab, cols, rows))
    return t.T @ t


def loadings_abs(snps, tab, vec, cols=None, rows=None):
    """sum_i |t(s, i)| |vec[i][c]|"""
    return np.abs(values(snps, tab, cols, rows)) @ np.abs(np.asarray(vec, dtype=np.float64))


def _fsum_columns(m):
    """the exactly rounded sum of every column of m (every product of two doubles below is itself rounded once: see gram_exact)"""
    return np.array([math.fsum(col) for col in np.ascontiguousarray(m.T).tolist()])


def _two_product(a, b):
    """a * b = hi + lo exactly (Dekker's product with Veltkamp's split; no overflow at the magnitudes of a class table)"""
    hi = a * b
    split = 134217729.0
    ca, cb = split * a, split * b
    a1, b1 = ca - (ca - a), cb - (cb - b)
    a2, b2 = a - a1, b - b1
    return hi, a2 * b2 - (((hi - a1 * b1) - a2 * b1) - a1 * b2)


def gram_exact(snps, tab, cols=None, rows=None, cell_rows=None):
    """the exactly rounded Gram matrix: every product as an exact pair hi + lo, ``math.fsum`` over the 2 R terms of a cell.
    ``cell_rows``: only these rows i of the matrix (all columns), as [len(cell_rows), n_cols]"""
    t = values(snps, tab, cols, rows)
    which = range(t.shape[1]) if cell_rows is None else cell_rows
    out = np.empty((len(which), t.shape[1]))
    for k, i in enumerate(which):
        hi, lo = _two_product(t[:, [i]], t)
        out[k] = _fsum_columns(np.concatenate([hi, lo], axis=0))
    return out


def loadings_exact(snps, tab, vec, cols=None, rows=None):
    """the exactly rounded loadings, as gram_exact"""
    t, vec = values(snps, tab, cols, rows), np.asarray(vec, dtype=np.float64)
    out = np.empty((t.shape[0], vec.shape[1]))
    for c in range(vec.shape[1]):
        hi, lo = _two_product(t, vec[None, :, c])
        out[:, c] = _fsum_columns(np.concatenate([hi, lo], axis=1).T)
    return out


def integer_table(rng, n_rows):
    """a class table of small integers, -3 .. 3 per entry: every partial sum of a Gram matrix or of loadings with an integer vec is
    an exact integer"""
    return rng.integers(-3, 4, size=(n_rows, 4)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ the planted panel of the command tests
PLANTED_POPS, PLANTED_PER_POP, PLANTED_ROWS, PLANTED_FST = 3, 13, 600, 0.15


def planted_case(seed):
    """3 populations x 13 inbred accessions x 600 rows on two chromosomes.  Balding-Nichols: the ancestral frequency of a row uniform
    in 0.1 .. 0.9, a population's frequency Beta(p (1 - F) / F, (1 - p) (1 - F) / F) with F = 0.15, every accession homozygous for
    an allele drawn at that frequency; then 2 % of the calls het, then 3 % missing.  The LAST accession of every population is the
    held-out one: ``panel`` lists the other 36 (population by population)."""
    rng = np.random.default_rng(1000 + seed)
    n_acc = PLANTED_POPS * PLANTED_PER_POP
    anc = rng.uniform(0.1, 0.9, size=PLANTED_ROWS)
    f = (1.0 - PLANTED_FST) / PLANTED_FST
    snps = np.empty((PLANTED_ROWS, n_acc), dtype=np.int8)
    for q in range(PLANTED_POPS):
        freq = rng.beta(anc * f, (1.0 - anc) * f)
        snps[:, q * PLANTED_PER_POP:(q + 1) * PLANTED_PER_POP] = rng.random((PLANTED_ROWS, PLANTED_PER_POP)) < freq[:, None]
    snps[rng.random(snps.shape) < 0.02] = 2
    snps[rng.random(snps.shape) < 0.03] = -1
    names = np.array(["p%da%02d" % (a // PLANTED_PER_POP, a % PLANTED_PER_POP) for a in range(n_acc)])
    pop = np.array(["pop%d" % (a // PLANTED_PER_POP) for a in range(n_acc)])
    held = np.array([(q + 1) * PLANTED_PER_POP - 1 for q in range(PLANTED_POPS)])
    panel = np.array([a for a in range(n_acc) if a not in held.tolist()])
    chrs = np.array(["Chr1", "Chr2"])
    chr_regions = np.array([[0, 350], [350, 600]])
    positions = np.concatenate([101 + 1000 * np.arange(350), 101 + 1000 * np.arange(250)]).astype(np.int64)
    return {"snps": snps, "names": names, "pop": pop, "held": held, "panel": panel, "positions": positions, "chrs": chrs, "chr_regions": chr_regions}
