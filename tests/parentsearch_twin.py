"""numpy twin of ``snpm_panel_parent_counts`` / ``k_par_count`` (test infrastructure, written from the definition and not from the
library code): every pair of accession columns scored, window by window, as the parents of a recombinant sample.  Per window the
indicator products run in fp64 through BLAS (sums of 0/1 products far below 2^53: exact) and are converted to int64.

Per cell (a, b) -- positions in the column list -- and window, over the rows ``ni`` where the F1 of a and b is informative (both
called, not 2 with 2, not other with other) AND the sample has a class: n = |ni|, hA / hB = rows of ni where a's / b's code is the
sample's class, hF = rows of ni where the F1's class (ref where both are 0, alt where both are 1, het where they differ) is it.
A window with n < min_win_sites adds nothing.  Else with hom = max(hA, hB): hF > hom gives score += hF, w_het += 1; otherwise
score += hom and w_first[a, b] += 1 when hA > hB or (hA == hB and a <= b) -- cell (b, a) evaluates the same rule for itself;
n_tot += n."""
import numpy as np

NO_CLASS = 0xFF


def _select(snps, sample_class, cols, rows):
    v = np.asarray(snps)
    if rows is not None:
        v = v[rows, :]
    if cols is not None:
        v = v[:, np.asarray(cols, dtype=np.int64)]
    s = np.asarray(sample_class).reshape(-1)
    assert len(s) == len(v), "one sample class per selected row"
    return v, s


def _window_matrices(v, s):
    """(n, hA, hF) int64 [k, k] of one window's rows; hB is hA transposed"""
    info = v >= 0
    f0, f1, f2 = ((v == c).astype(np.float64) for c in (0, 1, 2))
    f3 = (info & (v != 0) & (v != 1) & (v != 2)).astype(np.float64)
    fi = info.astype(np.float64)
    s0, s1, s2 = ((s == c).astype(np.float64)[:, None] for c in (0, 1, 2))
    cls = s0 + s1 + s2                                          # the row has a class
    ma = f0 * s0 + f1 * s1 + f2 * s2                            # the column's code is the sample's class
    # informative(a, b, row) = fi_a fi_b - f2_a f2_b - f3_a f3_b
    n = (fi * cls).T @ fi - (f2 * cls).T @ f2 - (f3 * cls).T @ f3
    ha = (fi * ma).T @ fi - (f2 * ma).T @ f2 - (f3 * ma).T @ f3
    het = (fi * s2).T @ fi - sum((p * s2).T @ p for p in (f0, f1, f2, f3))
    hf = (f0 * s0).T @ f0 + (f1 * s1).T @ f1 + het
    return tuple(np.rint(m).astype(np.int64) for m in (n, ha, hf))


def parent_counts(snps, sample_class, win_off, min_win_sites=1, cols=None, rows=None):
    """snps int8 [n_snp, n_acc] (negative = missing, 0 / 1 / 2, anything else one further class); sample_class uint8, one class per
    selected row (0 / 1 / 2, anything else: none); win_off [n_win + 1] offsets into the selected rows; cols / rows as numpy fancy
    indices (repeats count as listed) or None for all.  Returns (score, n_tot, w_first, w_het), int32 [n_cols, n_cols]."""
    v, s = _select(snps, sample_class, cols, rows)
    win_off = np.asarray(win_off, dtype=np.int64)
    assert win_off[0] == 0 and win_off[-1] == len(v) and (np.diff(win_off) >= 0).all() and int(min_win_sites) >= 1
    k = v.shape[1]
    score, n_tot, w_first, w_het = (np.zeros((k, k), dtype=np.int64) for _ in range(4))
    a_le_b = np.arange(k)[:, None] <= np.arange(k)[None, :]
    for lo, hi in zip(win_off[:-1].tolist(), win_off[1:].tolist()):
        if hi == lo:
            continue
        n, ha, hf = _window_matrices(v[lo:hi], s[lo:hi])
        hb = ha.T
        used = n >= int(min_win_sites)
        hom = np.maximum(ha, hb)
        as_f1 = hf > hom
        score += np.where(used, np.where(as_f1, hf, hom), 0)
        n_tot += np.where(used, n, 0)
        w_het += used & as_f1
        w_first += used & ~as_f1 & ((ha > hb) | ((ha == hb) & a_le_b))
    return tuple(m.astype(np.int32) for m in (score, n_tot, w_first, w_het))


def pair_windows(snps, sample_class, win_off, a, b, cols=None, rows=None):
    """the raw (n, hA, hB, hF) of every window for the cell (a, b), int64 [n_win, 4], row by row from the rules"""
    v, s = _select(snps, sample_class, cols, rows)
    x, y = v[:, a].astype(np.int64), v[:, b].astype(np.int64)
    x, y = (np.where(c < 0, -1, np.where(c > 2, 3, c)) for c in (x, y))
    s = s.astype(np.int64)
    f1 = np.where((x == 0) & (y == 0), 0, np.where((x == 1) & (y == 1), 1, np.where((x >= 0) & (y >= 0) & (x != y), 2, -1)))
    ni = (f1 >= 0) & (s <= 2)
    out = np.zeros((len(win_off) - 1, 4), dtype=np.int64)
    for w, (lo, hi) in enumerate(zip(win_off[:-1], win_off[1:])):
        m = ni[lo:hi]
        out[w] = (m.sum(), (m & (x[lo:hi] == s[lo:hi])).sum(), (m & (y[lo:hi] == s[lo:hi])).sum(), (m & (f1[lo:hi] == s[lo:hi])).sum())
    return out


def parent_counts_direct(snps, sample_class, win_off, min_win_sites=1):
    """the same four matrices cell by cell through ``pair_windows`` (small inputs)"""
    k = np.asarray(snps).shape[1]
    score, n_tot, w_first, w_het = (np.zeros((k, k), dtype=np.int32) for _ in range(4))
    for a in range(k):
        for b in range(k):
            for n, ha, hb, hf in pair_windows(snps, sample_class, win_off, a, b).tolist():
                if n < min_win_sites:
                    continue
                n_tot[a, b] += n
                if hf > max(ha, hb):
                    score[a, b] += hf
                    w_het[a, b] += 1
                else:
                    score[a, b] += max(ha, hb)
                    if ha > hb or (ha == hb and a <= b):
                        w_first[a, b] += 1
    return score, n_tot, w_first, w_het


# ------------------------------------------------------------------------------------------------ the planted case
PLANTED_PARENTS = (3, 17)
PLANTED_MOSAIC = "AA AB AB BB AB AA AB BB BB AB AB AA".split()
PLANTED_BIN = 2500                     # bp per window: 250 DB rows, ten bp apart


def planted_case():
    """A DB of 40 accessions x 3000 rows on two chromosomes of six windows of 250 rows each, and a hard-called sample that is the
    exact mosaic PLANTED_MOSAIC of accessions 3 and 17: parent A in an AA window, parent B in a BB window, their F1 in an AB window.
    Twelve decoys (accessions 20 .. 31) copy the sample's calls -- about half of its het rows kept as DB hets, the others drawn
    homozygous at random.  Every row is matched.  Returns a dict: snps, names, positions, chrs, chr_regions (the DB), genome (the
    content of a genome JSON), s_chr, s_pos, s_gt (the sample), classes, win_off."""
    rng = np.random.default_rng(11)
    n, na, per = 3000, 40, 250
    a, b = PLANTED_PARENTS
    db = rng.choice(np.array([0, 1], dtype=np.int8), size=(n, na))
    miss = rng.random((n, na)) < 0.05
    miss[:, [a, b]] = False
    db[miss] = -1
    f1 = np.where(db[:, a] == db[:, b], db[:, a], 2).astype(np.int8)
    state = np.repeat(np.array(PLANTED_MOSAIC), per)
    sample = np.where(state == "AA", db[:, a], np.where(state == "BB", db[:, b], f1)).astype(np.int8)
    for d in range(20, 32):
        col = sample.copy()
        het = np.flatnonzero(sample == 2)
        redraw = het[rng.random(len(het)) >= 0.5]
        col[redraw] = rng.integers(0, 2, len(redraw))
        db[:, d] = col
    half = n // 2
    positions = np.concatenate([np.arange(10, 10 + 10 * half, 10), np.arange(10, 10 + 10 * half, 10)]).astype(np.int64)
    regions = np.array([[0, half], [half, n]], dtype=np.int64)
    genome = {"ref_chrs": ["Chr1", "Chr2"], "ref_chrlen": [10 * half + 1, 10 * half + 1]}
    s_chr = np.array(["Chr%d" % c for c in np.repeat([1, 2], half)])
    return dict(snps=db, names=np.array(["acc%02d" % i for i in range(na)]), positions=positions, chrs=np.array(["Chr1", "Chr2"]),
                chr_regions=regions, genome=genome, s_chr=s_chr, s_pos=positions.copy(), s_gt=np.array(["0/0", "1/1", "0/1"])[sample],
                classes=sample.astype(np.uint8), win_off=np.arange(0, n + 1, per, dtype=np.int64))
