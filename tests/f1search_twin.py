"""numpy twin of ``snpm_panel_f1_counts`` / ``k_f1x_count`` (test infrastructure): hits and ninfo of the in-silico F1 of every pair of
accession columns against one sample's hard calls.  The indicator products run in fp64 through BLAS (sums of 0/1 products far below
2^53: exact) and are converted to int32."""
import numpy as np

NO_CLASS = 0xFF


def f1_counts(snps, sample_class, cols=None, rows=None):
    """snps int8 [n_snp, n_acc] (negative = missing, 0 / 1 / 2, anything else one further class); sample_class uint8, one class per
    selected row (0 ref, 1 alt, 2 het, anything else: none); cols / rows as numpy fancy indices (repeats count as listed), a slice
    for rows, or None for all.  Returns (hits, ninfo) int32 [n_cols, n_cols].

    The F1 of columns a, b at a row: ref where both are 0, alt where both are 1, het where both are called and differ, else
    uninformative (a call missing, 2 with 2, other with other)."""
    v = np.asarray(snps)
    if rows is not None:
        v = v[rows, :]
    if cols is not None:
        v = v[:, np.asarray(cols, dtype=np.int64)]
    s = np.asarray(sample_class).reshape(-1)
    assert len(s) == len(v), "one sample class per selected row"
    info = v >= 0
    planes = [v == 0, v == 1, v == 2, info & (v != 0) & (v != 1) & (v != 2)]
    f = [p.astype(np.float64) for p in planes]
    fi = info.astype(np.float64)
    s0, s1, s2 = ((s == c).astype(np.float64)[:, None] for c in (0, 1, 2))
    ninfo = fi.T @ fi - f[2].T @ f[2] - f[3].T @ f[3]
    het_hits = (fi * s2).T @ fi - sum((p * s2).T @ p for p in f)
    hits = (f[0] * s0).T @ f[0] + (f[1] * s1).T @ f[1] + het_hits
    return np.rint(hits).astype(np.int32), np.rint(ninfo).astype(np.int32)


def f1_counts_direct(snps, sample_class):
    """the same counts pair by pair, straight from the rules (small inputs)"""
    v = np.asarray(snps).astype(np.int64)
    s = np.asarray(sample_class).astype(np.int64)
    k = v.shape[1]
    hits, ninfo = np.zeros((k, k), dtype=np.int32), np.zeros((k, k), dtype=np.int32)
    c = np.where(v < 0, -1, np.where(v > 2, 3, v))
    for a in range(k):
        for b in range(k):
            x, y = c[:, a], c[:, b]
            f1 = np.where((x == 0) & (y == 0), 0, np.where((x == 1) & (y == 1), 1, np.where((x >= 0) & (y >= 0) & (x != y), 2, -1)))
            ninfo[a, b] = np.count_nonzero(f1 >= 0)
            hits[a, b] = np.count_nonzero((f1 >= 0) & (f1 == s))
    return hits, ninfo


# ------------------------------------------------------------------------------------------------ the planted case
PLANTED_PARENTS = (3, 17)


def planted_case():
    """A DB of 40 accessions x 4000 rows on two chromosomes and a hard-called sample that is the exact F1 of accessions 3 and 17 at
    the 3000 first rows where both are called (plus 50 positions the DB does not have).  Twelve decoys (accessions 20 .. 31) copy
    the F1's calls there -- half of its het rows kept as DB hets, the others drawn homozygous at random -- so that each matches the
    sample better ON ITS OWN than either parent does.  Returns a dict: snps, names, positions, chrs, chr_regions (the DB), s_chr,
    s_pos, s_gt (the sample, in file order), db_rows, classes (the matched rows and the sample's classes there)."""
    rng = np.random.default_rng(4017)
    n, na = 4000, 40
    a, b = PLANTED_PARENTS
    db = rng.choice(np.array([0, 1], dtype=np.int8), size=(n, na))
    db[rng.random((n, na)) < 0.05] = -1
    both = (db[:, a] >= 0) & (db[:, b] >= 0)
    rows = np.flatnonzero(both)[:3000]
    f1 = np.where(db[:, a] == db[:, b], db[:, a], 2).astype(np.int8)
    for d in range(20, 32):
        col = f1.copy()
        het = np.flatnonzero(f1 == 2)
        redraw = het[rng.random(len(het)) >= 0.5]
        col[redraw] = rng.integers(0, 2, len(redraw))
        col[~both] = -1
        db[:, d] = col
    positions = np.concatenate([np.arange(10, 10 + 10 * 2500, 10), np.arange(7, 7 + 10 * 1500, 10)]).astype(np.int64)
    regions = np.array([[0, 2500], [2500, 4000]], dtype=np.int64)
    chrom = np.where(rows < 2500, 1, 2)
    text = np.array(["0/0", "1/1", "0/1"])[f1[rows]]
    # 25 positions per chromosome that the DB does not have (odd offsets), merged in position order
    extra_chr = np.repeat([1, 2], 25)
    extra_pos = np.concatenate([np.arange(15, 15 + 500 * 25, 500) + 1, np.arange(12, 12 + 300 * 25, 300) + 1]).astype(np.int64)
    s_chr = np.concatenate([chrom, extra_chr])
    s_pos = np.concatenate([positions[rows], extra_pos])
    s_gt = np.concatenate([text, np.repeat("1/1", 50)])
    order = np.lexsort((s_pos, s_chr))
    assert not np.isin(extra_pos[:25], positions[:2500]).any() and not np.isin(extra_pos[25:], positions[2500:]).any()
    return dict(snps=db, names=np.array(["acc%02d" % i for i in range(na)]), positions=positions, chrs=np.array(["Chr1", "Chr2"]),
                chr_regions=regions, s_chr=np.array(["Chr%d" % c for c in s_chr[order]]), s_pos=s_pos[order], s_gt=s_gt[order],
                db_rows=rows, classes=f1[rows].astype(np.uint8))
