"""numpy twin of ``snpm_panel_site_counts`` / ``k_site_counts`` and of ``engine.site_counts`` (test infrastructure): the four allele
counts of every selected panel row per group of accession columns, and the reference's frequencies from them.  Groups are numpy
fancy indices: a column listed twice counts twice."""
import numpy as np


def site_counts(snps, groups=None, rows=None):
    """snps int8 [n_snp, n_acc] (negative = missing, 0 / 1 / 2 the counted codes, anything else informative only); groups: None
    (one group of all columns), one index array or a list of index arrays; rows: a fancy index, a slice / range, or None.
    Returns int32 [G, n_rows, 4]: c0, c1, c2, ninfo."""
    v = np.asarray(snps)
    if rows is not None:
        v = v[np.arange(rows.start, rows.stop) if isinstance(rows, range) else rows, :]
    if groups is None:
        groups = [np.arange(v.shape[1])]
    elif isinstance(groups, np.ndarray) or (len(groups) and np.isscalar(groups[0])):
        groups = [groups]
    out = np.zeros((len(groups), v.shape[0], 4), dtype=np.int32)
    for g, cols in enumerate(groups):
        sub = v[:, np.asarray(cols, dtype=np.int64).reshape(-1)]
        for code in (0, 1, 2):
            out[g, :, code] = (sub == code).sum(axis=1)
        out[g, :, 3] = (sub >= 0).sum(axis=1)
    return out


def frequency(counts, min_informative=0, polarize_geno=1, return_maf=True):
    """(2 c[polarize_geno] + c2) / (2 ninfo) in fp64, one correctly rounded division; nan where ninfo <= min_informative"""
    c = counts.astype(np.int64)
    ninfo, num_alt = c[..., 3], 2 * c[..., polarize_geno] + c[..., 2]
    af = np.full(ninfo.shape, np.nan)
    ok = ninfo > min_informative
    af[ok] = num_alt[ok].astype(np.float64) / (2 * ninfo[ok]).astype(np.float64)
    return np.minimum(af, 1 - af) if return_maf else af
