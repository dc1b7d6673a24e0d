"""numpy twin of ``snpm_panel_kinship_counts`` / ``k_kin_count`` (test infrastructure): the three relatedness counts of every pair
of accession columns over panel rows, and the reference's kinship from them.  The indicator products run in fp64 through BLAS
(sums of 0/1 products far below 2^53: exact) and are converted to int32."""
import numpy as np


def kinship_counts(snps, cols=None, rows=None):
    """snps int8 [n_snp, n_acc] (negative = missing, 0 / 1 homozygous, anything else informative only); cols / rows as numpy fancy
    indices (repeats count as listed), a slice for rows, or None for all.  Returns (ninfo, same, diff) int32 [n_cols, n_cols]."""
    v = np.asarray(snps)
    if rows is not None:
        v = v[rows, :]
    if cols is not None:
        v = v[:, np.asarray(cols, dtype=np.int64)]
    info, p0, p1 = ((m).astype(np.float64) for m in (v >= 0, v == 0, v == 1))
    ninfo = info.T @ info
    same = p0.T @ p0 + p1.T @ p1
    p01 = p0.T @ p1
    diff = p01 + p01.T
    return tuple(np.rint(m).astype(np.int32) for m in (ninfo, same, diff))


def kinship(ninfo, same, diff):
    """(same - diff) / ninfo in fp64: one correctly rounded division of the reference's two exact sums; 0 / 0 = nan"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.divide((same.astype(np.int64) - diff).astype(np.float64), ninfo.astype(np.float64))
