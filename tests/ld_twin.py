"""numpy twin of ``snpm_panel_ld_band`` / ``k_ld_planes`` + ``k_ld_band``, of ``snpm_ld_prune`` and of ``Genotype.calculate_ld`` (test
infrastructure): the nine pair counts of every selected row with each of the ``band`` rows after it, r2 from them, the greedy prune
and the dense matrix."""
import numpy as np

NAMES = ("n", "Ak", "Hk", "Aj", "Hj", "AA", "AH", "HA", "HH")


def select(snps, cols=None, rows=None):
    v = np.asarray(snps)
    if rows is not None:
        v = v[np.arange(rows.start, rows.stop) if isinstance(rows, range) else np.asarray(rows, dtype=np.int64), :]
    if cols is not None:
        cols = np.asarray(cols, dtype=np.int64).reshape(-1)
        assert len(np.unique(cols)) == len(cols), "a repeated column is refused"
        v = v[:, cols]
    return v


def band_counts(snps, band, cols=None, rows=None):
    """snps int8 [n_snp, n_acc] (1 = alt, 2 = het, 0 = ref; anything else -- negative, 3 -- is outside m).  int32 [n_rows, band, 9]
    in the order of NAMES; cells with k + d >= n_rows are zero."""
    v = select(snps, cols, rows)
    a, h, m = v == 1, v == 2, (v >= 0) & (v <= 2)
    n = v.shape[0]
    out = np.zeros((n, band, 9), dtype=np.int32)
    for d in range(1, min(band, n - 1) + 1):
        k, j = slice(0, n - d), slice(d, n)
        pairs = ((m[k], m[j]), (a[k], m[j]), (h[k], m[j]), (a[j], m[k]), (h[j], m[k]), (a[k], a[j]), (a[k], h[j]), (h[k], a[j]), (h[k], h[j]))
        for q, (x, y) in enumerate(pairs):
            out[:n - d, d - 1, q] = (x & y).sum(axis=1)
    return out


def r2_from_counts(counts, v_alt=2, v_het=1, min_n=2):
    """the formula of the issue in int64 and three fp64 operations; nan where n < min_n or a row is constant"""
    c = np.asarray(counts).astype(np.int64)
    n, ak, hk, aj, hj, aa, ah, ha, hh = (c[..., q] for q in range(9))
    sx, sxx = v_alt * ak + v_het * hk, v_alt * v_alt * ak + v_het * v_het * hk
    sy, syy = v_alt * aj + v_het * hj, v_alt * v_alt * aj + v_het * v_het * hj
    sxy = v_alt * v_alt * aa + v_alt * v_het * (ah + ha) + v_het * v_het * hh
    num, dx, dy = n * sxy - sx * sy, n * sxx - sx * sx, n * syy - sy * sy
    ok = (n >= min_n) & (dx != 0) & (dy != 0)
    out = np.full(n.shape, np.nan, dtype=np.float64)
    numf, dxf, dyf = num[ok].astype(np.float64), dx[ok].astype(np.float64), dy[ok].astype(np.float64)
    out[ok] = (numf * numf) / (dxf * dyf)
    return out


def ld_band(snps, band, cols=None, rows=None, v_alt=2, v_het=1, min_n=2):
    counts = band_counts(snps, band, cols, rows)
    return counts, r2_from_counts(counts, v_alt, v_het, min_n)


def prune(r2, eligible=None, threshold=0.2):
    """greedy in row order: keep[k] = eligible[k] and no kept j in [k - band, k) with r2[j][k - j - 1] > threshold"""
    n, band = r2.shape
    keep = np.zeros(n, dtype=np.uint8)
    for k in range(n):
        ok = True if eligible is None else bool(eligible[k])
        for j in range(max(0, k - band), k):
            if ok and keep[j] and r2[j, k - j - 1] > threshold:
                ok = False
        keep[k] = ok
    return keep


def dense(snps, snp_ix, accs_ix=None, v_alt=2, v_het=1, min_n=2):
    """the full symmetric r2 matrix of the listed rows among the listed columns, pair by pair, the diagonal from the row itself"""
    v = select(snps, accs_ix, np.asarray(snp_ix, dtype=np.int64))
    n = v.shape[0]
    out = np.full((n, n), np.nan)
    for x in range(n):
        for y in range(x, n):
            pair = band_counts(v[[x, y]], 1)[0, 0]
            out[x, y] = out[y, x] = r2_from_counts(pair, v_alt, v_het, min_n)
    return out


def brute_counts(snps, band, cols=None, rows=None):
    """band_counts by a loop over every column of every pair"""
    v = select(snps, cols, rows)
    n = v.shape[0]
    out = np.zeros((n, band, 9), dtype=np.int32)
    for k in range(n):
        for d in range(1, band + 1):
            if k + d >= n:
                continue
            for x, y in zip(v[k].tolist(), v[k + d].tolist()):
                mx, my = 0 <= x <= 2, 0 <= y <= 2
                out[k, d - 1] += [mx and my, x == 1 and my, x == 2 and my, y == 1 and mx, y == 2 and mx,
                                  x == 1 and y == 1, x == 1 and y == 2, x == 2 and y == 1, x == 2 and y == 2]
    return out
