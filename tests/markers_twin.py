"""The numpy twin of ``snpm_panel_marker_select``: the greedy choice of a small set of SNPs that separates
every pair of accessions ``depth`` times.  The round loop is a plain Python loop, each round is vectorised; all of it is integer
arithmetic, so the device must give the same arrays bit for bit.

Row r (a position in the row selection) *separates* the unordered pair {a, b} (positions in the column list, a != b) when both calls
are homozygous and different: code 0 in one column, 1 in the other.  ``need`` starts at ``depth`` off the diagonal; a round computes
for every eligible row the number of pairs with need > 0 it separates, picks the largest (ties: the smallest position), decrements
the need of those pairs, and makes the pick -- and, with ``coord``, every row closer than ``min_dist`` to it -- ineligible.

Stop reasons: 0 every pair resolved (checked first), 1 ``max_markers`` picks made, 2 no eligible row separates an unresolved pair.
"""
import numpy as np

STOP_RESOLVED, STOP_MAX_MARKERS, STOP_NO_GAIN = 0, 1, 2
NO_LIMIT = 2 ** 62            # max_markers=None: what ``engine.marker_select`` hands to the library


def planes(snps, cols=None, rows=None):
    """(H0, H1) booleans [n_rows, ncols] of the selection: the call is code 0 / code 1"""
    snps = np.asarray(snps)
    if rows is not None:
        snps = snps[np.asarray(rows if not isinstance(rows, range) else np.arange(rows.start, rows.stop), dtype=np.int64)]
    if cols is not None:
        snps = snps[:, np.asarray(cols, dtype=np.int64)]
    return snps == 0, snps == 1


def gains(h0, h1, unresolved):
    """int64 [n_rows]: the unordered pairs of ``unresolved`` (boolean, symmetric) each row separates -- a in H0 and b in H1 names
    every such pair once.  (The product runs in fp64, where sums of at most 2^53 ones are exact: BLAS instead of an integer loop.)"""
    return np.rint((h0.astype(np.float64) @ unresolved.astype(np.float64)) * h1).astype(np.int64).sum(axis=1)


def separated(h0_row, h1_row):
    """boolean [ncols, ncols], symmetric: the pairs one row separates"""
    s = h0_row[:, None] & h1_row[None, :]
    return s | s.T


def too_close(coord, at, min_dist):
    """rows with |coord[r] - coord[at]| < min_dist, exact for any two int64 values (the difference is taken in uint64)"""
    c = np.asarray(coord, dtype=np.int64)
    u, u0 = c.view(np.uint64), c.view(np.uint64)[at]
    dist = np.where(c > c[at], u - u0, u0 - u)
    return dist < np.uint64(min_dist)


def marker_select(snps, depth=1, max_markers=None, coord=None, min_dist=0, eligible=None, cols=None, rows=None, first_gain=True):
    """the dict of ``engine.marker_select``: chosen int64 [n_chosen], gain_at int32 [n_chosen], n_chosen, remaining, stop_reason,
    need uint8 [ncols, ncols], first_gain int32 [n_rows] (None when not asked for)"""
    h0, h1 = planes(snps, cols, rows)
    n_rows, ncols = h0.shape
    assert 1 <= depth <= 255 and min_dist >= 0 and (coord is not None or min_dist == 0)
    max_markers = NO_LIMIT if max_markers is None else int(max_markers)
    need = np.full((ncols, ncols), depth, dtype=np.uint8)
    np.fill_diagonal(need, 0)
    remaining = int(depth) * (ncols * (ncols - 1) // 2)
    elig = np.ones(n_rows, dtype=bool) if eligible is None else np.asarray(eligible).reshape(-1) != 0
    assert len(elig) == n_rows and (coord is None or len(coord) == n_rows)
    chosen, gain_at = [], []
    first = np.zeros(n_rows, dtype=np.int32)
    if first_gain and ncols >= 2 and n_rows > 0 and max_markers > 0:        # a call that launches nothing reports zeros
        first = gains(h0, h1, need > 0).astype(np.int32)
    while True:
        if remaining == 0:
            reason = STOP_RESOLVED
            break
        if len(chosen) == max_markers:
            reason = STOP_MAX_MARKERS
            break
        gain = np.where(elig, gains(h0, h1, need > 0), 0)
        best = int(np.argmax(gain)) if n_rows else 0                       # (argmax: the first of equal values)
        if n_rows == 0 or gain[best] == 0:
            reason = STOP_NO_GAIN
            break
        chosen.append(best)
        gain_at.append(int(gain[best]))
        need[separated(h0[best], h1[best]) & (need > 0)] -= 1
        remaining -= int(gain[best])
        elig[best] = False
        if coord is not None:
            elig &= ~too_close(coord, best, min_dist)
    return {"chosen": np.array(chosen, dtype=np.int64), "gain_at": np.array(gain_at, dtype=np.int32), "n_chosen": len(chosen),
            "remaining": remaining, "stop_reason": reason, "need": need, "first_gain": first if first_gain else None}


def brute_force(snps, depth=1, max_markers=None, coord=None, min_dist=0, eligible=None, cols=None, rows=None):
    """the definition as loops over rows and pairs, on Python integers: nothing shared with the vectorised rounds"""
    snps = np.asarray(snps)
    row_list = list(range(snps.shape[0])) if rows is None else [int(r) for r in rows]
    col_list = list(range(snps.shape[1])) if cols is None else [int(c) for c in cols]
    v = [[int(snps[r, c]) for c in col_list] for r in row_list]
    n_rows, ncols = len(row_list), len(col_list)
    max_markers = NO_LIMIT if max_markers is None else max_markers
    need = [[0 if a == b else depth for b in range(ncols)] for a in range(ncols)]
    remaining = depth * (ncols * (ncols - 1) // 2)
    elig = [True if eligible is None else eligible[r] != 0 for r in range(n_rows)]
    sep = lambda r, a, b: (v[r][a] == 0 and v[r][b] == 1) or (v[r][a] == 1 and v[r][b] == 0)      # noqa: E731
    launches = ncols >= 2 and n_rows > 0 and max_markers > 0
    first = [sum(sep(r, a, b) for a in range(ncols) for b in range(a + 1, ncols)) if launches else 0 for r in range(n_rows)]
    chosen, gain_at = [], []
    while True:
        if remaining == 0:
            reason = STOP_RESOLVED
            break
        if len(chosen) == max_markers:
            reason = STOP_MAX_MARKERS
            break
        best, best_gain = -1, 0
        for r in range(n_rows):
            if not elig[r]:
                continue
            g = sum(1 for a in range(ncols) for b in range(a + 1, ncols) if need[a][b] > 0 and sep(r, a, b))
            if g > best_gain:
                best, best_gain = r, g
        if best < 0:
            reason = STOP_NO_GAIN
            break
        chosen.append(best)
        gain_at.append(best_gain)
        for a in range(ncols):
            for b in range(ncols):
                if a != b and need[a][b] > 0 and sep(best, a, b):
                    need[a][b] -= 1
        remaining -= best_gain
        elig[best] = False
        if coord is not None:
            for r in range(n_rows):
                if abs(int(coord[r]) - int(coord[best])) < min_dist:
                    elig[r] = False
    return {"chosen": np.array(chosen, dtype=np.int64), "gain_at": np.array(gain_at, dtype=np.int32), "n_chosen": len(chosen),
            "remaining": remaining, "stop_reason": reason, "need": np.array(need, dtype=np.uint8).reshape(ncols, ncols),
            "first_gain": np.array(first, dtype=np.int32)}


def replay(snps, chosen, depth=1, cols=None, rows=None):
    """the need matrix after the rows of ``chosen`` (positions in the selection), one after the other"""
    h0, h1 = planes(snps, cols, rows)
    need = np.full((h0.shape[1],) * 2, depth, dtype=np.uint8)
    np.fill_diagonal(need, 0)
    for r in chosen:
        need[separated(h0[r], h1[r]) & (need > 0)] -= 1
    return need


KEYS = ("chosen", "gain_at", "n_chosen", "remaining", "stop_reason", "need", "first_gain")


def same(got, want, keys=KEYS):
    """every entry equal, arrays with their dtype and shape"""
    for k in keys:
        g, w = got[k], want[k]
        if isinstance(w, np.ndarray):
            if not (isinstance(g, np.ndarray) and g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)):
                return False
        elif g != w:
            return False
    return True


# ------------------------------------------------------------------------------------------------ the planted panel of the command tests
PLANTED_SEED = 41
PLANTED_TWINS = (7, 29)             # two identical accessions: no row separates them
PLANTED_HIDDEN = (12, 33)           # differ only at the rows of PLANTED_HIDDEN_ROWS, which the site list of the tests leaves out
PLANTED_HIDDEN_ROWS = (50, 350, 351)


def planted_case():
    """40 accessions x 600 rows on two chromosomes: calls drawn independently (30 % alt, 6 % missing, 3 % het), accession 29 a copy of
    7, accession 33 a copy of 12 except at three rows, where the two are homozygous and different"""
    rng = np.random.default_rng(PLANTED_SEED)
    n_rows, n_acc = 600, 40
    snps = (rng.random((n_rows, n_acc)) < 0.3).astype(np.int8)
    u = rng.random((n_rows, n_acc))
    snps[u < 0.06] = -1
    snps[(u >= 0.06) & (u < 0.09)] = 2
    snps[:, PLANTED_TWINS[1]] = snps[:, PLANTED_TWINS[0]]
    snps[:, PLANTED_HIDDEN[1]] = snps[:, PLANTED_HIDDEN[0]]
    for r in PLANTED_HIDDEN_ROWS:
        snps[r, PLANTED_HIDDEN[0]], snps[r, PLANTED_HIDDEN[1]] = 0, 1
    chrs = np.array(["Chr1", "Chr2"])
    chr_regions = np.array([[0, 350], [350, 600]])
    positions = np.concatenate([101 + 1000 * np.arange(350), 101 + 1000 * np.arange(250)]).astype(np.int64)
    names = np.array(["acc%02d" % a for a in range(n_acc)])
    return {"snps": snps, "names": names, "positions": positions, "chrs": chrs, "chr_regions": chr_regions}
