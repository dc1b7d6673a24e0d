"""The numpy twin of ``snpm_panel_window_counts`` (csrc/snpm_k_win.hpp): per window of the selected rows the call counts of every listed
column and the agreement counts of listed pairs of columns, from a host panel [rows, accessions] of -1 / 0 / 1 / 2 / 3, and the two
values the reference derives from them (core/snp_genotype.py:297-345) in its own arithmetic.  Test infrastructure: slow and plain."""
import numpy as np


def _select(snps, cols, rows):
    snps = np.asarray(snps)
    if rows is not None:
        snps = snps[np.asarray(rows if not isinstance(rows, range) else list(rows), dtype=np.int64)]
    if cols is not None:
        snps = snps[:, np.asarray(cols, dtype=np.int64)]
    return snps.astype(np.int64)


def _per_window(flags, win_off):
    """sums of the 0 / 1 flags [rows, ...] over the rows of every window: differences of a running sum, so an empty window is zero"""
    run = np.concatenate([np.zeros((1,) + flags.shape[1:], dtype=np.int64), np.cumsum(flags, axis=0, dtype=np.int64)])
    win_off = np.asarray(win_off, dtype=np.int64)
    return run[win_off[1:]] - run[win_off[:-1]]


def window_counts(snps, win_off, cols=None, pairs=None, rows=None):
    """(acc_counts int32 [n_win, n_cols, 4], pair_counts int32 [n_pairs, n_win, 4] or None)"""
    v = _select(snps, cols, rows)
    win_off = np.asarray(win_off, dtype=np.int64)
    assert win_off[0] == 0 and win_off[-1] == len(v) and (np.diff(win_off) >= 0).all()
    acc = np.stack([_per_window(v == 0, win_off), _per_window(v == 1, win_off), _per_window(v == 2, win_off), _per_window(v >= 0, win_off)], axis=-1)
    if pairs is None:
        return acc.astype(np.int32), None
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    out = np.zeros((len(pairs), len(win_off) - 1, 4), dtype=np.int64)
    for i, (a, b) in enumerate(pairs.tolist()):
        x, y = v[:, a], v[:, b]
        both = (x >= 0) & (x <= 2) & (y >= 0) & (y <= 2)
        hom = both & (x <= 1) & (y <= 1)
        out[i] = np.stack([_per_window(both, win_off), _per_window(both & (x == y), win_off), _per_window(hom & (x == y), win_off),
                           _per_window(hom & (x != y), win_off)], axis=-1)
    return acc.astype(np.int32), out.astype(np.int32)


def brute_counts(snps, win_off, cols=None, pairs=None, rows=None):
    """the same by loops over windows, rows and columns"""
    v = _select(snps, cols, rows)
    n_win = len(win_off) - 1
    acc = np.zeros((n_win, v.shape[1], 4), dtype=np.int32)
    pairs = np.zeros((0, 2), dtype=np.int64) if pairs is None else np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    out = np.zeros((len(pairs), n_win, 4), dtype=np.int32)
    for w in range(n_win):
        for r in range(int(win_off[w]), int(win_off[w + 1])):
            for c in range(v.shape[1]):
                x = v[r, c]
                if 0 <= x <= 2:
                    acc[w, c, x] += 1
                acc[w, c, 3] += x >= 0
            for i, (a, b) in enumerate(pairs.tolist()):
                x, y = v[r, a], v[r, b]
                if 0 <= x <= 2 and 0 <= y <= 2:
                    out[i, w, 0] += 1
                    out[i, w, 1] += x == y
                    if x <= 1 and y <= 1:
                        out[i, w, 2 if x == y else 3] += 1
    return acc, out


def het(acc_counts, y_min=5):
    """c2 / ninfo of the reference's ``np_get_fraction(.., y_min)``: ``float(x) / y``, nan where y <= y_min"""
    c2, ninfo = np.asarray(acc_counts)[..., 2], np.asarray(acc_counts)[..., 3]
    out = np.full(c2.shape, np.nan)
    for at in np.ndindex(c2.shape):
        if ninfo[at] > y_min:
            out[at] = float(c2[at]) / float(ninfo[at])
    return out


def mismatch(pair_counts):
    """1 - eq / n: what ``1 - np.nanmean(..)`` of the reference's 0 / 1 / nan vector gives; nan where n == 0"""
    eq, n = np.asarray(pair_counts)[..., 1], np.asarray(pair_counts)[..., 0]
    out = np.full(eq.shape, np.nan)
    for at in np.ndindex(eq.shape):
        if n[at] > 0:
            out[at] = 1.0 - float(eq[at]) / float(n[at])
    return out
