"""numpy twin of ``snpm_panel_ibd_counts`` / ``k_ibd_count`` / ``k_ibd_runs`` (test infrastructure, written from the definition and
not from the library code): for every pair of accession columns the windows in which the two are identical, and the runs they form.
Per window the indicator products run in fp64 through BLAS (sums of 0/1 products far below 2^53: exact) and are converted to int64.

Per cell (a, b) -- positions in the column list -- and window: n = rows where both calls are homozygous (0 or 1), d = rows among
them where the two differ.  Hets, every other code and missing calls count nowhere.  A window is *used* iff n >= min_win_sites,
*shared* iff used and d * 1 000 000 <= max_diff_ppm * n (integers), a *break* iff used and not shared.  Scanned in order, a run is a
maximal set of shared windows without a break between two consecutive members; unused windows neither break a run nor count in
it; its length is its number of shared windows; it is reported when its length is at least min_run."""
import numpy as np

PPM = 1000000


def _select(snps, cols, rows):
    v = np.asarray(snps)
    if rows is not None:
        v = v[np.arange(rows.start, rows.stop) if isinstance(rows, range) else rows, :]
    if cols is not None:
        v = v[:, np.asarray(cols, dtype=np.int64)]
    return v


def _window_nd(v):
    """(n, d) int64 [k, k] of one window's rows"""
    f0, f1 = (v == 0).astype(np.float64), (v == 1).astype(np.float64)
    hom = f0 + f1
    n = hom.T @ hom
    same = f0.T @ f0 + f1.T @ f1
    return np.rint(n).astype(np.int64), np.rint(n - same).astype(np.int64)


def _check(win_off, n_rows, min_win_sites, max_diff_ppm, min_run):
    win_off = np.asarray(win_off, dtype=np.int64)
    assert win_off[0] == 0 and win_off[-1] == n_rows and (np.diff(win_off) >= 0).all()
    assert int(min_win_sites) >= 1 and 0 <= int(max_diff_ppm) <= PPM and int(min_run) >= 1
    return win_off


def window_counts(snps, win_off, cols=None, rows=None):
    """(n, d) int64 [n_win, k, k] of every cell and window (small inputs)"""
    v = _select(snps, cols, rows)
    win_off = np.asarray(win_off, dtype=np.int64)
    k = v.shape[1]
    n, d = (np.zeros((len(win_off) - 1, k, k), dtype=np.int64) for _ in range(2))
    for w, (lo, hi) in enumerate(zip(win_off[:-1].tolist(), win_off[1:].tolist())):
        if hi > lo:
            n[w], d[w] = _window_nd(v[lo:hi])
    return n, d


def pair_windows(snps, win_off, a, b, cols=None, rows=None):
    """the raw (n, d) of every window for the cell (a, b), int64 [n_win, 2], row by row from the rules"""
    v = _select(snps, cols, rows)
    x, y = v[:, a].astype(np.int64), v[:, b].astype(np.int64)
    both = ((x == 0) | (x == 1)) & ((y == 0) | (y == 1))
    out = np.zeros((len(win_off) - 1, 2), dtype=np.int64)
    for w, (lo, hi) in enumerate(zip(win_off[:-1], win_off[1:])):
        out[w] = (both[lo:hi].sum(), (both[lo:hi] & (x[lo:hi] != y[lo:hi])).sum())
    return out


def states(n, d, min_win_sites, max_diff_ppm):
    """(used, shared) of counts of any shape, by the two integer rules"""
    n, d = np.asarray(n, dtype=np.int64), np.asarray(d, dtype=np.int64)
    used = n >= int(min_win_sites)
    return used, used & (d * PPM <= int(max_diff_ppm) * n)


def runs_of(used, shared, min_run=1):
    """the reported runs of ONE cell from its window states (sequences of booleans), window by window from the rules:
    a list of (first_window, last_window, n_shared)"""
    runs, first, last, length = [], -1, -1, 0
    for w, (u, s) in enumerate(zip(used, shared)):
        if not u:
            continue
        if s:
            if length == 0:
                first = w
            last, length = w, length + 1
        else:
            if length >= int(min_run):
                runs.append((first, last, length))
            length = 0
    if length >= int(min_run):
        runs.append((first, last, length))
    return runs


def pack_bits(flags):
    """bool [n_win, ...] -> uint32 [..., ceil(n_win / 32)]: window w is bit w % 32 of word w / 32"""
    flags = np.asarray(flags, dtype=bool)
    n_win = flags.shape[0]
    out = np.zeros(flags.shape[1:] + ((n_win + 31) // 32,), dtype=np.uint32)
    for w in range(n_win):
        out[..., w >> 5] |= flags[w].astype(np.uint32) << np.uint32(w & 31)
    return out


def ibd_counts(snps, win_off, min_win_sites=20, max_diff_ppm=1000, min_run=1, cols=None, rows=None):
    """snps int8 [n_snp, n_acc] (negative = missing, 0 / 1 homozygous, anything else counts nowhere); win_off [n_win + 1] offsets
    into the selected rows; cols / rows as numpy fancy indices (repeats count as listed; rows also a ``range``) or None for all.
    Returns a dict: w_used, w_shared, n_shared, d_shared, run_max, n_runs, w_in_runs int32 [k, k], used_bits, shared_bits uint32
    [k, k, ceil(n_win / 32)].  The windows are walked in order, all cells at once; the open run of every cell is one integer."""
    v = _select(snps, cols, rows)
    win_off = _check(win_off, len(v), min_win_sites, max_diff_ppm, min_run)
    k, n_win = v.shape[1], len(win_off) - 1
    w_used, w_shared, n_shared, d_shared, run_max, n_runs, w_in_runs, open_len = (np.zeros((k, k), dtype=np.int64) for _ in range(8))
    used_bits, shared_bits = (np.zeros((k, k, (n_win + 31) // 32), dtype=np.uint32) for _ in range(2))

    def close(where):
        closing = np.where(where, open_len, 0)
        np.maximum(run_max, closing, out=run_max)
        reported = closing >= int(min_run)                          # (min_run >= 1: a cell that closes nothing reports nothing)
        np.add(n_runs, reported, out=n_runs)
        np.add(w_in_runs, np.where(reported, closing, 0), out=w_in_runs)
        np.subtract(open_len, closing, out=open_len)
    for w, (lo, hi) in enumerate(zip(win_off[:-1].tolist(), win_off[1:].tolist())):
        if hi == lo:
            continue                        # an empty window: n = 0 < min_win_sites, unused
        n, d = _window_nd(v[lo:hi])
        used, shared = states(n, d, min_win_sites, max_diff_ppm)
        w_used += used
        w_shared += shared
        n_shared += np.where(shared, n, 0)
        d_shared += np.where(shared, d, 0)
        used_bits[:, :, w >> 5] |= used.astype(np.uint32) << np.uint32(w & 31)
        shared_bits[:, :, w >> 5] |= shared.astype(np.uint32) << np.uint32(w & 31)
        open_len += shared
        close(used & ~shared)
    close(np.ones((k, k), dtype=bool))
    out = {name: m.astype(np.int32) for name, m in (("w_used", w_used), ("w_shared", w_shared), ("n_shared", n_shared), ("d_shared", d_shared),
                                                    ("run_max", run_max), ("n_runs", n_runs), ("w_in_runs", w_in_runs))}
    out.update(used_bits=used_bits, shared_bits=shared_bits)
    return out


def ibd_counts_direct(snps, win_off, min_win_sites=20, max_diff_ppm=1000, min_run=1):
    """the same nine arrays cell by cell through ``pair_windows`` and ``runs_of`` (small inputs)"""
    k, n_win = np.asarray(snps).shape[1], len(win_off) - 1
    names = ("w_used", "w_shared", "n_shared", "d_shared", "run_max", "n_runs", "w_in_runs")
    out = {name: np.zeros((k, k), dtype=np.int32) for name in names}
    out.update(used_bits=np.zeros((k, k, (n_win + 31) // 32), dtype=np.uint32), shared_bits=np.zeros((k, k, (n_win + 31) // 32), dtype=np.uint32))
    for a in range(k):
        for b in range(k):
            nd = pair_windows(snps, win_off, a, b)
            used, shared = states(nd[:, 0], nd[:, 1], min_win_sites, max_diff_ppm)
            every = runs_of(used, shared, 1)
            reported = runs_of(used, shared, min_run)
            out["w_used"][a, b], out["w_shared"][a, b] = used.sum(), shared.sum()
            out["n_shared"][a, b], out["d_shared"][a, b] = nd[shared, 0].sum(), nd[shared, 1].sum()
            out["run_max"][a, b] = max([r[2] for r in every] or [0])
            out["n_runs"][a, b], out["w_in_runs"][a, b] = len(reported), sum(r[2] for r in reported)
            out["used_bits"][a, b], out["shared_bits"][a, b] = pack_bits(used), pack_bits(shared)
    return out


# ------------------------------------------------------------------------------------------------ the planted case
PLANTED_SEED = 31
PLANTED_BIN = 1000                     # bp per window: 100 DB rows, ten bp apart
PLANTED_WINDOWS = (18, 12)             # of Chr1, Chr2
# (a, b, chromosome, first window, last window): b copies a over those windows of that chromosome
PLANTED_COPIES = ((3, 17, 0, 5, 14), (8, 21, 1, 2, 9), (5, 30, 0, 10, 16))
PLANTED_NOISY = (8, 21, 1, 6)          # ... except this window, where 5 of the 100 rows differ
PLANTED_BLANK = (5, 30, 0, (12, 13))   # ... and these windows, where every call of b is missing
# the reported runs at --min_run 3 with the default thresholds: (chromosome, first window, last window, shared windows)
PLANTED_RUNS = {(3, 17): [(0, 5, 14, 10)], (8, 21): [(1, 2, 5, 4), (1, 7, 9, 3)], (5, 30): [(0, 10, 16, 5)]}


def planted_case():
    """A DB of 40 accessions on two chromosomes of 18 and 12 windows of 100 rows each (numpy.random.default_rng(PLANTED_SEED)).
    Every accession is a common ancestor with each call flipped at a rate that makes two accessions differ at about 30 % of the
    rows; 5 % of the calls are missing and 1 % heterozygous.  Then PLANTED_COPIES / PLANTED_NOISY / PLANTED_BLANK are planted.
    The generator asserts that no other pair of accessions has a single shared window at the default thresholds (20 sites, 1000 ppm).
    Returns a dict: snps, names, positions, chrs, chr_regions (the DB), genome (the content of a genome JSON), win_off and win_chr
    over all rows."""
    rng = np.random.default_rng(PLANTED_SEED)
    per, na = 100, 40
    n = per * sum(PLANTED_WINDOWS)
    flip = (1.0 - np.sqrt(1.0 - 2.0 * 0.30)) / 2.0                # 2 q (1 - q) = 0.30
    ancestor = rng.integers(0, 2, n).astype(np.int8)
    db = np.where(rng.random((n, na)) < flip, 1 - ancestor[:, None], ancestor[:, None]).astype(np.int8)
    u = rng.random((n, na))
    db[u < 0.05] = -1
    db[(u >= 0.05) & (u < 0.06)] = 2
    chr_row0 = (0, per * PLANTED_WINDOWS[0])

    def rows_of(c, w_lo, w_hi):
        return np.arange(chr_row0[c] + per * w_lo, chr_row0[c] + per * (w_hi + 1))
    for a, b, c, w_lo, w_hi in PLANTED_COPIES:
        r = rows_of(c, w_lo, w_hi)
        db[r, b] = db[r, a]
    a, b, c, w = PLANTED_NOISY
    r = rows_of(c, w, w)
    r = r[(db[r, a] == 0) | (db[r, a] == 1)][:5]
    assert len(r) == 5
    db[r, b] = 1 - db[r, a]
    a, b, c, ws = PLANTED_BLANK
    for w in ws:
        db[rows_of(c, w, w), b] = -1
    win_off = np.arange(0, n + 1, per, dtype=np.int64)
    win_chr = np.repeat([0, 1], PLANTED_WINDOWS)
    # the decoys stay below the threshold: no pair outside the planted three shares a single window
    got = ibd_counts(db, win_off, 20, 1000, 1)
    decoy = ~np.eye(na, dtype=bool)
    for a, b, _, _, _ in PLANTED_COPIES:
        decoy[a, b] = decoy[b, a] = False
    assert got["w_shared"][decoy].max() == 0 and got["w_used"][decoy].min() >= len(win_off) - 1 - len(PLANTED_BLANK[3]), "choose another seed"
    positions = np.concatenate([np.arange(10, 10 + 10 * per * k, 10) for k in PLANTED_WINDOWS]).astype(np.int64)
    regions = np.array([[0, chr_row0[1]], [chr_row0[1], n]], dtype=np.int64)
    genome = {"ref_chrs": ["Chr1", "Chr2"], "ref_chrlen": [10 * per * k + 1 for k in PLANTED_WINDOWS]}
    return dict(snps=db, names=np.array(["acc%02d" % i for i in range(na)]), positions=positions, chrs=np.array(["Chr1", "Chr2"]),
                chr_regions=regions, genome=genome, win_off=win_off, win_chr=win_chr)
