"""numpy twin of ``snpm_cross_calls`` / ``k_gcross`` (test infrastructure): counts and the three-way decision per (window, sample).

Written from the rule, vectorised over all cells:
  value of an element = {0, 1, 2, -1, 0}[class] when its separator bit equals the one of the window's first row of that sample,
  else 0;  m1 = #(value == p1), mh = #(value == 2), m2 = #(value == p2), tot = rows of the window;
  tot < n_marker_thres or no match -> NA;  L_k = likeliTest(tot, m_k);  ratio_k = L_k / nanmin(L);  more than one ratio == 1 -> 1;
  high = nanargmin(L);  lr_next = nanmin of the ratios != 1 (lr_thres when there is none);  0 / 2 need lr_next >= lr_thres.
"""
import numpy as np

CLASS_VALUE = np.array([0, 1, 2, -1, 0, 0, 0, 0], dtype=np.int8)


def counts(codes, p1, p2, win_off):
    """int32 [n_win, n_samples, 3] = (m1, mh, m2)"""
    codes = np.asarray(codes, dtype=np.uint8)
    n, ns = codes.shape
    win_off = np.asarray(win_off, dtype=np.int64)
    n_win = len(win_off) - 1
    sizes = np.diff(win_off)
    first_row = np.repeat(win_off[:-1], sizes)                       # first row of the window every row lies in
    bar = (codes >> 3) & 1
    value = np.where(bar == bar[first_row], CLASS_VALUE[codes & 7], 0).astype(np.int8) if n else np.zeros((0, ns), np.int8)
    p1 = np.asarray(p1, dtype=np.int8).reshape(n, 1)
    p2 = np.asarray(p2, dtype=np.int8).reshape(n, 1)
    out = np.zeros((n_win, ns, 3), dtype=np.int32)
    for k, hit in enumerate((value == p1, value == 2, value == p2)):
        run = np.concatenate([np.zeros((1, ns), dtype=np.int64), np.cumsum(hit, axis=0, dtype=np.int64)])
        out[:, :, k] = run[win_off[1:]] - run[win_off[:-1]]
    return out


def likeli(tot, m):
    """likeliTest on arrays: NaN for tot == 0 or m == 0, 1 for m == tot"""
    tot = np.asarray(tot, dtype=np.float64)
    m = np.asarray(m, dtype=np.float64)
    p = 0.99999999
    with np.errstate(divide="ignore", invalid="ignore"):
        ps = m / tot
        general = m * np.log(ps / p) + (tot - m) * np.log((1 - ps) / (1 - p))
    return np.where((tot == 0) | (m == 0), np.nan, np.where(m == tot, 1.0, general))


def decide(cnt, tot, lr_thres, n_marker_thres=5):
    """(geno int8 [n_win, n_samples] with -1 = NA, lr_next float64 of the same shape: NaN where the threshold is not consulted
    or where lr_next is the threshold itself because no other finite ratio exists)"""
    cnt = np.asarray(cnt)
    tot = np.broadcast_to(np.asarray(tot, dtype=np.int64).reshape(-1, 1), cnt.shape[:2])
    lik = likeli(tot[:, :, None], cnt)
    some = ~np.all(np.isnan(lik), axis=2)
    safe = np.where(np.isnan(lik), np.inf, lik)
    top = safe.min(axis=2)
    high = safe.argmin(axis=2)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where((top > 0)[:, :, None], lik / top[:, :, None], np.nan)
    ties = (ratio == 1).sum(axis=2) > 1
    others = np.where(np.isnan(ratio) | (ratio - 1 == 0), np.inf, ratio).min(axis=2)
    lr_next = np.where(np.isinf(others), lr_thres, others)
    geno = np.full(cnt.shape[:2], -1, dtype=np.int8)
    geno[(high == 0) & (lr_next >= lr_thres)] = 0
    geno[(high == 2) & (lr_next >= lr_thres)] = 2
    geno[high == 1] = 1
    geno[ties] = 1
    undecidable = (tot < n_marker_thres) | ~some
    geno[undecidable] = -1
    consulted = ~undecidable & ~ties & (high != 1)
    # reported: the COMPUTED lr_next only -- where it is lr_thres by substitution no logarithm is involved
    return geno, np.where(consulted & ~np.isinf(others), lr_next, np.nan)


def cross_calls(codes, p1, p2, win_off, lr_thres, n_marker_thres=5):
    """(geno, counts, lr_next)"""
    cnt = counts(codes, p1, p2, win_off)
    geno, lr_next = decide(cnt, np.diff(np.asarray(win_off, dtype=np.int64)), lr_thres, n_marker_thres)
    return geno, cnt, lr_next


KNIFE_EDGE_WIDTH = 1e-9             # relative; tests/test_gpu_gcross_table.py measures what the device and numpy need of it


def knife_edge_cells(lr_next, lr_thres):
    """cells whose lr_next lies within 1e-9 relative of the threshold: a last-bit difference of two log implementations could flip them"""
    with np.errstate(invalid="ignore"):
        return int(np.count_nonzero(np.abs(lr_next - lr_thres) <= KNIFE_EDGE_WIDTH * lr_thres))
