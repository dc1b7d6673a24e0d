"""numpy twin of ``snpm_pair_counts`` / ``k_pair_count`` (test infrastructure): common and matching record counts of every pair of
samples, per segment.

Written from the rule, one integer matrix product per id that occurs:
  P = ids != 0;  common = P.T @ P;  match = sum over k >= 1 of (ids == k).T @ (ids == k)
"""
import numpy as np


def pair_counts(ids, seg_off):
    """(common, match), both int32 [n_seg, n_samples, n_samples]"""
    ids = np.asarray(ids, dtype=np.uint8)
    seg_off = np.asarray(seg_off, dtype=np.int64)
    n_seg, ns = len(seg_off) - 1, ids.shape[1]
    common = np.zeros((n_seg, ns, ns), dtype=np.int64)
    match = np.zeros((n_seg, ns, ns), dtype=np.int64)
    for s in range(n_seg):
        part = ids[seg_off[s]:seg_off[s + 1]]
        present = (part != 0).astype(np.int64)
        common[s] = present.T @ present
        for k in np.unique(part):
            if k:
                one = (part == k).astype(np.int64)
                match[s] += one.T @ one
    assert common.max(initial=0) < 2 ** 31
    return common.astype(np.int32), match.astype(np.int32)
