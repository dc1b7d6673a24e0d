#!/usr/bin/env python3
"""
Generate tests/golden/gcross_table.npz: what the rule of ``getWindowGenotype`` says, at 50 digits, of EVERY count tuple a window
of up to 40 rows can give.  Needs ``mpmath`` (1.3.0 was used); the tests read the file and need none.  Run from the repo root:

    python tests/golden/make_golden_gcross_table.py

A second run writes the same bytes (the script says so itself when a file is already there).

The tuples are the distinct ``(m1, mh, m2, tot)`` that ``tests/gcross_table.build`` produces for the six ordered parent pairs and
``tot`` 1..40: all ``(a, h, b)`` with ``a + h + b <= tot`` for parents 0 / 1, and the overlapping counts ``m1 == mh`` / ``m2 == mh``
that a heterozygous parent makes.  The decisions come from ``gcross_table.reference_decide`` (``mpmath``, 50 digits, equality of
likelihoods decided on the counts); nothing of the reference project is run or read.

    key    int8    [k, 4]   (tot, m1, mh, m2), lexicographic
    call   int8    [k, 3]   the call (-1 NA, 0, 1, 2) for lr_thres 1.0, 1.5 and 2.706, n_marker_thres 5
    ratio  float64 [k]      the runner-up ratio (smallest ratio other than 1), rounded from 50 digits; NaN where there is none.
                            It does not depend on either threshold and is stored for windows below 5 rows too
    high   int8    [k]      first class with the smallest likelihood (-1: all NaN);  tie  bool [k]  more than one ratio equal to 1
                            (with ``ratio`` these give the call for any thresholds: ``gcross_table.stored_decide``)
    thresholds float64 [3], n_marker_thres int
    min_distance float64 [3]  smallest |ratio - thres| / thres at 50 digits over the tuples whose call consults the threshold
                              (no tie, heterozygous not the most likely, a runner-up exists), windows below 5 rows included
    consulted  int64          how many tuples that is
    lik    float64 [41, 41]   likeliTest(tot, m) at [m, tot] for 1 <= m < tot <= 40 rounded from 50 digits, NaN elsewhere
"""
import hashlib
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import gcross_table as gt  # noqa: E402


def distinct_tuples():
    found = set()
    for parents in gt.PARENT_PAIRS:
        for tot in range(1, gt.TOP_TOT + 1):
            found.update((tot, int(a), int(b), int(c)) for a, b, c in np.unique(gt.true_counts(gt.triples(tot), parents), axis=0))
    return sorted(found)


def main():
    mp = gt._mp()
    keys = distinct_tuples()
    k = len(keys)
    call = np.empty((k, 3), dtype=np.int8)
    ratio = np.empty(k, dtype=np.float64)
    high = np.empty(k, dtype=np.int8)
    tie = np.empty(k, dtype=bool)
    nearest = [None, None, None]
    consulted = 0
    for i, (tot, m1, mh, m2) in enumerate(keys):
        high[i], tie[i], exact = gt.reference_parts(m1, mh, m2, tot)
        ratio[i] = gt.reference_decide(m1, mh, m2, tot, 1.5, n_marker_thres=0)[1]
        for j, thres in enumerate(gt.THRESHOLDS):
            call[i, j] = gt.reference_decide(m1, mh, m2, tot, thres, gt.N_MARKER_THRES)[0]
        if exact is not None and not tie[i] and high[i] != 1:
            consulted += 1
            for j, thres in enumerate(gt.THRESHOLDS):
                d = abs(exact - mp.mpf(thres)) / mp.mpf(thres)
                nearest[j] = d if nearest[j] is None or d < nearest[j] else nearest[j]
    lik = np.full((gt.TOP_TOT + 1, gt.TOP_TOT + 1), np.nan)
    for tot in range(2, gt.TOP_TOT + 1):
        for m in range(1, tot):
            lik[m, tot] = float(gt.reference_likeli(m, tot))
    out = os.path.join(HERE, "gcross_table.npz")
    before = hashlib.sha256(open(out, "rb").read()).hexdigest() if os.path.exists(out) else None
    np.savez_compressed(out, key=np.array(keys, dtype=np.int8), call=call, ratio=ratio, high=high, tie=tie,
                        thresholds=np.array(gt.THRESHOLDS), n_marker_thres=np.array(gt.N_MARKER_THRES),
                        min_distance=np.array([float(d) for d in nearest]), consulted=np.array(consulted, dtype=np.int64), lik=lik)
    after = hashlib.sha256(open(out, "rb").read()).hexdigest()
    print("gcross_table.npz %d bytes  sha256 %s  %s" % (os.path.getsize(out), after[:16],
                                                      "(new)" if before is None else "(same bytes as before)" if before == after else "(CHANGED)"))
    print("%d tuples, %d consult the threshold; smallest relative distance to 1.0 / 1.5 / 2.706: %s" % (
        k, consulted, " / ".join(mp.nstr(d, 6) for d in nearest)))
    print("calls per threshold (NA, 0, 1, 2): %s" % [np.bincount(call[:, j].astype(int) + 1, minlength=4).tolist() for j in range(3)])


if __name__ == "__main__":
    main()
