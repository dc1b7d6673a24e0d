#!/usr/bin/env python3
"""
Generate tests/golden/ld_*.npz by RUNNING THE UNMODIFIED REFERENCE module function ``calculate_ld`` (SNPmatch v5.0.1, expected at
/root/reference).  Run from the repo root:

    python tests/golden/make_golden_ld.py

How the reference is driven (nothing of it is modified or copied; the prelude is the one of make_golden_sitestats.py):
  * ``allel``, ``h5py``, ``hmmlearn(.hmm)`` are only imported at the top of reference files: empty placeholder modules stand in;
  * ``calculate_ld`` is written on ``sp.transpose`` / ``sp.mean`` / ``sp.std`` / ``sp.dot``, aliases of numpy's functions that
    scipy has since dropped: the name ``sp`` of the LOADED module is bound to a namespace of numpy's functions of those names --
    what the aliases were -- and the function runs as it stands, on the panel as a float array;
  * the method ``Genotype.calculate_ld`` cannot be driven at all (it indexes the wrong axis and assigns ``nan`` into an int8 array).

Panels are complete (codes 0 / 1 / 2 only: the dense form has no notion of a missing call), 2, 7 and 130 accessions wide and 1, 2
and 200 rows long, with planted rows from five rows on: all ref, all alt, a singleton, its duplicate, its complement.  The
reference takes the codes as numbers, so alt counts 1 and het 2: ``v_alt = 1, v_het = 2`` in this package's terms.

Per case the fixture keeps the panel (``snps``) and the reference's matrix as its upper triangle with the diagonal (``r2_upper``,
in the order of ``np.triu_indices``; the matrix is symmetric: ASSERTED here).

After the reference has spoken the integer formula of the numpy twin (tests/ld_twin.py) must have ``nan`` exactly where the
reference has ``nan``, never exceed 1, and lie within 1e-12 of it: ASSERTED here, and the largest difference is printed per case.

The .npz members are written with a fixed timestamp, so that running this file again gives the same bytes.
"""
import io
import os
import sys
import types
import warnings
import zipfile

import numpy as np

sys.dont_write_bytecode = True
for _m in ("allel", "h5py", "hmmlearn", "hmmlearn.hmm"):
    sys.modules[_m] = types.ModuleType(_m)
sys.modules["hmmlearn"].hmm = sys.modules["hmmlearn.hmm"]
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, "/root/reference")
warnings.filterwarnings("ignore")

import logging  # noqa: E402
logging.disable(logging.CRITICAL)

from snpmatch.core import snp_genotype as ref_snp_genotype  # noqa: E402

ref_snp_genotype.sp = types.SimpleNamespace(transpose=np.transpose, mean=np.mean, std=np.std, dot=np.dot)

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ld_twin  # noqa: E402

ACCESSIONS = [2, 7, 130]
ROWS = [1, 2, 200]
BOUND = 1e-12


def panel(rng, n_rows, n_acc):
    snps = rng.choice(np.array([0, 1, 2], dtype=np.int8), size=(n_rows, n_acc), p=[0.55, 0.37, 0.08])
    if n_rows >= 5:
        snps[0] = 0                         # all ref
        snps[1] = 1                         # all alt
        snps[2] = 0
        snps[2, n_acc // 2] = 1             # a singleton
        snps[3] = snps[2]                   # its duplicate
        snps[4] = 1 - snps[2]               # its complement
    return snps


def save(path, **arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def one(n_acc, n_rows):
    rng = np.random.default_rng(12000 + 10 * n_rows + n_acc)
    snps = panel(rng, n_rows, n_acc)
    with np.errstate(all="ignore"):
        ref = np.asarray(ref_snp_genotype.calculate_ld(snps.astype(np.float64)))
    assert ref.dtype == np.float64 and ref.shape == (n_rows, n_rows)
    nan = np.isnan(ref)
    assert np.array_equal(nan, nan.T) and np.array_equal(ref[~nan], ref.T[~nan])
    twin = ld_twin.dense(snps, np.arange(n_rows), None, v_alt=1, v_het=2, min_n=1)
    assert np.array_equal(np.isnan(twin), nan) and (twin[~nan] <= 1.0).all()
    worst = float(np.abs(twin[~nan] - ref[~nan]).max()) if (~nan).any() else 0.0
    assert worst <= BOUND, worst
    if n_rows >= 5:
        assert nan[0].all() and nan[1].all() and not nan[2, 3]
        assert twin[2, 3] == 1.0 and twin[2, 4] == 1.0 and abs(ref[2, 3] - 1.0) <= BOUND and abs(ref[2, 4] - 1.0) <= BOUND
    name = "ld_a%d_r%d" % (n_acc, n_rows)
    path = os.path.join(HERE, name + ".npz")
    save(path, snps=snps, r2_upper=ref[np.triu_indices(n_rows)])
    assert os.path.getsize(path) < 200000, (name, os.path.getsize(path))
    print("%-14s %7d bytes  defined %6d  max |twin - reference| %.2e" % (name, os.path.getsize(path), int((~nan).sum()), worst))
    return worst


if __name__ == "__main__":
    for n_acc in ACCESSIONS:
        print("accessions %d: max |twin - reference| %.2e" % (n_acc, max(one(n_acc, n_rows) for n_rows in ROWS)))
