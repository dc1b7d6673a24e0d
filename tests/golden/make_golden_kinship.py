#!/usr/bin/env python3
"""
Generate tests/golden/kinship_*.npz by RUNNING THE UNMODIFIED REFERENCE ``calc_kinship_mat`` and ``Genotype.kinship_given_snps``
(SNPmatch v5.0.1, expected at /root/reference).  Run from the repo root with an interpreter whose scipy still has ``scipy.mat``
and ``scipy.zeros`` (removed from scipy 1.12 on; the fixtures were written with scipy 1.7.1):

    /opt/conda/bin/python3.9 tests/golden/make_golden_kinship.py

How the reference is driven (nothing of it is modified or copied; the prelude is the one of make_golden_pairsnp.py):
  * ``allel``, ``h5py``, ``hmmlearn(.hmm)`` are only imported at the top of reference files: empty placeholder modules stand in;
  * ``calc_kinship_mat(snps, return_counts=True)`` and ``calc_kinship_mat(snps)`` run on whole arrays;
  * ``kinship_given_snps`` runs UNMODIFIED as a method of a ``Genotype`` made without its constructor (which opens HDF5 files): the
    stub carries ``g.snps`` (a numpy array) and ``accessions``, the only attributes the method reads.  It is called with an
    explicit ``filter_acc_ix`` (with ``None`` the method indexes with ``[:, None]`` and fails) and ``filter_snp_ix=None`` (a given
    list is overwritten by ``arange(len)`` at its line 272).  From 1001 rows on its 1000-row chunk loop runs more than once.

Per case the fixture keeps the panel, the reference's two count matrices (fp64, exact integers), its kinship of the whole array,
the accession list given to the method and the method's kinship.  After the reference has spoken the numpy twin
(tests/kinship_twin.py) must reproduce every count and every kinship bit (``nan`` where the reference has ``nan``), and no zero of
a reference kinship may be a negative zero (the twin's division of integers cannot produce one): both are ASSERTED here.

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

sys.path.insert(0, os.path.join(ROOT, "tests"))
import kinship_twin  # noqa: E402

ACCESSIONS = [1, 2, 7]
ROWS = [1, 999, 1000, 1001, 2500]


def panel(rng, n_rows, n_acc):
    """-1 / 0 / 1 / 2 mixed.  With seven accessions: column 2 entirely missing (a nan row and column of the kinship), column 4 equal
    to column 3, columns 5 and 6 never informative in the same row (5 on even rows, 6 on odd ones)."""
    snps = rng.choice(np.array([-1, 0, 1, 2], dtype=np.int8), size=(n_rows, n_acc), p=[0.15, 0.45, 0.32, 0.08])
    if n_acc >= 7:
        snps[:, 2] = -1
        snps[:, 4] = snps[:, 3]
        snps[1::2, 5] = -1
        snps[0::2, 6] = -1
    return snps


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


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
    rng = np.random.default_rng(7000 + 10 * n_rows + n_acc)
    snps = panel(rng, n_rows, n_acc)
    k_mat, num_snps = ref_snp_genotype.calc_kinship_mat(snps, return_counts=True)
    kin = ref_snp_genotype.calc_kinship_mat(snps)
    k_mat, num_snps, kin = (np.asarray(m, dtype=np.float64) for m in (k_mat, num_snps, kin))
    # the method, on a stub genotype, for a shuffled accession list with one repeat (numpy fancy indexing counts it as listed)
    acc_ix = rng.permutation(n_acc)
    if n_acc > 1:
        acc_ix = np.append(acc_ix, acc_ix[0])
    stub = ref_snp_genotype.Genotype.__new__(ref_snp_genotype.Genotype)
    stub.g = types.SimpleNamespace(snps=snps)
    stub.accessions = np.array(["A%d" % i for i in range(n_acc)])
    method_kin = np.asarray(stub.kinship_given_snps(filter_acc_ix=acc_ix, filter_snp_ix=None), dtype=np.float64)
    # the twin reproduces the reference
    ninfo, same, diff = kinship_twin.kinship_counts(snps)
    assert np.array_equal(ninfo, num_snps) and np.array_equal(same.astype(np.int64) - diff, k_mat)
    assert same_bits(kinship_twin.kinship(ninfo, same, diff), kin)
    assert same_bits(kinship_twin.kinship(*kinship_twin.kinship_counts(snps, cols=acc_ix)), method_kin)
    for m in (kin, method_kin):
        assert not np.any(np.signbit(m) & (m == 0)), "a negative zero in a reference kinship"
    if n_acc >= 7:
        assert np.isnan(kin[2]).all() and np.isnan(kin[:, 2]).all() and np.isnan(kin[5, 6]) and num_snps[5, 6] == 0
        assert np.array_equal(num_snps[3], num_snps[4]) and (n_rows < 2 or kin[3, 4] == kin[3, 3])
    name = "kinship_a%d_r%d" % (n_acc, n_rows)
    out = os.path.join(HERE, name + ".npz")
    save(out, snps=snps, k_mat=k_mat, num_snps=num_snps, kinship=kin, acc_ix=acc_ix.astype(np.int64), method_kinship=method_kin)
    assert os.path.getsize(out) < 20000
    print("%-22s %6d bytes  nan cells %d" % (name, os.path.getsize(out), int(np.isnan(kin).sum())))


if __name__ == "__main__":
    for n_acc in ACCESSIONS:
        for n_rows in ROWS:
            one(n_acc, n_rows)
