#!/usr/bin/env python3
"""
Generate tests/golden/sitestats_*.npz by RUNNING THE UNMODIFIED REFERENCE ``calculate_af_snp_mat``, ``_polarize_snps`` and
``Genotype.get_af_snps`` (SNPmatch v5.0.1, expected at /root/reference).  Run from the repo root:

    python tests/golden/make_golden_sitestats.py

How the reference is driven (nothing of it is modified or copied; the prelude is the one of make_golden_kinship.py):
  * ``allel``, ``h5py``, ``hmmlearn(.hmm)`` are only imported at the top of reference files: empty placeholder modules stand in;
  * ``calculate_af_snp_mat`` runs on the first CALC_ROWS rows of the panel with ``polarize_geno`` 0, 1 and 2, ``return_maf`` both
    ways and ``min_informative`` 0 and 2 (twelve results); ``_polarize_snps`` on the same rows with ``polarize_geno`` 0 and 1;
  * ``get_af_snps`` runs UNMODIFIED as a method of a ``Genotype`` made without its constructor (which opens HDF5 files): the stub
    carries ``g.snps`` (a numpy array), the only attribute the method reads.  It is called with the accession filter ``None``, an
    array with one repeat, and a dict of two overlapping populations of which one has a repeat; with the row filter ``None`` (from
    1001 rows on its 1000-row chunk loop runs more than once: three times at 2500) and a row list that is unsorted with repeats.
    Every case has the calls (None, None), (array, row list) and (dict, row list); the cases up to 1001 rows also (array, None),
    (dict, None) and (None, row list).

Per case the fixture keeps the panel, the filters, ``calc_af`` [the twelve variants in the order of CALC_VARIANTS, row],
``calc_num_alleles``, ``polarized`` [polarize_geno, row, accession] and per method call (and population) one fp64 array [2, row]:
the frequencies and the informative counts.  The dtypes the method returns (int64 counts in the plain form, fp64 in the dict form)
are asserted here.

Panels are 1, 2 and 7 accessions wide, -1 / 0 / 1 / 2 / 3 mixed, with planted rows: all missing, all code 3, all alt, and exactly
half of the accessions alt (the ``> n / 2`` edge of the polarisation: such a row is NOT flipped) -- of the eight listed ones at
seven accessions, of all accessions at two.

After the reference has spoken the numpy twin (tests/sitestats_twin.py) must reproduce every count and every frequency as fp64
bits (``nan`` where the reference has ``nan``): ASSERTED here.

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
import sitestats_twin  # noqa: E402

ACCESSIONS = [1, 2, 7]
ROWS = [1, 999, 1000, 1001, 2500]
CALC_ROWS = 150
CALC_VARIANTS = [(pg, maf, mi) for pg in (0, 1, 2) for maf in (True, False) for mi in (0, 2)]


def acc_filters(n_acc):
    """the array with one repeat, and the two overlapping populations (the second with a repeat)"""
    if n_acc == 1:
        return np.array([0, 0]), {"north": np.array([0]), "south": np.array([0, 0])}
    if n_acc == 2:
        return np.array([1, 0, 1]), {"north": np.array([0, 1]), "south": np.array([1, 1])}
    return np.array([5, 0, 3, 6, 2, 1, 4, 5]), {"north": np.array([0, 1, 2, 3]), "south": np.array([3, 6, 4, 3, 5])}


def panel(rng, n_rows, n_acc, listed):
    snps = rng.choice(np.array([-1, 0, 1, 2, 3], dtype=np.int8), size=(n_rows, n_acc), p=[0.14, 0.42, 0.32, 0.08, 0.04])
    if n_rows >= 5:
        snps[0] = -1
        snps[1] = 3
        snps[2] = 1
        snps[3] = 0                         # exactly half of the LISTED accessions (repeat included) alt
        half, n_alt = len(listed) // 2, 0
        for a in listed:
            if n_alt + int((listed == a).sum()) <= half and snps[3, a] == 0:
                snps[3, a] = 1
                n_alt += int((listed == a).sum())
        assert n_acc == 1 or len(listed) % 2 or 2 * int((snps[3, listed] == 1).sum()) == len(listed)
        if n_acc % 2 == 0:
            snps[4, : n_acc // 2], snps[4, n_acc // 2:] = 1, 0      # ... and of all accessions, where their number is even
    else:
        snps[0] = [-1, 1, 3, 2, 0, 1, 1][:n_acc] if n_acc != 2 else [1, 0]
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
    rng = np.random.default_rng(9000 + 10 * n_rows + n_acc)
    listed, pops = acc_filters(n_acc)
    snps = panel(rng, n_rows, n_acc, listed)
    out = {"snps": snps, "acc_ix": listed.astype(np.int64), "pop_north": pops["north"].astype(np.int64), "pop_south": pops["south"].astype(np.int64)}
    # the two functions on the first rows
    head = snps[:CALC_ROWS]
    counts = sitestats_twin.site_counts(head)
    calc = []
    for pg, maf, mi in CALC_VARIANTS:
        got, num = ref_snp_genotype.calculate_af_snp_mat(head, min_informative=mi, polarize_geno=pg, return_maf=maf)
        assert got.dtype == np.float64 and num.dtype == np.int64
        assert np.array_equal(num, counts[0, :, 3]) and same_bits(sitestats_twin.frequency(counts[0], mi, pg, maf), got)
        calc.append(got)
    out["calc_af"] = np.array(calc)                                  # [variant of CALC_VARIANTS, row]
    out["calc_num_alleles"] = np.asarray(num, dtype=np.int64)
    polarized = []
    for pg in (0, 1):
        pol = ref_snp_genotype._polarize_snps(head, polarize_geno=pg)
        flipped = (pol != head).any(axis=1)
        want = counts[0, :, pg] > head.shape[1] / 2.0
        assert not (flipped & ~want).any()                           # (a flipped row of 2s and 3s only would look unchanged)
        polarized.append(np.asarray(pol, dtype=np.int8))
    out["polarized"] = np.array(polarized)                           # [polarize_geno, row, accession]
    # the method, on a stub genotype
    stub = ref_snp_genotype.Genotype.__new__(ref_snp_genotype.Genotype)
    stub.g = types.SimpleNamespace(snps=snps)
    row_list = rng.integers(0, n_rows, size=max(1, min(n_rows, 1400) // 2)).astype(np.int64)   # unsorted, with repeats
    if len(row_list) > 2:
        row_list[-1] = row_list[0]
    out["row_ix"] = row_list
    # (name, accession filter, row filter, no_accs_missing_info, polarize_geno, return_maf)
    calls = [("all", None, None, 0, 1, True), ("listed_rows", listed, row_list, 0, 0, True), ("pops_rows", pops, row_list, 2, 1, False)]
    if n_rows <= 1001:                      # (the 2500-row fixtures stay below 20 kB without these)
        calls += [("listed", listed, None, 1, 1, False), ("pops", pops, None, 0, 1, True), ("all_rows", None, row_list, 0, 2, False)]
    for name, acc, rows, mi, pg, maf in calls:
        got, nind = stub.get_af_snps(mi, return_nind=True, filter_snps_ix=rows, filter_acc_ix=acc, polarize_geno=pg, return_maf=maf)
        only = stub.get_af_snps(mi, filter_snps_ix=rows, filter_acc_ix=acc, polarize_geno=pg, return_maf=maf)
        groups = None if acc is None else ([acc[k] for k in acc] if isinstance(acc, dict) else [acc])
        twin = sitestats_twin.site_counts(snps, groups, rows)
        if isinstance(acc, dict):
            assert list(got) == list(acc) == ["north", "south"]
            for k, pop in enumerate(acc):
                assert got[pop].dtype == np.float64 and nind[pop].dtype == np.float64 and same_bits(only[pop], got[pop])
                assert np.array_equal(nind[pop], twin[k, :, 3]) and same_bits(sitestats_twin.frequency(twin[k], mi, pg, maf), got[pop])
                out["m_%s_%s" % (name, pop)] = np.array([got[pop], nind[pop]])      # [af | nind, row]
        else:
            assert got.dtype == np.float64 and nind.dtype == np.int64 and same_bits(only, got)
            assert np.array_equal(nind, twin[0, :, 3]) and same_bits(sitestats_twin.frequency(twin[0], mi, pg, maf), got)
            out["m_%s" % name] = np.array([got, nind.astype(np.float64)])
    if n_rows >= 5:
        c = sitestats_twin.site_counts(snps, [listed])[0]
        assert c[0, 3] == 0 and np.isnan(out["m_all"][0, 0])                                   # all missing
        assert c[1].tolist() == [0, 0, 0, len(listed)] and out["m_all"][0, 1] == 0.0            # all code 3: informative, no allele
        assert c[2, 1] == len(listed) and out["m_listed_rows"].shape[0] == 2                           # all alt
        assert len(listed) % 2 or n_acc == 1 or (2 * c[3, 1] == len(listed) and not (out["polarized"][1, 3] != snps[3]).any())
        assert (out["polarized"][1, 2] == 0).all()                                               # all alt: flipped
    name = "sitestats_a%d_r%d" % (n_acc, n_rows)
    path = os.path.join(HERE, name + ".npz")
    save(path, **out)
    assert os.path.getsize(path) < 20000, (name, os.path.getsize(path))
    print("%-24s %6d bytes  members %d" % (name, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    for n_acc in ACCESSIONS:
        for n_rows in ROWS:
            one(n_acc, n_rows)
