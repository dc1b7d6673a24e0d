#!/usr/bin/env python3
"""
Generate tests/golden/windows_*.npz by RUNNING THE UNMODIFIED REFERENCE ``Genotype.calculate_heterozygosity_windows`` and
``Genotype.mismatch_between_accs`` (SNPmatch v5.0.1, expected at /root/reference).  Run from the repo root:

    python tests/golden/make_golden_windows.py

How the reference is driven (nothing of it is modified or copied; the prelude is the one of make_golden_sitestats.py):
  * ``allel``, ``h5py``, ``hmmlearn(.hmm)`` are only imported at the top of reference files: empty placeholder modules stand in;
  * both methods run UNMODIFIED as methods of a ``Genotype`` made without its constructor (which opens HDF5 files): ``g.g`` and
    ``g.g_acc`` are duck-typed on a numpy panel (``snps``, ``accessions``, ``positions``, ``chrs``, ``chr_regions``);
  * the ``Genome`` is the reference's own class on a toy JSON of this repository (tests/golden/windows_toy_genome.json: Chr1 of
    1000 bp, Chr2 of 650 bp), so its ``get_bins_genome`` cuts the windows.

Panels are 2 and 7 accessions wide, -1 / 0 / 1 / 2 / 3 mixed; window lengths 100 and 300.  Planted (asserted below):
  * a window with every call missing (Chr1 101-200 at 100 bp; Chr2 301-600 at both lengths);
  * ``ninfo`` exactly 5 and exactly 6 for one accession -- accession 0 in Chr1 201-300 / 301-400 at 100 bp, accession 1 in
    Chr1 601-900 / Chr2 1-300 at 300 bp: the ``y_min = 5`` edge, nan at 5 and a value at 6;
  * a window where the pair (0, 1) never shares a call (Chr1 501-600 at 100 bp, Chr2 601-900 at 300 bp);
  * rows past the last window of their chromosome (Chr2 positions above 700 at 100 bp, above 900 at both lengths);
  * windows without a row (Chr1 401-500 at 100 bp, Chr1 901-1000 / 901-1200 at both lengths).
If the reference raised on a window without rows the generator would say so and stop: it does not (RAISED_ON_EMPTY below is
asserted False), so every window is in the fixtures.

Per case the fixture keeps the panel, positions, chr_regions, the window table (chr_ix, start, end, first, last -- first / last from
the reference's member lists), the index of the het frame, ``het`` [window, accession] for all accessions, ``het_listed`` for
``sample_ix`` = LISTED (with a repeat), and per pair of PAIRS ``mismatch`` [pair, window] and the per-row vector ``mismatch_rows``
[pair, row] of ``bin_length=None``.  The frames' shapes, column names and dtypes are asserted here.

After the reference has spoken the numpy twin (tests/windows_twin.py) must reproduce every value as fp64 bits (``nan`` where the
reference has ``nan``): ASSERTED here.

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

from snpmatch.core import genomes as ref_genomes  # noqa: E402
from snpmatch.core import snp_genotype as ref_snp_genotype  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import windows_twin  # noqa: E402

TOY_GENOME = os.path.join(HERE, "windows_toy_genome.json")
ACCESSIONS = [2, 7]
WINDOWS = [100, 300]
PAIRS = {2: [(0, 1), (1, 0), (0, 0)], 7: [(0, 1), (1, 0), (0, 0), (2, 5), (6, 3)]}
LISTED = {2: [1, 0, 1], 7: [5, 0, 3, 6, 5]}
RAISED_ON_EMPTY = False


def positions():
    """(Chr1, Chr2): sorted, none in Chr1 401-500 and 901-1000, some of Chr2 past 700 and past 900"""
    rng = np.random.default_rng(1900)
    chr1 = np.sort(rng.choice(np.concatenate([np.arange(1, 401), np.arange(501, 901)]), size=150, replace=False))
    chr2 = np.concatenate([np.sort(rng.choice(np.arange(1, 701), size=110, replace=False)), [703, 711, 720, 905, 910]])
    return chr1.astype(np.int64), chr2.astype(np.int64)


def panel(n_acc):
    rng = np.random.default_rng(1900 + n_acc)
    chr1, chr2 = positions()
    n1 = len(chr1)
    pos = np.concatenate([chr1, chr2])
    snps = rng.choice(np.array([-1, 0, 1, 2, 3], dtype=np.int8), size=(len(pos), n_acc), p=[0.12, 0.4, 0.3, 0.12, 0.06])
    on1, on2 = np.arange(len(pos)) < n1, np.arange(len(pos)) >= n1

    def rows(first_chr, lo, hi):
        return np.flatnonzero((on1 if first_chr else on2) & (pos >= lo) & (pos <= hi))

    def exactly(acc, where, k):             # accession `acc` keeps exactly k calls in the rows `where`
        assert len(where) > k
        called = rng.choice(where, size=k, replace=False)
        snps[where, acc] = -1
        snps[called, acc] = rng.choice(np.array([0, 1, 2, 3], dtype=np.int8), size=k)
        snps[called[0], acc] = 2            # (a het among them: the fraction is not zero)

    snps[rows(True, 101, 200)] = -1
    snps[rows(False, 301, 600)] = -1
    exactly(0, rows(True, 201, 300), 5)
    exactly(0, rows(True, 301, 400), 6)
    exactly(1, rows(True, 601, 900), 5)
    exactly(1, rows(False, 1, 300), 6)
    w = rows(True, 501, 600)                # the pair (0, 1) never shares a call
    snps[w[::2], 0], snps[w[1::2], 1] = -1, -1
    snps[w[1::2], 0], snps[w[::2], 1] = 1, 0
    snps[rows(False, 601, 900), 1] = -1
    return snps, pos, np.array([[0, n1], [n1, len(pos)]], dtype=np.int64)


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


def one(n_acc, win):
    snps, pos, regions = panel(n_acc)
    chrs = np.array(["Chr1", "Chr2"])
    db = types.SimpleNamespace(snps=snps, accessions=np.array(["A%d" % i for i in range(n_acc)]).astype("S"), positions=pos, chrs=chrs, chr_regions=regions)
    stub = ref_snp_genotype.Genotype.__new__(ref_snp_genotype.Genotype)
    stub.g, stub.g_acc = db, db
    genome = ref_genomes.Genome(TOY_GENOME)
    bins = list(genome.get_bins_genome(db, win))
    chr_ix = np.array([b[0] for b in bins], dtype=np.int64)
    start, end = (np.array([b[1][k] for b in bins], dtype=np.int64) for k in (0, 1))
    first, last, at = [], [], 0
    for b in bins:
        m = list(b[2])
        assert m == list(range(m[0], m[0] + len(m))) if m else True
        at = m[0] if m else (regions[b[0]][0] if b[1][0] == 1 else at)
        first.append(at)
        at += len(m)
        last.append(at)
    first, last = np.array(first, dtype=np.int64), np.array(last, dtype=np.int64)
    rows_sel = np.concatenate([np.arange(a, b) for a, b in zip(first, last)])
    win_off = np.concatenate([[0], np.cumsum(last - first)])
    out = {"snps": snps, "positions": pos, "chr_regions": regions, "chr_ix": chr_ix, "start": start, "end": end, "first": first, "last": last,
           "pairs": np.array(PAIRS[n_acc], dtype=np.int64), "listed": np.array(LISTED[n_acc], dtype=np.int64)}
    # heterozygosity: all accessions, and a list with a repeat
    acc_counts, pair_counts = windows_twin.window_counts(snps, win_off, None, PAIRS[n_acc], rows_sel)
    for key, ix in (("het", None), ("het_listed", np.array(LISTED[n_acc]))):
        frame = stub.calculate_heterozygosity_windows(genome, win, ix)
        cols = np.arange(n_acc) if ix is None else ix
        assert frame.shape == (len(bins), len(cols)) and list(frame.columns) == list(cols) and all(str(t) == "float64" for t in frame.dtypes)
        assert list(frame.index) == ["%s,%d,%d" % (genome.chrs[c], s, e) for c, s, e in zip(chr_ix, start, end)]
        got = frame.to_numpy(dtype=np.float64)
        assert same_bits(windows_twin.het(acc_counts[:, cols], 5), got), key
        out[key] = got
    out["index"] = np.array(list(frame.index)).astype("U")
    # mismatch: the frame per pair, and the per-row vector
    mism, per_row = [], []
    for i, (x, y) in enumerate(PAIRS[n_acc]):
        frame = stub.mismatch_between_accs(x, y, win, genome)
        assert list(frame.columns) == ["chr", "start", "end", "mismatch"] and frame.shape == (len(bins), 4) and all(str(t) == "object" for t in frame.dtypes)
        assert list(frame["chr"]) == [genome.chrs[c] for c in chr_ix] and list(frame["start"]) == start.tolist() and list(frame["end"]) == end.tolist()
        got = frame["mismatch"].to_numpy(dtype=np.float64)
        assert same_bits(windows_twin.mismatch(pair_counts[i]), got), (x, y)
        mism.append(got)
        vec = stub.mismatch_between_accs(x, y)
        a, b = snps[:, x].astype(int), snps[:, y].astype(int)
        both = (a >= 0) & (a <= 2) & (b >= 0) & (b <= 2)
        assert vec.dtype == np.float64 and np.array_equal(np.isnan(vec), ~both) and np.array_equal(vec[both], (a == b)[both].astype(float))
        per_row.append(vec)
    out["mismatch"], out["mismatch_rows"] = np.array(mism), np.array(per_row)
    # the planted cases
    bed = {t: k for k, t in enumerate(out["index"].tolist())}
    empty = last == first
    assert not RAISED_ON_EMPTY and empty.any() and np.isnan(out["het"][empty]).all() and np.isnan(out["mismatch"][:, empty]).all()
    assert empty[bed["Chr1,901,1000" if win == 100 else "Chr1,901,1200"]] and (win == 300 or empty[bed["Chr1,401,500"]])
    in_window = np.zeros(len(pos), dtype=bool)
    in_window[rows_sel] = True
    assert (~in_window).sum() == (5 if win == 100 else 2) and in_window[:regions[0][1]].all()      # Chr2 rows past its last window
    gone = [bed[t] for t in (["Chr1,101,200", "Chr2,301,400", "Chr2,401,500", "Chr2,501,600"] if win == 100 else ["Chr2,301,600"])]
    assert not acc_counts[gone, :, 3].any() and not empty[gone].any() and np.isnan(out["het"][gone]).all() and np.isnan(out["mismatch"][:, gone]).all()
    acc, five, six = (0, bed["Chr1,201,300"], bed["Chr1,301,400"]) if win == 100 else (1, bed["Chr1,601,900"], bed["Chr2,1,300"])
    assert acc_counts[five, acc, 3] == 5 and acc_counts[six, acc, 3] == 6 and np.isnan(out["het"][five, acc]) and out["het"][six, acc] > 0
    apart = bed["Chr1,501,600"] if win == 100 else bed["Chr2,601,900"]
    assert pair_counts[0, apart, 0] == 0 and acc_counts[apart, 0, 3] > 0 and np.isnan(out["mismatch"][0, apart]) and not empty[apart]
    assert out["mismatch"][2][~np.isnan(out["mismatch"][2])].max() == 0.0                            # an accession against itself
    name = "windows_a%d_w%d" % (n_acc, win)
    path = os.path.join(HERE, name + ".npz")
    save(path, **out)
    assert os.path.getsize(path) < 20000, (name, os.path.getsize(path))
    print("%-20s %6d bytes  windows %d (without rows %d)  members %d" % (name, os.path.getsize(path), len(bins), int(empty.sum()), len(out)))


if __name__ == "__main__":
    for n_acc in ACCESSIONS:
        for win in WINDOWS:
            one(n_acc, win)
