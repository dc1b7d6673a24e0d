#!/usr/bin/env python3
"""
Generate tests/golden/simulate_*.npz by RUNNING THE UNMODIFIED REFERENCE ``simulateSNPs`` / ``simulateSNPs_F1`` (SNPmatch v5.0.1,
expected at /root/reference) under ``np.random.seed``.  Run from the repo root:

    python tests/golden/make_golden_simulate.py [OUT_DIR]

(OUT_DIR: write the files there instead of next to this script -- tests/test_simulate_cpu.py compares such a run with the committed
files byte for byte, where the reference is at hand; without the reference this script exits with status 3.)

How the reference is driven (nothing of it is modified or copied; the prelude is the one of make_golden_f1search.py):
  * ``allel``, ``h5py``, ``hmmlearn(.hmm)`` are only imported at the top of reference files: empty placeholder modules stand in;
  * both functions run UNMODIFIED on a duck-typed ``g`` whose ``g.g`` and ``g.g_acc`` carry ``accessions``, ``snps``, ``chromosomes`` and
    ``positions`` of a numpy panel.

The panel: 6 accessions over 300 rows on two chromosomes.  A0 has missing calls and hets, A1 also the code 3, A2 / A3 are homozygous
and differ at many rows, A4 is A2 with other rows missing (a parent pair with no segregating row), A5 has no call.

Cases (asserted below where a property is planted):
  inbred_e0     A0, 50 of its rows, err_rate 0: int(err_rate * n) = 0 -- both draws of zero rows are still made
  inbred_e05    A0, 100 rows, err_rate 0.05: five calls redrawn, the values before the rows
  inbred_all    A0, ALL its informative rows, err_rate 0.05
  inbred_code3  A1, all its informative rows, err_rate 0: the code 3 has no text in snp_binary_to_gt -- the genotype is empty
  f1_h1 / f1_h05 / f1_h0   A2 x A3, 120 rows, err_rate 0.05, het_frac 1 / 0.5 / 0
  f1_noseg      A2 x A4, 60 rows, err_rate 0.05, het_frac 0.5: no het to redraw

Per case the fixture keeps the panel, the arguments, the seed and the returned frame's three columns as str (the reference's frame holds
the genotype as bytes under Python 3: decoded here).

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
REFERENCE = "/root/reference"
if not os.path.isdir(os.path.join(REFERENCE, "snpmatch", "core")):
    sys.stderr.write("the reference is not at %s\n" % REFERENCE)
    sys.exit(3)
sys.path.insert(0, REFERENCE)
warnings.filterwarnings("ignore")

import logging  # noqa: E402
logging.disable(logging.CRITICAL)

from snpmatch.core import simulate as ref_simulate  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else HERE
N_ROWS, N_ACC = 300, 6
CASES = [
    # name, f1, accession / parents, numSNPs (None: all), err_rate, het_frac, seed
    ("inbred_e0", False, "A0", 50, 0.0, 1.0, 11),
    ("inbred_e05", False, "A0", 100, 0.05, 1.0, 12),
    ("inbred_all", False, "A0", None, 0.05, 1.0, 13),
    ("inbred_code3", False, "A1", None, 0.0, 1.0, 14),
    ("f1_h1", True, "A2xA3", 120, 0.05, 1.0, 15),
    ("f1_h05", True, "A2xA3", 120, 0.05, 0.5, 16),
    ("f1_h0", True, "A2xA3", 120, 0.05, 0.0, 17),
    ("f1_noseg", True, "A2xA4", 60, 0.05, 0.5, 18),
]


def panel():
    rng = np.random.default_rng(2200)
    snps = np.empty((N_ROWS, N_ACC), dtype=np.int8)
    snps[:, 0] = rng.choice(np.array([-1, 0, 1, 2], dtype=np.int8), size=N_ROWS, p=[0.15, 0.4, 0.35, 0.1])
    snps[:, 1] = rng.choice(np.array([-1, 0, 1, 2, 3], dtype=np.int8), size=N_ROWS, p=[0.15, 0.35, 0.3, 0.1, 0.1])
    snps[:, 2] = rng.choice(np.array([0, 1], dtype=np.int8), size=N_ROWS)
    snps[:, 3] = rng.choice(np.array([-1, 0, 1, 2], dtype=np.int8), size=N_ROWS, p=[0.1, 0.4, 0.4, 0.1])
    snps[:, 4] = snps[:, 2]
    snps[rng.random(N_ROWS) < 0.3, 4] = -1
    snps[:, 5] = -1
    chromosomes = np.array(["Chr1"] * 170 + ["Chr2"] * 130)
    positions = np.concatenate([np.arange(50, 50 + 170 * 100, 100), np.arange(75, 75 + 130 * 100, 100)]).astype(np.int64)
    return snps, np.array(["A%d" % i for i in range(N_ACC)]), chromosomes, positions


def duck(snps, accessions, chromosomes, positions):
    side = types.SimpleNamespace(snps=snps, accessions=accessions, chromosomes=chromosomes, positions=positions)
    return types.SimpleNamespace(g=side, g_acc=side)


def as_text(column):
    return np.array([v.decode() if isinstance(v, bytes) else str(v) for v in column]).astype("U")


def save(path, **arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def one(name, f1, who, num, err_rate, het_frac, seed):
    snps, accessions, chromosomes, positions = panel()
    g = duck(snps, accessions, chromosomes, positions)
    if f1:
        a, b = (int(t[1:]) for t in who.split("x"))
        pool = int(((snps[:, a] >= 0) & (snps[:, b] >= 0) & (snps[:, a] < 2) & (snps[:, b] < 2)).sum())
    else:
        pool = int((snps[:, int(who[1:])] >= 0).sum())
    num = pool if num is None else num
    np.random.seed(seed)
    if f1:
        frame = ref_simulate.simulateSNPs_F1(g, who, num, None, err_rate, het_frac)
    else:
        frame = ref_simulate.simulateSNPs(g, who, num, None, err_rate)
    assert frame.shape == (num, 3)
    chrs, pos, gt = as_text(frame.iloc[:, 0]), as_text(frame.iloc[:, 1]), as_text(frame.iloc[:, 2])
    texts = set(gt.tolist())
    if name == "inbred_e0":
        assert int(err_rate * num) == 0 and texts == {"0/0", "1/1", "0/1"} and (snps[:, 0] == -1).any() and (snps[:, 0] == 2).any()
    if name in ("inbred_e05", "inbred_all"):
        assert int(err_rate * num) >= 5
    if name == "inbred_all":
        assert num == pool
    if name == "inbred_code3":
        assert "" in texts and (gt == "").sum() == (snps[:, 1] == 3).sum()
    if name == "f1_h1":
        assert "0/1" in texts
    if name == "f1_h0":
        assert "0/1" not in texts
    if name == "f1_noseg":
        assert "0/1" not in texts and not ((snps[:, 2] != snps[:, 4]) & (snps[:, 4] >= 0)).any()
    path = os.path.join(OUT, "simulate_%s.npz" % name)
    save(path, snps=snps, accessions=accessions.astype("U"), chromosomes=chromosomes.astype("U"), positions=positions, f1=np.array(f1),
         who=np.array(who), num=np.array(num, dtype=np.int64), err_rate=np.array(err_rate), het_frac=np.array(het_frac),
         seed=np.array(seed, dtype=np.int64), out_chr=chrs, out_pos=pos, out_gt=gt)
    assert os.path.getsize(path) < 20000, (name, os.path.getsize(path))
    print("%-22s %6d bytes  rows %3d of %3d  texts %s" % ("simulate_" + name, os.path.getsize(path), num, pool, sorted(texts)))


if __name__ == "__main__":
    for case in CASES:
        one(*case)
