#!/usr/bin/env python3
"""
Generate tests/golden/f1search_a*.npz by RUNNING THE UNMODIFIED REFERENCE ``CrossIdentifier.match_insilico_f1s`` (SNPmatch v5.0.1,
expected at /root/reference).  Run from the repo root:

    python tests/golden/make_golden_f1search.py

How the reference is driven (nothing of it is modified or copied; the prelude is the one of make_golden_windows.py):
  * ``allel``, ``h5py``, ``hmmlearn(.hmm)`` are only imported at the top of reference files: empty placeholder modules stand in;
  * ``match_insilico_f1s`` runs UNMODIFIED as a method of a ``CrossIdentifier`` made without its constructor: ``self.g`` is duck-typed
    on a numpy panel (``g_acc.snps``, ``accessions``, ``get_positions_idxs`` -> every row matched), ``self.inputs.wei`` comes from the
    reference's own ``ParseInputs.get_wei_from_GT`` of the GT texts;
  * the single-accession result it starts from is the reference's own ``GenotyperOutput`` with made-up scores in a shuffled order:
    with at most ten accessions the ten best are all of them, so the method returns 1, 21 and 45 crosses for 2, 7 and 10 accessions.

Panels are 2, 7 and 10 accessions wide over 240 rows, codes -1 / 0 / 1 / 2 / 3 mixed; GT texts 0/0, 1/1, 0/1, 1/0, 1/2 (not
recognised: counts as ref) and ./. (no class).  Planted (asserted below):
  * row 0: accessions 0 and 1 both 2 under a het sample -- uninformative, no hit;  row 1: both 3 -- uninformative;
  * from 7 accessions on: accession 2 without a call, and accessions 5 and 6 never called at the same row -- a pair with no
    informative row whose members are informative with others.

Per case the fixture keeps the panel, the GT texts, the reference's weights, and per returned cross its two accession indices, its
float score and its numinfo.  After the reference has spoken the numpy twin (tests/f1search_twin.py) on ``hard_classes`` of the
texts must equal every score and numinfo: ASSERTED here.

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

from snpmatch.core import csmatch as ref_csmatch  # noqa: E402
from snpmatch.core import parsers as ref_parsers  # noqa: E402
from snpmatch.core import snpmatch as ref_snpmatch  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import f1search_twin  # noqa: E402
from snpmatch_amd.core import f1search  # noqa: E402

ACCESSIONS = [2, 7, 10]
N_ROWS = 240
TEXTS = ["0/0", "1/1", "0/1", "1/0", "1/2", "./."]


def panel(n_acc):
    rng = np.random.default_rng(2100 + n_acc)
    snps = rng.choice(np.array([-1, 0, 1, 2, 3], dtype=np.int8), size=(N_ROWS, n_acc), p=[0.12, 0.4, 0.3, 0.12, 0.06])
    gt = rng.choice(np.array(TEXTS), size=N_ROWS, p=[0.3, 0.25, 0.15, 0.1, 0.1, 0.1])
    snps[0, :2], gt[0] = 2, "0/1"
    snps[1, :2], gt[1] = 3, "1/0"
    gt[2], gt[3] = "0/0", "1/2"             # (the first text names the separator; a text that is not recognised is among them)
    if n_acc >= 7:
        snps[:, 2] = -1
        snps[0::2, 5], snps[1::2, 6] = -1, -1
    return snps, gt


def save(path, **arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def one(n_acc):
    snps, gt = panel(n_acc)
    names = np.array(["A%d" % i for i in range(n_acc)])
    wei = ref_parsers.ParseInputs.get_wei_from_GT(gt)
    assert wei.shape == (N_ROWS, 3) and set(np.unique(wei).tolist()) == {0.0, 1.0}
    every = np.arange(N_ROWS)
    g = types.SimpleNamespace(g_acc=types.SimpleNamespace(snps=snps), accessions=names, get_positions_idxs=lambda chrs, pos: (every, every))
    stub = ref_csmatch.CrossIdentifier.__new__(ref_csmatch.CrossIdentifier)
    stub.g, stub.inputs = g, types.SimpleNamespace(wei=wei, chrs=None, pos=None)
    order = np.random.default_rng(n_acc).permutation(n_acc)
    single = ref_snpmatch.GenotyperOutput(names, (order + 1) * 10, np.repeat(200, n_acc), 1.0, N_ROWS, np.array([1.0]))
    out = stub.match_insilico_f1s(single, None)
    n_pairs = n_acc * (n_acc - 1) // 2
    assert len(out.accs) == n_acc + n_pairs and n_pairs == {2: 1, 7: 21, 10: 45}[n_acc]
    crosses = [str(t).split("x") for t in out.accs[n_acc:]]
    pair_a = np.array([int(a[1:]) for a, _ in crosses], dtype=np.int64)
    pair_b = np.array([int(b[1:]) for _, b in crosses], dtype=np.int64)
    score = np.asarray(out.scores[n_acc:], dtype=np.float64)
    numinfo = np.asarray(out.ninfo[n_acc:], dtype=np.int64)
    assert len(set(zip(np.minimum(pair_a, pair_b).tolist(), np.maximum(pair_a, pair_b).tolist()))) == n_pairs and (pair_a != pair_b).all()
    # the twin on the hard classes of the texts: every score, every numinfo
    classes = f1search.hard_classes(gt)
    assert np.array_equal(classes == 0, wei[:, 0] == 1) and np.array_equal(classes == 1, wei[:, 2] == 1) and np.array_equal(classes == 2, wei[:, 1] == 1)
    assert np.array_equal(classes == 0xFF, gt == "./.") and classes[3] == 0 and (classes == 0xFF).any()
    hits, ninfo = f1search_twin.f1_counts(snps, classes)
    assert np.array_equal(hits[pair_a, pair_b].astype(np.float64), score) and np.array_equal(ninfo[pair_a, pair_b].astype(np.int64), numinfo)
    direct = f1search_twin.f1_counts_direct(snps, classes)
    assert np.array_equal(direct[0], hits) and np.array_equal(direct[1], ninfo)
    # the planted rows and columns
    rest = f1search_twin.f1_counts(snps[2:], classes[2:])
    assert hits[0, 1] == rest[0][0, 1] and ninfo[0, 1] == rest[1][0, 1] and (snps[:2, :2] >= 2).all() and classes[0] == 2
    assert set(np.unique(snps).tolist()) == {-1, 0, 1, 2, 3} and set(gt.tolist()) == set(TEXTS)
    if n_acc >= 7:
        k56 = int(np.flatnonzero(((pair_a == 5) & (pair_b == 6)) | ((pair_a == 6) & (pair_b == 5)))[0])
        assert numinfo[k56] == 0 and score[k56] == 0 and ninfo[5, 0] > 0 and ninfo[6, 0] > 0
        with2 = (pair_a == 2) | (pair_b == 2)
        assert with2.sum() == n_acc - 1 and not numinfo[with2].any() and (snps[:, 2] == -1).all()
    name = "f1search_a%d" % n_acc
    path = os.path.join(HERE, name + ".npz")
    save(path, snps=snps, gt=gt.astype("U3"), wei=wei, pair_a=pair_a, pair_b=pair_b, score=score, numinfo=numinfo)
    assert os.path.getsize(path) < 20000, (name, os.path.getsize(path))
    print("%-14s %6d bytes  crosses %d  best %g of %d" % (name, os.path.getsize(path), n_pairs, score.max(), numinfo[int(np.argmax(score))]))


if __name__ == "__main__":
    for n_acc in ACCESSIONS:
        one(n_acc)
