#!/usr/bin/env python3
"""
Generate tests/golden/pairsnp_*.npz by RUNNING THE UNMODIFIED REFERENCE ``snpmatch.pairwiseScore`` (SNPmatch v5.0.1, expected at
/root/reference) in the build container, for every ordered pair of a small cohort.  Run from the repo root:

    python tests/golden/make_golden_pairsnp.py

How the reference is driven (nothing of it is modified or copied; the prelude is the one of make_golden_gcross.py):
  * ``allel``, ``h5py``, ``hmmlearn(.hmm)`` are absent here and only imported at the top of reference files: empty placeholder
    modules stand in for them;
  * the samples reach it as ``.npz`` parser dumps and as ``.bed`` files, both of which its ``ParseInputs`` reads without
    scikit-allel.  A ``.bed`` is parsed by the reference once before the pairs run: that first parse writes its dump
    (``<file>.snpmatch.npz``) and then fails in its statistics step (``np.nanmean("NA")``, the crash core/parsers.py of this package
    describes); every later ``ParseInputs`` of the file loads the dump, which is how the reference is used on BED files at all;
  * for the ``-d`` case a duck-typed stand-in sits at ``snpmatch.snp_genotype.Genotype``: it serves ``get_positions_idxs`` from
    arrays through the reference's own static ``get_common_positions``, which it keeps.

THE JSON TEXT.  The reference ends with ``json.dumps(stats, sort_keys=True, indent=4)``, and ``stats['matches'][1]`` is a numpy
integer: Python 2 printed it as an integer, Python 3 raises TypeError (checked below: the unmodified call must still fail that way,
or this note is out of date).  The text kept in a fixture is therefore that same call on the reference's own dict with a ``default``
that prints a numpy integer as the integer it is -- nothing else about the dict or the call changes.

After the reference has spoken, this package's ``pairwiseScore`` and ``PairCohort`` run on the same files with the numpy twin
(tests/pairsnp_twin.py) in the place of the device call, and the generator ASSERTS that both reproduce every text.  The cohort's
count matrices of that run are kept in the fixture too (``cohort_common`` / ``cohort_match``).
"""
import json
import os
import sys
import tempfile
import types
import warnings

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

from snpmatch.core import parsers as ref_parsers  # noqa: E402
from snpmatch.core import snp_genotype as ref_snp_genotype  # noqa: E402
from snpmatch.core import snpmatch as ref_snpmatch  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import pairsnp_util  # noqa: E402

REF_GENOTYPE = ref_snp_genotype.Genotype
CURRENT_DB = {}


class DuckDB(object):
    """what pairwiseScore asks of a DB: positions per chromosome"""
    get_common_positions = staticmethod(REF_GENOTYPE.get_common_positions)

    def __init__(self, hdf5_file, hdf5_acc_file):
        self.chromosomes = np.repeat(CURRENT_DB["chrs"], [b - a for a, b in CURRENT_DB["regions"]])
        self.positions = CURRENT_DB["positions"]

    def get_positions_idxs(self, chrs, pos):
        return self.get_common_positions(self.chromosomes, self.positions, chrs, pos)


def numpy_int_default(value):
    if isinstance(value, np.integer):
        return int(value)
    raise TypeError(type(value))


def universe(rng, chroms, per_chr=140, length=200000):
    return {c: np.sort(rng.choice(np.arange(1, length), size=per_chr, replace=False)) for c in chroms}


def sample(rng, uni, truth, name_of, keep=0.8, alphabet=("0/0", "1/1", "0/1"), err=0.08, chroms=None):
    """records of one sample: a share of the universe's positions, the shared 'truth' text with some calls redrawn"""
    chrs, pos, gt = [], [], []
    for c in (chroms or list(uni)):
        take = np.flatnonzero(rng.random(len(uni[c])) < keep)
        text = truth[c][take].copy()
        redo = rng.random(len(take)) < err
        text[redo] = rng.choice(np.array(alphabet), size=int(redo.sum()))
        chrs.append(np.repeat(name_of(c), len(take)))
        pos.append(uni[c][take])
        gt.append(text)
    return np.concatenate(chrs).astype("U"), np.concatenate(pos).astype(int), np.concatenate(gt).astype("U")


def truth_of(rng, uni, alphabet, p=None):
    return {c: rng.choice(np.array(alphabet), size=len(uni[c]), p=p) for c in uni}


def run_reference(case, directory):
    names = pairsnp_util.write_inputs(case, directory)
    db = pairsnp_util.DB_NAME if "db_positions" in case else None
    if db:
        CURRENT_DB.update(chrs=case["db_chrs"], regions=case["db_regions"].tolist(), positions=case["db_positions"])
        ref_snp_genotype.Genotype = DuckDB
    here = os.getcwd()
    os.chdir(directory)
    try:
        for name in names:
            if name.endswith(".bed"):
                try:
                    ref_parsers.ParseInputs(name, False)
                    raise SystemExit("the reference parsed a BED file to the end: the note in this file's docstring is out of date")
                except TypeError:
                    assert os.path.isfile(name + ".snpmatch.npz")
        pairs, texts = [], []
        for a in range(len(names)):
            for b in range(len(names)):
                if a == b:
                    continue
                stats = ref_snpmatch.pairwiseScore(names[a], names[b], False, None, db)
                try:
                    json.dumps(stats, sort_keys=True, indent=4)
                    raise SystemExit("json.dumps took the reference's dict as it is: the note in this file's docstring is out of date")
                except TypeError:
                    pass
                pairs.append((a, b))
                texts.append(json.dumps(stats, sort_keys=True, indent=4, default=numpy_int_default))
    finally:
        os.chdir(here)
        ref_snp_genotype.Genotype = REF_GENOTYPE
    return np.array(pairs, dtype=np.int64), np.array(texts, dtype="U")


def check_with_twin(name, case, pairs, texts):
    sys.path.insert(0, ROOT)
    import pairsnp_twin
    from snpmatch_amd.core import pairsnp
    keep = pairsnp.count_pairs
    pairsnp.count_pairs = pairsnp_twin.pair_counts
    here = os.getcwd()
    try:
        with tempfile.TemporaryDirectory() as tmp:
            names = pairsnp_util.write_inputs(case, tmp)
            db = pairsnp_util.write_db(case, tmp)
            os.chdir(tmp)
            cohort = pairsnp.PairCohort.from_files(names, db, False)
            for (a, b), text in zip(pairs.tolist(), texts.tolist()):
                mine = pairsnp.pairwiseScore(names[a], names[b], False, "out", db)
                assert pairsnp.dumps(mine) == text, "%s: pairwiseScore + twin differ from the reference for pair %d, %d" % (name, a, b)
                assert open("out.matches.json").read() == text
                assert pairsnp.dumps(cohort.stats(a, b)) == text, "%s: PairCohort + twin differ from the reference for pair %d, %d" % (name, a, b)
            for p in parsed_threads():
                p.join()
    finally:
        os.chdir(here)
        pairsnp.count_pairs = keep
    return cohort


def parsed_threads():
    import threading
    return [t for t in threading.enumerate() if t.name == "snpmatch-parse-cache"]


def write(name, names, samples, db=None):
    case = {"names": np.array(names, dtype="U")}
    for k, (c, p, g) in enumerate(samples):
        case["chr_%d" % k], case["pos_%d" % k], case["gt_%d" % k] = c, p, g
    if db is not None:
        case["db_chrs"], case["db_regions"], case["db_positions"] = db
    with tempfile.TemporaryDirectory() as tmp:
        pairs, texts = run_reference(case, tmp)
    cohort = check_with_twin(name, case, pairs, texts)
    out = os.path.join(HERE, name + ".npz")
    # (the cohort's count matrices, as the twin gave them: every ordered pair of them reproduced a reference dict above)
    np.savez_compressed(out, pairs=pairs, json=texts, cohort_common=cohort.common, cohort_match=cohort.match, **case)
    assert os.path.getsize(out) < 100000
    fr = [json.loads(t)["matches"] for t in texts.tolist()]
    print("%-24s %6d bytes  %d samples  %2d pairs  matches: %s" % (name, os.path.getsize(out), len(names), len(pairs),
                                                                  " ".join("%.3f/%d" % (f, c) for f, c in fr[:4])))


def main():
    rng = np.random.default_rng(20261018)
    plain = lambda c: "Chr" + c      # noqa: E731

    # a. plain diploid texts, five chromosomes
    uni = universe(rng, ["1", "2", "3", "4", "5"])
    truth = truth_of(rng, uni, ("0/0", "1/1", "0/1"), p=[0.5, 0.4, 0.1])
    samples = [sample(rng, uni, truth, plain) for _ in range(4)]
    samples.append(samples[1])                                  # a duplicated sample: every common call matches
    write("pairsnp_a_plain", ["s%d.npz" % i for i in range(5)], samples)

    # b. '/' and '|' mixed; 0/1 against 1/0 and 0|1: three different texts
    uni = universe(rng, ["1", "2", "3"])
    alphabet = ("0/0", "1/1", "0/1", "1/0", "0|1", "1|0", "0|0", "1|1")
    truth = truth_of(rng, uni, alphabet)
    samples = [sample(rng, uni, truth, plain, alphabet=alphabet, err=0.3) for _ in range(4)]
    write("pairsnp_b_phasing", ["p%d.npz" % i for i in range(4)], samples)

    # c. multi-allelic texts, texts of different lengths
    alphabet = ("0/0", "1/1", "0/1", "1/2", "0/2", "2/2", "1|2", "10/11", "0/10", "1", "0", "./.")
    truth = truth_of(rng, uni, alphabet)
    samples = [sample(rng, uni, truth, plain, alphabet=alphabet, err=0.25) for _ in range(4)]
    write("pairsnp_c_multiallelic", ["m%d.npz" % i for i in range(4)], samples)

    # d. 'Chr1' / 'chr1' / '1' / 'CHR1' naming; chromosome 4 only in one sample
    uni = universe(rng, ["1", "2", "3", "4"])
    truth = truth_of(rng, uni, ("0/0", "1/1", "0/1"))
    namers = [plain, lambda c: "chr" + c, lambda c: c, lambda c: "CHR" + c]
    samples = [sample(rng, uni, truth, namers[k], chroms=["1", "2", "3", "4"] if k == 2 else ["1", "2", "3"]) for k in range(4)]
    write("pairsnp_d_naming", ["n%d.npz" % i for i in range(4)], samples)

    # e. a chromosome two samples name without sharing a position on it (the NaN line); a sample with nothing in common with anyone
    uni = universe(rng, ["1", "2", "3"])
    truth = truth_of(rng, uni, ("0/0", "1/1", "0/1"))
    s0 = sample(rng, uni, truth, plain)
    s1 = sample(rng, uni, truth, plain)
    on2 = s1[0] == "Chr2"
    moved = s1[1].copy()
    moved[on2] = np.sort(rng.choice(np.arange(300000, 400000), size=int(on2.sum()), replace=False))     # chromosome 2 elsewhere
    s1 = (s1[0], moved, s1[2])
    s2 = sample(rng, uni, truth, lambda c: "scaffold_" + c, chroms=["1"])
    s3 = sample(rng, uni, truth, plain, chroms=["3", "1"])      # chromosomes in another order
    write("pairsnp_e_disjoint", ["e%d.npz" % i for i in range(4)], [s0, s1, s2, s3])

    # f. a DB that lacks some positions (and a whole chromosome)
    uni = universe(rng, ["1", "2", "3"])
    truth = truth_of(rng, uni, ("0/0", "1/1", "0/1"))
    samples = [sample(rng, uni, truth, plain) for _ in range(4)]
    held = {c: uni[c][rng.random(len(uni[c])) < 0.7] for c in ("1", "2")}
    regions, row = [], 0
    for c in ("1", "2"):
        regions.append((row, row + len(held[c])))
        row += len(held[c])
    db = (np.array(["1", "2"], dtype="U"), np.array(regions, dtype=np.int64), np.concatenate([held["1"], held["2"]]).astype("i4"))
    write("pairsnp_f_db", ["d%d.npz" % i for i in range(4)], samples, db)

    # g. BED inputs; './.' lines are calls of a BED like any other
    truth = truth_of(rng, uni, ("0/0", "1/1", "0/1", "./."), p=[0.45, 0.35, 0.1, 0.1])
    samples = [sample(rng, uni, truth, plain, alphabet=("0/0", "1/1", "0/1", "./.")) for _ in range(3)]
    write("pairsnp_g_bed", ["b%d.bed" % i for i in range(3)], samples)


if __name__ == "__main__":
    main()
