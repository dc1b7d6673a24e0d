"""shared by the genotype_cross tests: the golden cases (tests/golden/gcross_*.npz, written by make_golden_gcross.py from the
unmodified reference), a duck-typed DB, and writers for the VCF / genome files a case describes"""
import gzip
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["gcross_a_f2", "gcross_b_phasing", "gcross_c_multiallelic", "gcross_d_sparse", "gcross_e_extremes",
         "gcross_f_thres2706", "gcross_f_thres1"]
_loaded = {}


def load(name):
    """the arrays of one golden case (read once, shared, read-only)"""
    if name not in _loaded:
        with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
            case = {k: z[k] for k in z.files}
        for a in case.values():
            a.flags.writeable = False
        _loaded[name] = case
    return _loaded[name]


class _Columns(object):
    def __init__(self, snps, chromosomes, positions):
        self.snps, self.chromosomes, self.positions = snps, chromosomes, positions


class DuckGenotype(object):
    """what GenotypeCross asks of a DB that is not a ``Genotype``: ``accessions`` and ``g_acc.snps / chromosomes / positions``"""

    def __init__(self, case):
        reps = (case["chr_regions"][:, 1] - case["chr_regions"][:, 0]).astype(int)
        self.accessions = case["accessions"]
        self.g_acc = _Columns(case["panel"], np.repeat(case["chrs"], reps), case["positions"])


def write_genome(case, path):
    with open(path, "w") as fh:
        fh.write(str(case["genome_json"]))
    return path


def write_vcf(path, chrom, pos, gt, samples, fmt="GT:DP"):
    """a multi-sample VCF holding exactly these records (``path`` ending in .gz: gzip)"""
    opener = gzip.open if path.endswith(".gz") else open
    keys = fmt.split(":")
    entry = lambda g: ":".join(str(g) if k == "GT" else "7" for k in keys)       # noqa: E731
    with opener(path, "wt") as fh:
        fh.write("##fileformat=VCFv4.2\n")
        fh.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(str(s) for s in samples) + "\n")
        for c, p, row in zip(chrom, pos, gt):
            fh.write("%s\t%d\t.\tA\tT\t50\tPASS\tDP=21\t%s\t%s\n" % (c, p, fmt, "\t".join(entry(g) for g in row)))
    return path
