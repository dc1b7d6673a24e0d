#!/usr/bin/env python3
"""
Generate tests/golden/gcross_*.npz by RUNNING THE UNMODIFIED REFERENCE ``GenotypeCross(...).genotype_cross(...)`` (SNPmatch
v5.0.1, expected at /root/reference) in the build container.  Run from the repo root:

    python tests/golden/make_golden_gcross.py

How the reference is driven (nothing of it is modified or copied; the prelude is the one of make_golden.py):
  * ``allel``, ``h5py``, ``hmmlearn(.hmm)`` are absent here and only imported at the top of reference files: empty placeholder
    modules stand in for them;
  * ``parsers.import_vcf_file`` (scikit-allel in the reference) is replaced by a function that returns the prepared dict
    (``samples``, ``gt``, ``chr``, ``pos``);
  * ``g`` is duck-typed: ``accessions`` and ``g_acc.snps`` / ``chromosomes`` / ``positions`` are all the path reads;
  * ``genotype_cross.genome`` is a reference ``Genome`` built from a toy JSON file (3 chromosomes of 1 000 000, 650 000 and
    300 000 bp: 20 windows of 100 kb).

Every fixture holds the inputs (panel, positions, chromosome regions, accession names, parents, the VCF's chr / pos / GT text and
sample names, binLen, lr_thres, the genome JSON text) and the reference's output lines.

After the reference has spoken, this package's host layer is run on the same inputs with the numpy twin (tests/gcross_twin.py) in
the place of the device call.  That run must reproduce the lines, and it yields the twin's ``lr_next`` of every cell: the generator
ASSERTS that no cell of any fixture has a computed ``lr_next`` within 1e-9 (relative) of ``lr_thres`` -- device and numpy
logarithms may differ in the last bits, and such a knife-edge cell would not be a fair check.  (A cell whose ``lr_next`` is the
threshold itself by substitution -- no other finite ratio exists -- involves no logarithm and is not a knife edge.)
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

from snpmatch.core import genomes as ref_genomes  # noqa: E402
from snpmatch.core import genotype_cross as ref_gc  # noqa: E402
from snpmatch.core import parsers as ref_parsers  # noqa: E402

CHR_LEN = [1000000, 650000, 300000]
BIN = 100000
GENOME_PLAIN = {"ref_chrs": ["Chr1", "Chr2", "Chr3"], "ref_chrlen": CHR_LEN}
GENOME_RATES = {"ref_chrs": ["Chr1", "Chr2", "Chr3"], "ref_chrlen": CHR_LEN, "recomb_rates": [3.4, 3.6, 4.25]}
ACCESSIONS = np.array(["6091", "6191", "7000", "8000", "9100", "9332"], dtype="U")
PARENTS = "6191x9100"
CALL_TEXT = {0: "0/0", 1: "1/1", 2: "0/1", -1: "./."}


class Columns(object):
    def __init__(self, snps, chromosomes, positions):
        self.snps, self.chromosomes, self.positions = snps, chromosomes, positions


class DuckGenotype(object):
    def __init__(self, snps, chrs, regions, positions):
        chromosomes = np.repeat(np.array(chrs, dtype="U"), [b - a for a, b in regions])
        self.accessions = ACCESSIONS
        self.g_acc = Columns(snps, chromosomes, positions)


def make_panel(rng, per_chr=(620, 400, 180)):
    positions, regions, row = [], [], 0
    for n, length in zip(per_chr, CHR_LEN):
        positions.append(np.sort(rng.choice(np.arange(1, length + 1), size=n, replace=False)))
        regions.append((row, row + n))
        row += n
    positions = np.concatenate(positions).astype("i4")
    snps = rng.choice(np.array([-1, 0, 1, 2], dtype=np.int8), size=(row, len(ACCESSIONS)), p=[0.05, 0.5, 0.4, 0.05])
    return snps, ["1", "2", "3"], regions, positions


def f2_sample(rng, chrom, par1, par2, err=0.03, nocall=0.10):
    """GT text of one F2-like individual at records whose parental calls are par1 / par2 (-1 where the record is no marker):
    blocks copied from parent 1, parent 2 or heterozygous, then errors and no-calls"""
    n = len(chrom)
    state = np.zeros(n, dtype=np.int8)
    for c in np.unique(chrom):
        where = np.flatnonzero(chrom == c)
        cuts = np.sort(rng.choice(len(where), size=min(len(where), int(rng.integers(0, 4))), replace=False))
        for block in np.split(where, cuts):
            state[block] = rng.choice([0, 1, 2], p=[0.25, 0.5, 0.25])
    call = np.where(state == 0, par1, np.where(state == 2, par2, 2))
    call = np.where((par1 < 0) | (par2 < 0), rng.choice([0, 1, 2], size=n), call)
    wrong = rng.random(n) < err
    call = np.where(wrong, rng.choice([0, 1, 2], size=n), call)
    call = np.where(rng.random(n) < nocall, -1, call)
    return np.array([CALL_TEXT[int(v)] for v in call], dtype="U3")


def records(rng, panel, keep=0.8, extra=150, drop_chr=()):
    """VCF records: a share of the panel's positions plus positions the panel does not hold; chromosome names as 'Chr<n>'"""
    snps, chrs, regions, positions = panel
    chrom, pos, row = [], [], []
    for name, (a, b), length in zip(chrs, regions, CHR_LEN):
        if name in drop_chr:
            continue
        mine = np.flatnonzero(rng.random(b - a) < keep) + a
        other = np.setdiff1d(rng.choice(np.arange(1, length + 1), size=extra // 3, replace=False), positions[a:b])
        p = np.concatenate([positions[mine], other])
        r = np.concatenate([mine, np.full(len(other), -1)])
        order = np.argsort(p, kind="stable")
        chrom.append(np.repeat("Chr" + name, len(p)))
        pos.append(p[order])
        row.append(r[order])
    return np.concatenate(chrom).astype("U"), np.concatenate(pos).astype(int), np.concatenate(row)


def parental_calls(panel, rows):
    snps = panel[0]
    i1, i2 = [int(np.flatnonzero(ACCESSIONS == a)[0]) for a in PARENTS.split("x")]
    one = np.where(rows >= 0, snps[np.maximum(rows, 0), i1], -1)
    two = np.where(rows >= 0, snps[np.maximum(rows, 0), i2], -1)
    marker = (one != two) & (one >= 0) & (two >= 0)
    return np.where(marker, one, -1), np.where(marker, two, -1)


def run_reference(panel, vcf, samples, gt, genome_json, lr_thres):
    snps, chrs, regions, positions = panel
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "toy_genome.json")
        with open(path, "w") as fh:
            json.dump(genome_json, fh)
        ref_gc.genome = ref_genomes.Genome(path)
    prepared = {"samples": np.array(samples, dtype="U"), "gt": gt, "chr": vcf[0], "pos": vcf[1]}
    ref_parsers.import_vcf_file = lambda **kw: prepared
    cross = ref_gc.GenotypeCross(DuckGenotype(snps, chrs, regions, positions), PARENTS, BIN, None, False)
    return np.array(cross.genotype_cross("prepared.vcf", lr_thres), dtype="U")


def check_with_twin(name, panel, vcf, samples, gt, genome_json, lr_thres, lines):
    """this package's host layer + the numpy twin reproduce the lines, and no cell sits on the threshold"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gcross_twin
    from snpmatch_amd.core import genomes, genotype_cross, parsers
    snps, chrs, regions, positions = panel
    seen = {}

    def twin(codes, p1, p2, win_off, thres):
        geno, cnt, lr_next = gcross_twin.cross_calls(codes, p1, p2, win_off, thres)
        seen["edge"] = gcross_twin.knife_edge_cells(lr_next, thres)
        seen["geno"], seen["counts"], seen["win_off"] = geno, cnt, np.asarray(win_off)
        return geno

    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "toy_genome.json")
        with open(path, "w") as fh:
            json.dump(genome_json, fh)
        genotype_cross.genome = genomes.Genome(path)
    keep_reader, keep_step = parsers.import_vcf_calls, genotype_cross.count_and_decide
    parsers.import_vcf_calls = lambda *a, **kw: {"samples": np.array(samples, dtype="U"), "chr": vcf[0], "pos": vcf[1],
                                                 "codes": parsers.gt_call_codes(gt)}
    genotype_cross.count_and_decide = twin
    try:
        cross = genotype_cross.GenotypeCross(DuckGenotype(snps, chrs, regions, positions), PARENTS, BIN, None, False)
        mine = cross.genotype_cross("prepared.vcf", lr_thres)
    finally:
        parsers.import_vcf_calls, genotype_cross.count_and_decide = keep_reader, keep_step
    assert list(mine) == list(lines), "%s: host layer + twin differ from the reference" % name
    assert seen["edge"] == 0, "%s: %d cell(s) with lr_next within 1e-9 of lr_thres: change the seed" % (name, seen["edge"])
    return seen


def write(name, panel, vcf, samples, gt, genome_json, lr_thres):
    lines = run_reference(panel, vcf, samples, gt, genome_json, lr_thres)
    seen = check_with_twin(name, panel, vcf, samples, gt, genome_json, lr_thres, lines)
    snps, chrs, regions, positions = panel
    out = os.path.join(HERE, name + ".npz")
    np.savez_compressed(out, panel=snps, positions=positions, chrs=np.array(chrs, dtype="U"), chr_regions=np.array(regions, dtype=np.int64),
                        accessions=ACCESSIONS, parents=np.array(PARENTS), vcf_chr=vcf[0], vcf_pos=vcf[1], vcf_gt=gt,
                        samples=np.array(samples, dtype="U"), binLen=np.array(BIN), lr_thres=np.array(float(lr_thres)),
                        genome_json=np.array(json.dumps(genome_json)), lines=lines,
                        geno=seen["geno"], counts=seen["counts"], win_off=seen["win_off"])
    calls = np.array([ln.split(",")[3:] for ln in lines[2:]])
    print("%-24s %6d bytes  %3d samples %5d records  calls: %s" % (
        name, os.path.getsize(out), len(samples), len(vcf[1]), dict(zip(*np.unique(calls, return_counts=True)))))


def main():
    rng = np.random.default_rng(20261017)
    panel = make_panel(rng)

    # a. 37 random F2-like individuals
    vcf = records(rng, panel)
    one, two = parental_calls(panel, vcf[2])
    gt = np.stack([f2_sample(rng, vcf[0], one, two) for _ in range(37)], axis=1)
    write("gcross_a_f2", panel, vcf, ["F2_%02d" % i for i in range(37)], gt, GENOME_PLAIN, 1.5)

    # b. phasing: one fully phased individual, one with 30 % of its calls written with the other separator (both directions),
    #    and an unphased one for contrast
    vcf = records(rng, panel)
    one, two = parental_calls(panel, vcf[2])
    cols = [f2_sample(rng, vcf[0], one, two) for _ in range(4)]
    cols[0] = np.char.replace(cols[0], "/", "|")
    flip = rng.random(len(cols[1])) < 0.3
    cols[1] = np.where(flip, np.char.replace(cols[1], "/", "|"), cols[1])
    flip = rng.random(len(cols[2])) < 0.3
    cols[2] = np.where(flip, cols[2], np.char.replace(cols[2], "/", "|"))
    write("gcross_b_phasing", panel, vcf, ["phased", "mixed_30_bar", "mixed_30_slash", "plain"], np.stack(cols, axis=1), GENOME_RATES, 1.5)

    # c. multi-allelic calls: 1/2, 0/2, 2/2 and a phased 1|2 sprinkled over 15 % of the calls
    vcf = records(rng, panel)
    one, two = parental_calls(panel, vcf[2])
    cols = []
    for _ in range(5):
        col = f2_sample(rng, vcf[0], one, two).astype("U3")
        odd = rng.random(len(col)) < 0.15
        col = np.where(odd, rng.choice(np.array(["1/2", "0/2", "2/2", "1|2"]), size=len(col)), col)
        cols.append(col)
    write("gcross_c_multiallelic", panel, vcf, ["M%d" % i for i in range(5)], np.stack(cols, axis=1), GENOME_PLAIN, 1.5)

    # d. sparse windows: the first four windows of chromosome 1 hold 0, 1, 4 and 5 matched markers, chromosome 3 is absent
    chrom, pos, rows = records(rng, panel, keep=0.9, drop_chr=("3",))
    one, two = parental_calls(panel, rows)
    marker = one >= 0
    drop = np.zeros(len(pos), dtype=bool)
    for window, wanted in enumerate((0, 1, 4, 5)):
        inside = np.flatnonzero((chrom == "Chr1") & (pos >= 1 + window * BIN) & (pos <= (window + 1) * BIN) & marker)
        assert len(inside) >= wanted
        drop[rng.permutation(inside)[wanted:]] = True
    vcf = (chrom[~drop], pos[~drop], rows[~drop])
    one, two = one[~drop], two[~drop]
    gt = np.stack([f2_sample(rng, vcf[0], one, two, err=0.0, nocall=0.0) for _ in range(6)], axis=1)
    write("gcross_d_sparse", panel, vcf, ["S%d" % i for i in range(6)], gt, GENOME_RATES, 1.5)

    # e. extremes: an individual identical to parent 1 (every likelihood of a window is 1 or NaN), one identical to parent 2, one
    #    heterozygous everywhere, one never called, and an F2 for contrast
    vcf = records(rng, panel)
    one, two = parental_calls(panel, vcf[2])
    filler = rng.choice([0, 1, 2], size=len(one))
    as_text = lambda calls: np.array([CALL_TEXT[int(v)] for v in calls], dtype="U3")      # noqa: E731
    cols = [as_text(np.where(one >= 0, one, filler)), as_text(np.where(two >= 0, two, filler)), np.repeat("0/1", len(one)),
            np.repeat("./.", len(one)), f2_sample(rng, vcf[0], one, two)]
    write("gcross_e_extremes", panel, vcf, ["is_p1", "is_p2", "all_het", "no_calls", "f2"], np.stack(cols, axis=1), GENOME_PLAIN, 1.5)

    # f. other thresholds on noisy individuals (15 % errors: ratios on both sides of 1.0, 1.5 and 2.706)
    vcf = records(rng, panel, keep=0.35)
    one, two = parental_calls(panel, vcf[2])
    gt = np.stack([f2_sample(rng, vcf[0], one, two, err=0.45, nocall=0.2) for _ in range(12)], axis=1)
    samples = ["N%02d" % i for i in range(12)]
    write("gcross_f_thres2706", panel, vcf, samples, gt, GENOME_RATES, 2.706)
    write("gcross_f_thres1", panel, vcf, samples, gt, GENOME_PLAIN, 1.0)


if __name__ == "__main__":
    main()
