"""
``snpmatch pairsnp`` on MI355X, and its form for a whole cohort.

``pairwiseScore`` follows the reference function of that name (core/snpmatch.py:270-309) statement by statement in what it
computes: the records two sample files share (optionally only those a DB holds), how many of them carry the same genotype TEXT,
per chromosome and in total, and how many records either file has to itself.  ``PairCohort`` does the same for every pair of a
plate or sequencing batch at once -- the reference is one process per pair.

Division of labour
  * host (this file): parsing, the record axis, the dictionary of genotype texts, result dicts and files.
  * device (``count_pairs`` -> ``engine.pair_counts`` -> ``snpm_pair_counts``): one id byte per (record, sample) compared and
    counted for every pair of samples per chromosome.  Tests of the host side replace ``count_pairs`` by a numpy twin.

The comparison is whole-string equality, as in the reference: ``0/1``, ``1/0`` and ``0|1`` are three different calls.  The call
codes of ``parsers.gt_call_code`` merge them (and every multi-allelic text) and are therefore NOT used here: ``text_ids`` numbers
the distinct texts of a job.

Differences from the reference
  * ``<outFile>.matches.json``: the reference hands ``json.dumps`` a numpy integer (``np.sum(common)``), which Python 2 printed
    as an integer and Python 3 refuses (TypeError).  Here the same call prints it as the integer it is.
  * ``PairCohort`` refuses a sample whose positions repeat or decrease within a chromosome: the reference's
    ``np.in1d(assume_unique=True)`` has no defined result there.  ``pairwiseScore`` keeps ``get_common_positions``, quirks included.
"""
import json
import logging
import os

import numpy as np

from . import parsers
from . import snp_genotype
from .snpmatch import get_fraction
from .. import engine

log = logging.getLogger(__name__)

MAX_TEXTS = engine.PAIR_MAX_ID


def count_pairs(ids, seg_off):
    """(common, match) int32 [n_seg, n_samples, n_samples] of ``engine.pair_counts``: the one step that runs on the device.  Tests
    of the host side replace this function by a numpy twin."""
    if len(seg_off) <= 1 or ids.shape[0] == 0 or ids.shape[1] == 0:
        return engine.pair_counts(None, ids, seg_off)           # nothing to count: the library answers without a device
    return engine.pair_counts(engine.default_context(), ids, seg_off)


def text_ids(gts):
    """One dictionary of the distinct genotype texts of a job: ``(ids, texts)`` with ``ids[k]`` uint8 of the shape of ``gts[k]`` and
    ``texts[ids - 1]`` the text (ids from 1 in ``np.unique`` order; 0 is kept for "no record").  More than 127 distinct texts are
    refused: an id is seven bits wide on the device."""
    arrays = [np.asarray(g).astype("U") for g in gts]
    flat = [a.ravel() for a in arrays if a.size]
    if not flat:
        return [np.zeros(a.shape, dtype=np.uint8) for a in arrays], np.zeros(0, dtype="U1")
    width = max(a.dtype.itemsize for a in flat) // 4
    texts = np.unique(np.concatenate([np.unique(a).astype("U%d" % width) for a in flat]))
    if len(texts) > MAX_TEXTS:
        raise ValueError("%d distinct genotype texts in this job, at most %d can be compared on the device (first ones: %s)"
                         % (len(texts), MAX_TEXTS, ", ".join(texts[:6].tolist())))
    return [(np.searchsorted(texts, a) + 1).astype(np.uint8).reshape(a.shape) for a in arrays], texts


def _stats(stats, common_chrs, t_common, t_scores, names, totals, n_common):
    """the result dict of ``pairwiseScore`` from its counts, with the reference's expressions (and so its number types)"""
    common = np.zeros(0, dtype=int)
    scores = np.zeros(0, dtype=int)
    for i, c, s in zip(common_chrs, t_common, t_scores):
        c, s = int(c), np.int64(s)
        stats[i] = [get_fraction(s, c), c]
        common = np.append(common, c)
        scores = np.append(scores, s)
    stats['matches'] = [get_fraction(np.sum(scores), np.sum(common)), np.sum(common)]
    stats['unique'] = {"%s" % names[0]: [get_fraction(totals[0] - n_common, totals[0]), totals[0]],
                       "%s" % names[1]: [get_fraction(totals[1] - n_common, totals[1]), totals[1]]}
    return stats


def _json_default(value):
    if isinstance(value, np.integer):
        return int(value)
    raise TypeError("Object of type %s is not JSON serializable" % type(value).__name__)


def dumps(stats):
    """the text of ``<outFile>.matches.json``"""
    return json.dumps(stats, sort_keys=True, indent=4, default=_json_default)


def pairwiseScore(inFile_1, inFile_2, logDebug, outFile=None, hdf5File=None):
    snpmatch_stats = {}
    log.info("loading input files")
    inputs_1 = parsers.ParseInputs(inFile=inFile_1, logDebug=logDebug)
    inputs_2 = parsers.ParseInputs(inFile=inFile_2, logDebug=logDebug)
    if hdf5File is not None:
        log.info("loading database file to identify common SNP positions")
        g = snp_genotype.Genotype(hdf5File, None)
        snpmatch_stats['hdf5'] = hdf5File
        commonSNPs_1 = g.get_positions_idxs(inputs_1.chrs, inputs_1.pos)
        common_inds = snp_genotype.Genotype.get_common_positions(inputs_1.chrs[commonSNPs_1[1]], inputs_1.pos[commonSNPs_1[1]],
                                                                 inputs_2.chrs, inputs_2.pos)
        common_inds = (commonSNPs_1[1][common_inds[0]], common_inds[1])
    else:
        log.info("identify common positions")
        common_inds = snp_genotype.Genotype.get_common_positions(inputs_1.chrs, inputs_1.pos, inputs_2.chrs, inputs_2.pos)
    log.info("done!")
    inputs_1.filter_chr_names()
    inputs_2.filter_chr_names()
    common_chrs = np.intersect1d(inputs_1.g_chrs_ids, inputs_2.g_chrs_ids)
    # the common rows as an id matrix [K, 2], chromosome by chromosome (a stable sort: the reference's np.where keeps file order,
    # and a count does not depend on it anyway); one device call with two samples
    rows_1, rows_2 = common_inds
    chrom = inputs_1.g_chrs[rows_1]
    code = np.searchsorted(common_chrs, chrom) if len(common_chrs) else np.zeros(len(chrom), dtype=np.int64)
    named = np.zeros(len(chrom), dtype=bool)
    if len(common_chrs):
        named = common_chrs[np.minimum(code, len(common_chrs) - 1)] == chrom
    order = np.flatnonzero(named)
    order = order[np.argsort(code[order], kind="stable")]
    (id_1, id_2), _ = text_ids([inputs_1.gt[rows_1[order]], inputs_2.gt[rows_2[order]]])
    ids = np.stack([id_1, id_2], axis=1) if len(order) else np.zeros((0, 2), dtype=np.uint8)
    seg_off = np.concatenate([[0], np.cumsum(np.bincount(code[order], minlength=len(common_chrs)))]).astype(np.int64)
    log.info("comparing %d common positions on %d chromosomes", len(order), len(common_chrs))
    common, match = count_pairs(ids, seg_off)
    _stats(snpmatch_stats, common_chrs, common[:, 0, 1], match[:, 0, 1], (os.path.basename(inFile_1), os.path.basename(inFile_2)),
           (len(inputs_1.chrs), len(inputs_2.chrs)), len(common_inds[0]))
    if outFile:
        log.info("writing output in a file: %s" % outFile + ".matches.json")
        with open(outFile + ".matches.json", "w") as out_stats:
            out_stats.write(dumps(snpmatch_stats))
        log.info("finished!")
    return snpmatch_stats


class PairCohort(object):
    """Every pair of a set of samples in one device call.  ``from_files``: one sample per file (VCF / BED / ``.npz``, through
    ``ParseInputs``); ``from_vcf``: the sample columns of one VCF.  ``stats(a, b)`` is the dict ``pairwiseScore`` returns for the
    two samples, ``write(prefix)`` the table of all pairs."""

    POS_LIMIT = 1 << 40         # (chromosome, position) of a record as one integer: chromosome * POS_LIMIT + position

    def __init__(self, names, chrs, pos, gts, hdf5File=None):
        """``names`` [S]; per sample its records: chromosome names, positions, genotype texts (file order)"""
        assert len(names) == len(chrs) == len(pos) == len(gts), "one chromosome, position and genotype array per sample"
        self.samples = [str(n) for n in names]
        self.hdf5File = hdf5File
        self.calls = np.array([len(c) for c in chrs], dtype=np.int64)
        self.chr_ids = []                       # chromosomes of the record axis, in order of first appearance
        self.sample_chr_ids = []                # per sample: the chromosomes it names anywhere
        keys = []
        for name, c, p in zip(self.samples, chrs, pos):
            ins = parsers.ParseInputs("")
            ins.load_snp_info(snpCHR=c, snpPOS=p, snpGT="", snpWEI=np.nan, DPmean=0)
            ins.filter_chr_names()
            mine = [str(x) for x in ins.g_chrs_ids.tolist()]
            self.sample_chr_ids.append(np.array(mine, dtype="U"))
            for x in mine:
                if x not in self.chr_ids:
                    self.chr_ids.append(x)
            p = np.asarray(ins.pos, dtype=np.int64)
            if len(p) and (p.min() < 0 or p.max() >= self.POS_LIMIT):
                raise ValueError("sample %s: a position below 0 or above 2^40" % name)
            code = np.array([self.chr_ids.index(x) for x in mine], dtype=np.int64)[ins.g_chr_codes] if len(p) else np.zeros(0, dtype=np.int64)
            by_chr = np.argsort(code, kind="stable")
            k = code[by_chr] * self.POS_LIMIT + p[by_chr]
            if len(k) > 1 and not np.all(k[1:] > k[:-1]):
                at = by_chr[int(np.flatnonzero(k[1:] <= k[:-1])[0]) + 1]
                raise ValueError("sample %s: the positions of chromosome %s repeat or decrease (record %d, position %d): such a "
                                 "file has no defined set of common positions" % (name, np.asarray(c)[at], at + 1, p[at]))
            keys.append(code * self.POS_LIMIT + p)
        axis = np.unique(np.concatenate(keys)) if keys else np.zeros(0, dtype=np.int64)
        if hdf5File is not None and len(axis):
            log.info("loading database file to identify common SNP positions")
            g = hdf5File if isinstance(hdf5File, snp_genotype.Genotype) else snp_genotype.Genotype(hdf5File, None)
            held = g.get_positions_idxs(np.array(self.chr_ids, dtype="U")[axis // self.POS_LIMIT], axis % self.POS_LIMIT)[1]
            axis = axis[np.sort(held)]
        self.axis_chr = axis // self.POS_LIMIT
        self.axis_pos = axis % self.POS_LIMIT
        self.seg_off = np.concatenate([[0], np.cumsum(np.bincount(self.axis_chr, minlength=len(self.chr_ids)))]).astype(np.int64)
        codes, self.texts = text_ids(gts)
        ids = np.zeros((len(axis), len(self.samples)), dtype=np.uint8)
        for s, (k, code) in enumerate(zip(keys, codes)):
            at = np.searchsorted(axis, k)
            on_axis = np.zeros(len(k), dtype=bool)
            if len(axis):
                on_axis = axis[np.minimum(at, len(axis) - 1)] == k      # (a DB drops records from the axis)
            ids[at[on_axis], s] = code[on_axis]
        self.ids = ids
        log.info("comparing %d samples at %d positions on %d chromosomes", len(self.samples), len(axis), len(self.chr_ids))
        self.common, self.match = count_pairs(ids, self.seg_off)

    @classmethod
    def from_files(cls, inFiles, hdf5File=None, logDebug=False):
        parsed = [parsers.ParseInputs(inFile=f, logDebug=logDebug) for f in inFiles]
        return cls([os.path.basename(f) for f in inFiles], [p.chrs for p in parsed], [p.pos for p in parsed], [p.gt for p in parsed], hdf5File)

    @classmethod
    def from_vcf(cls, inFile, hdf5File=None, logDebug=False):
        calls = parsers.import_vcf_file(inFile, logDebug, samples_to_load=None)
        gt = np.asarray(calls['gt'])
        present = (gt != './.') & (gt != '.|.')                 # read_vcf's own rule for a record of a sample
        cols = [np.flatnonzero(present[:, s]) for s in range(gt.shape[1])]
        return cls([str(s) for s in calls['samples']], [calls['chr'][r] for r in cols], [calls['pos'][r] for r in cols],
                   [gt[r, s] for s, r in enumerate(cols)], hdf5File)

    def n_common(self, a, b):
        return int(self.common[:, a, b].sum())

    def stats(self, a, b):
        """what ``pairwiseScore`` returns for samples ``a`` and ``b`` (indices)"""
        out = {}
        if self.hdf5File is not None:
            out['hdf5'] = self.hdf5File
        common_chrs = np.intersect1d(self.sample_chr_ids[a], self.sample_chr_ids[b])
        seg = [self.chr_ids.index(str(c)) for c in common_chrs.tolist()]
        return _stats(out, common_chrs, self.common[seg, a, b], self.match[seg, a, b], (self.samples[a], self.samples[b]),
                      (int(self.calls[a]), int(self.calls[b])), self.n_common(a, b))

    def write(self, prefix):
        """``<prefix>.pairs.tsv``: a line per pair a < b; ``<prefix>.pairs.npz``: the count matrices"""
        total_c, total_m = self.common.sum(axis=0, dtype=np.int64), self.match.sum(axis=0, dtype=np.int64)
        with open(prefix + ".pairs.tsv", "w") as out:
            out.write("sample_1\tsample_2\tmatches\tcommon\tfraction\tunique_1\tunique_2\n")
            for a in range(len(self.samples)):
                for b in range(a + 1, len(self.samples)):
                    c, m = int(total_c[a, b]), int(total_m[a, b])
                    out.write("%s\t%s\t%d\t%d\t%r\t%d\t%d\n" % (self.samples[a], self.samples[b], m, c, float(get_fraction(m, c)),
                                                               int(self.calls[a]) - c, int(self.calls[b]) - c))
        np.savez(prefix + ".pairs.npz", samples=np.array(self.samples, dtype="U"), chrs=np.array(self.chr_ids, dtype="U"),
                 common=self.common, match=self.match, calls=self.calls)


def potatoPairCohort(args):
    files = args['inFiles']
    one_vcf = len(files) == 1 and (files[0].endswith(".vcf") or files[0].endswith(".vcf.gz"))
    if one_vcf:
        cohort = PairCohort.from_vcf(files[0], args['hdf5File'], args['logDebug'])
    else:
        cohort = PairCohort.from_files(files, args['hdf5File'], args['logDebug'])
    cohort.write(args['outFile'])
    log.info("finished!")
    return cohort
