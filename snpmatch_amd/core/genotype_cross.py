"""
``snpmatch genotype_cross`` on MI355X: per genome window and F2 individual, is the window parent 1 (``0``), heterozygous
(``1``), parent 2 (``2``) or undecided (``NA``)?  Output: an R/qtl CSV.

Public surface follows the reference module ``snpmatch.core.genotype_cross`` (core/genotype_cross.py:21-49, :52-111, :184-249):
``getWindowGenotype``, ``GenotypeCross`` (``get_segregating_snps_parents``, ``genotype_cross``, ``genotype_cross_hmm``, the static
``get_window_genotype_gts`` and ``write_output_genotype_cross``; attributes ``commonSNPsCHR``, ``commonSNPsPOS``, ``snpsP1``,
``snpsP2``, ``p1_ix``, ``p2_ix``, ``window_size``) and ``potatoCrossGenotyper``.

The reference loops over windows x samples, parsing genotype strings and calling ``likeliTest`` three times per cell.  Here the
multi-sample VCF is read once into one call code per (record, sample) (``parsers.import_vcf_calls``), its positions are
intersected with the panel, the two parents are read at the matched rows, the rows where the parents segregate are kept, and
ONE device call (``engine.cross_calls`` -> ``k_gcross``) counts and decides every (window, sample).  Only matched markers count in
the reference, so intersecting first and filtering by "segregating" afterwards selects the same markers.

``genotype_cross_hmm`` (core/genotype_cross.py:113-181 of the reference) labels every matched segregating marker of every F2
individual AA / AB / BB (0 / 1 / 2) by a 3-state Viterbi per (sample, chromosome).  One chain is serial; a job is samples x
chromosomes chains that walk the same markers, so they run side by side: the host builds the tables of logarithms with numpy
(``core.infer``), ONE device call (``engine.cross_hmm`` -> ``k_ghmm``, one lane per chain) returns every path.  It differs from
the reference in three places: a genome chromosome without matched markers contributes no lines (the reference divides by
zero), chromosome names are compared as bare ids (the reference compares ``genome.chrs`` with ``chrs_ids`` and finds nothing
when the JSON says ``Chr1``), and a chromosome whose recombination fraction per marker exceeds 1 (a handful of markers on a very
long chromosome: the transition matrix turns negative) is refused instead of carried through as NaN.

Refused, with a message:
  * ``--hmm`` of the ``genotype_cross`` subcommand: the HMM genotyper is the subcommand ``genotype_cross_hmm``;
  * ``-q / --father`` (parents from two VCF files): that branch of the reference indexes per-chromosome subsets into whole-file
    arrays (:73-82) and is only self-consistent for one chromosome with identical position sets;
  * genotypes without a separator (haploid calls): the reference's "unable to parse the format of GT in vcf!";
  * positions of one VCF chromosome that are not strictly increasing (duplicates make the reference fail its own assertion);
  * a parent with a panel value above 2 at a matched segregating marker (no sample call can equal it).
"""
import logging

import numpy as np

from . import genomes
from . import infer
from . import parsers
from . import snp_genotype
from .. import engine

log = logging.getLogger(__name__)

HMM_REFUSED = ("--hmm is not provided by this package as a flag of genotype_cross: "
               "the HMM genotyper is its own subcommand, genotype_cross_hmm (same -i / -d / -e / -p / --genome / -o)")
FATHER_REFUSED = ("-q / --father (parents from two VCF files) is not provided by this package: "
                  "name the parents as two accessions of the database, -p 6091x6191")
genome = None                        # set by potatoCrossGenotyper, as in the reference (a module global there too)


def die(msg):
    parsers.die(msg)


def _likeli(n, y):
    """likeliTest (core/snpmatch.py:40-55) for one (informative n, matched y)"""
    assert y <= n, "provided y is greater than n"
    p = 0.99999999
    if n == 0 or y == 0:
        return np.nan
    if y == n:
        return 1.0
    ps = float(y) / n
    return y * np.log(ps / p) + (n - y) * np.log((1 - ps) / (1 - p))


def getWindowGenotype(matchedNos, totalMarkers, lr_thres, n_marker_thres=5):
    """(call, ratios) of ONE window from its three matched counts (parent 1, heterozygous, parent 2): the scalar form of what
    ``k_gcross`` decides per (window, sample) on the device -- 'NA' below ``n_marker_thres`` markers or without any match, 1 when
    two classes tie, 0 / 2 when that parent is the most likely and the next ratio reaches ``lr_thres``, 1 when heterozygous is.
    ``ratios``: the three likelihood ratios as '%.2f' joined by commas ('NA' for an undecidable window)."""
    if totalMarkers < n_marker_thres:
        return ('NA', 'NA')
    assert len(matchedNos) == 3
    if not any(int(m) for m in matchedNos):
        return ('NA', 'NA')
    likes = np.array([_likeli(totalMarkers, m) for m in matchedNos], dtype=float)
    top = np.nanmin(likes)
    ratios = likes / top if top > 0 else np.repeat(np.nan, 3)
    pval = ",".join("%.2f" % r for r in ratios)
    if np.count_nonzero(ratios == 1) > 1:
        return (1, pval)
    high = int(np.nanargmin(likes))
    rest = ratios[np.nonzero(ratios - 1)]
    rest = rest[~np.isnan(rest)]
    lr_next = rest.min() if len(rest) else lr_thres
    geno = 'NA'
    if high == 0 and lr_next >= lr_thres:
        geno = 0
    elif high == 2 and lr_next >= lr_thres:
        geno = 2
    if high == 1:
        geno = 1
    return (geno, pval)


def count_and_decide(codes, p1, p2, win_off, lr_thres):
    """int8 [n_win, n_samples] calls (-1 = NA) of every (window, sample): the one step that runs on the device.  Tests of the
    host side replace this function by a numpy twin."""
    return engine.cross_calls(engine.default_context(), codes, p1, p2, win_off, lr_thres)


def viterbi_paths(codes, depth_rank, pair, chain_off, logT, logI, logE):
    """int8 [n, n_samples] states (0 AA, 1 AB, 2 BB) of every (chain, sample): the one step of ``genotype_cross_hmm`` that runs on
    the device.  Tests of the host side replace this function by a numpy twin."""
    return engine.cross_hmm(engine.default_context(), codes, depth_rank, pair, chain_off, logT, logI, logE)


class GenotypeCross(object):

    def __init__(self, g, parents, binLen=0, father=None, logDebug=True):
        self.logDebug = logDebug
        self.g = g
        self.get_segregating_snps_parents(parents, father)
        self.window_size = int(binLen)

    def get_segregating_snps_parents(self, parents, father):
        """``p1_ix`` / ``p2_ix``: the parents' columns in the panel.  The whole-panel views of the reference (``snpsP1``,
        ``snpsP2``, ``commonSNPsCHR``, ``commonSNPsPOS``: the rows where the parents differ and both are called) are derived on
        first use -- ``genotype_cross`` itself reads the parents only at the rows the VCF matches."""
        if father is not None:
            die(FATHER_REFUSED)
        assert len(parents.split("x")) == 2, "parents should be provided as '6091x6191'"
        try:
            accessions = np.asarray(self.g.accessions)
            self.p1_ix = int(np.where(accessions == parents.split("x")[0])[0][0])
            self.p2_ix = int(np.where(accessions == parents.split("x")[1])[0][0])
        except IndexError:
            die("parents are not in the dataset")
        self._segregating = None

    def _whole_panel(self):
        if self._segregating is None:
            log.info("loading genotype data for parents, and identify segregating SNPs")
            one = np.asarray(self.g.g_acc.snps[:, self.p1_ix])
            two = np.asarray(self.g.g_acc.snps[:, self.p2_ix])
            keep = np.where((one != two) & (one >= 0) & (two >= 0))[0]
            log.info("number of segregating snps between parents: %s", len(keep))
            self._segregating = (np.array(self.g.g_acc.chromosomes)[keep].astype('U'), np.array(self.g.g_acc.positions)[keep],
                                 one[keep], two[keep])
        return self._segregating

    commonSNPsCHR = property(lambda self: self._whole_panel()[0])
    commonSNPsPOS = property(lambda self: self._whole_panel()[1])
    snpsP1 = property(lambda self: self._whole_panel()[2])
    snpsP2 = property(lambda self: self._whole_panel()[3])

    def _panel_chromosomes(self, db_rows):
        """the panel's chromosome name of every row in ``db_rows``"""
        inner = getattr(self.g, "g", None)
        if inner is not None and hasattr(inner, "chr_regions") and hasattr(inner, "chrs"):
            ends = np.asarray(inner.chr_regions)[:, 1]
            return np.asarray(inner.chrs).astype('U')[np.searchsorted(ends, db_rows, side="right")]
        return np.asarray(self.g.g_acc.chromosomes)[db_rows].astype('U')

    def genotype_cross_hmm(self, input_file, min_na_per_sample=0.8):
        """lines of the R/qtl CSV: two header lines, then one line per matched segregating marker, ``chr:pos,chr,cM,<state per
        kept sample>`` (0 AA, 1 AB, 2 BB).  Samples whose share of markers with DP <= 0 reaches ``min_na_per_sample`` are dropped."""
        the_genome = genome
        assert the_genome is not None, "set genotype_cross.genome (potatoCrossGenotyper does) before genotyping"
        log.info("loading input files!")
        vcf = parsers.import_vcf_calls(input_file, self.logDebug, depth=True)
        samples, codes, depth = np.asarray(vcf['samples']), vcf['codes'], vcf['calldata/DP']
        if np.any(codes == parsers.GT_NO_SEPARATOR):
            die("unable to parse the format of GT in vcf!")
        vcf_chr, vcf_pos = np.asarray(vcf['chr']), np.asarray(vcf['pos'], dtype=np.int64)
        chr_ids = genomes._bare(vcf_chr) if len(vcf_chr) else np.zeros(0, dtype="U1")
        the_genome._check(np.unique(chr_ids), "given SNPs")
        for cid in np.unique(chr_ids):
            if cid not in the_genome.chrs_ids:
                raise ValueError("%s: chromosome %s is not in the genome (%s)" % (input_file, cid, ", ".join(the_genome.chrs_ids)))
            here = vcf_pos[chr_ids == cid]
            if len(here) > 1 and np.any(here[1:] <= here[:-1]):
                dup = np.any(here[1:] == here[:-1])
                raise ValueError("%s: chromosome %s holds %s; genotype_cross_hmm needs every position once, in increasing order"
                                 % (input_file, cid, "a position more than once" if dup else "positions out of order"))
        db_rows, vcf_rows = self._matched_rows(vcf_chr, vcf_pos)
        db_rows, vcf_rows = np.asarray(db_rows), np.asarray(vcf_rows)
        p1, p2 = self._parent_calls(db_rows)
        keep = np.flatnonzero((p1 != p2) & (p1 >= 0) & (p2 >= 0))
        log.info("number of segregating snps between parents among the %d matched positions: %d", len(db_rows), len(keep))
        if len(keep) == 0:
            die("no marker of the VCF is a position of the database at which the parents differ: nothing to genotype")
        db_rows, vcf_rows, p1, p2 = db_rows[keep], vcf_rows[keep], p1[keep], p2[keep]
        if max(int(p1.max()), int(p2.max())) > 2:
            raise ValueError("a parent carries call codes other than -1 / 0 / 1 / 2 at %d of the matched markers: genotype_cross_hmm "
                             "models parental calls 0 / 1 / 2 only" % int(np.count_nonzero((p1 > 2) | (p2 > 2))))
        num_markers = len(keep)
        depth = depth[vcf_rows]
        low = (depth <= 0).sum(axis=0) / float(num_markers)
        good = np.where(low < min_na_per_sample)[0]
        log.info("filtering %s samples due to very low number of informative markers" % str(len(samples) - len(good)))
        samples = samples[good]
        halved = depth[:, good] / 2
        levels, rank = np.unique(np.rint(halved), return_inverse=True)
        if len(levels) > 65536:
            raise ValueError("more than 65536 distinct rounded depths in %s" % input_file)
        rank = np.asarray(rank).reshape(halved.shape).astype(np.uint16)
        if "recomb_rates" in the_genome.json.keys():
            mean_recomb_rates = np.mean(np.array(the_genome.json['recomb_rates']))
        else:
            log.warning("Average recombination rates were missing in genome file. Add rates for each chromosome as an array in genome json file under 'recomb_rates' key. Using default rate of 3.5")
            mean_recomb_rates = 3.5

        # one chain per genome chromosome, its markers in panel order; the lines keep the panel's order of chromosomes
        names = self._panel_chromosomes(db_rows)
        positions = np.asarray(self.g.g_acc.positions)[db_rows]
        marker_ids = genomes._bare(names)
        unknown = np.setdiff1d(np.unique(marker_ids), the_genome.chrs_ids)
        if len(unknown):
            raise ValueError("the database names chromosome(s) %s, which the genome does not hold" % ", ".join(unknown))
        order, chain_off, logT = [], [0], []
        for cid, length in zip(the_genome.chrs_ids, the_genome.chrlen):
            mine = np.flatnonzero(marker_ids == cid)
            order.append(mine)
            chain_off.append(chain_off[-1] + len(mine))
            log_t = np.zeros((3, 3))
            if len(mine) >= 2:               # (a chain of one marker takes no step; none at all: no lines, where the reference divides by zero)
                log_t = infer.log_transition(infer._transition_frame(length / 1000000, len(mine), mean_recomb_rates).values)
                if np.isnan(log_t).any():
                    raise ValueError("chromosome %s: %d markers on %d bp at %s cM/Mb give a recombination fraction above 1 per marker; "
                                     "its transition matrix has negative entries" % (cid, len(mine), int(length), mean_recomb_rates))
            logT.append(log_t)
        order = np.concatenate(order)
        _, logI, logE = infer.emission_tables(levels, 0.036)
        state = viterbi_paths(np.ascontiguousarray(codes[vcf_rows[order]][:, good]), np.ascontiguousarray(rank[order]),
                              infer.pair_index(p1[order], p2[order]), np.array(chain_off, dtype=np.int64), np.array(logT), logI, logE)
        in_panel_order = np.empty_like(state)
        in_panel_order[order] = state

        lines = ['id,,,' + ",".join(str(s) for s in samples), 'pheno,,' + ',0' * len(samples)]
        text = np.array(["0", "1", "2"])
        for k in range(num_markers):
            cm = the_genome.estimated_cM_distance("%s,%s" % (names[k], positions[k]))
            lines.append("%s:%s,%s,%s,%s" % (names[k], positions[k], names[k], cm, ",".join(text[in_panel_order[k]])))
        log.info("done!")
        return np.array(lines, dtype=str)

    @staticmethod
    def get_window_genotype_gts(input_gt, snpsP1_gt, snpsP2_gt, lr_thres):
        """one window of one sample from genotype texts (host form, core/genotype_cross.py:184-195)"""
        num_snps = len(input_gt)
        assert num_snps == len(snpsP1_gt), "provide same number of SNPs"
        assert num_snps == len(snpsP2_gt), "provide same number of SNPs"
        calls = parsers.parseGT(input_gt)
        matched = [int(np.count_nonzero(calls == np.asarray(snpsP1_gt))), int(np.count_nonzero(calls == 2)),
                   int(np.count_nonzero(calls == np.asarray(snpsP2_gt)))]
        return getWindowGenotype(matched, num_snps, lr_thres)

    def filter_good_samples(self, snpvcf, good_samples_file):
        return snpvcf                            # (the reference's own call path never passes a file here either)

    # ------------------------------------------------------------------ the accelerated path
    def _matched_rows(self, vcf_chr, vcf_pos):
        """(panel rows, VCF records) of the positions both hold"""
        if hasattr(self.g, "get_positions_idxs"):
            return self.g.get_positions_idxs(vcf_chr, vcf_pos)
        return snp_genotype.Genotype.get_common_positions(self.g.g_acc.chromosomes, self.g.g_acc.positions, vcf_chr, vcf_pos)

    def _parent_calls(self, db_rows):
        """raw panel values of the two parents at ``db_rows`` (int8 each).  A ``Genotype`` serves them from the panel resident on
        the device (``query.gather_columns``: plain, group and streamed panels alike).  That call folds every panel value >= 3 into
        one code, so when either parent shows it the two columns' raw values are fetched on the host instead.  Any other ``g``
        (``accessions`` and ``g_acc.snps`` / ``chromosomes`` / ``positions`` are all that is asked of it) is read on the host."""
        from .. import dist
        if len(db_rows) and hasattr(self.g, "panel") and dist.job() is None:       # (an accession-sharded job holds a parent on another rank)
            query = self.g.panel().query(db_rows, np.zeros((len(db_rows), 3)))
            try:
                two = query.gather_columns(np.array([self.p1_ix, self.p2_ix]))
            finally:
                query.free()
            if int(np.where(two == 0xFF, 0, two).max(initial=0)) <= 2:
                return np.where(two == 0xFF, -1, two).astype(np.int8)
            log.info("a parent carries call codes above 2: reading the two columns on the host")
        snps = self.g.g_acc.snps
        return np.stack([np.asarray(snps[db_rows, self.p1_ix]), np.asarray(snps[db_rows, self.p2_ix])]).astype(np.int8)

    def genotype_cross(self, input_file, lr_thres, good_samples_file=None):
        """lines of the R/qtl CSV: two header lines, then one line per genome window"""
        the_genome = genome
        assert the_genome is not None, "set genotype_cross.genome (potatoCrossGenotyper does) before genotyping"
        log.info("loading input files!")
        vcf = parsers.import_vcf_calls(input_file, self.logDebug)
        samples, codes = vcf['samples'], vcf['codes']
        num_samples = len(samples)
        log.info("number of samples printed: %s" % num_samples)
        if np.any(codes == parsers.GT_NO_SEPARATOR):
            die("unable to parse the format of GT in vcf!")
        vcf_chr, vcf_pos = np.asarray(vcf['chr']), np.asarray(vcf['pos'], dtype=np.int64)
        chr_ids = genomes._bare(vcf_chr) if len(vcf_chr) else np.zeros(0, dtype="U1")
        the_genome._check(np.unique(chr_ids), "given SNPs")
        for cid in np.unique(chr_ids):
            here = vcf_pos[chr_ids == cid]
            if len(here) and here[0] < 1:
                raise ValueError("%s: chromosome %s holds a position below 1" % (input_file, cid))
            if len(here) > 1 and np.any(here[1:] <= here[:-1]):
                dup = np.any(here[1:] == here[:-1])
                raise ValueError("%s: chromosome %s holds %s; genotype_cross needs every position once, in increasing order"
                                 % (input_file, cid, "a position more than once" if dup else "positions out of order"))
        db_rows, vcf_rows = self._matched_rows(vcf_chr, vcf_pos)
        p1, p2 = self._parent_calls(db_rows)
        keep = np.flatnonzero((p1 != p2) & (p1 >= 0) & (p2 >= 0))
        log.info("number of segregating snps between parents among the %d matched positions: %d", len(db_rows), len(keep))
        vcf_rows, p1, p2 = np.asarray(vcf_rows)[keep], p1[keep], p2[keep]
        if len(keep) and max(int(p1.max()), int(p2.max())) > 2:
            raise ValueError("a parent carries call codes other than -1 / 0 / 1 / 2 at %d of the matched markers: genotype_cross "
                             "compares the parents with sample calls 0 / 1 / 2 only" % int(np.count_nonzero((p1 > 2) | (p2 > 2))))

        # window of every marker: windows [1 + k b, (k + 1) b] of every genome chromosome, in genome order (Genome.get_bins_arrays)
        table = the_genome.window_table(self.window_size)
        n_win = len(table)
        per_chr = np.array([len(range(1, int(n), self.window_size)) for n in the_genome.chrlen], dtype=np.int64)
        first_win = np.concatenate(([0], np.cumsum(per_chr)))
        chr_ix = np.full(len(vcf_rows), -1, dtype=np.int64)
        marker_ids = chr_ids[vcf_rows]
        for k, cid in enumerate(the_genome.chrs_ids):
            chr_ix[marker_ids == cid] = k
        rel = (vcf_pos[vcf_rows] - 1) // self.window_size
        inside = (chr_ix >= 0) & (rel >= 0) & (rel < per_chr[np.maximum(chr_ix, 0)])
        win = first_win[np.maximum(chr_ix, 0)] + rel
        vcf_rows, p1, p2, win = vcf_rows[inside], p1[inside], p2[inside], win[inside]
        order = np.lexsort((vcf_rows, win))          # window by window, file order inside a window (its first record governs the separator)
        vcf_rows, p1, p2, win = vcf_rows[order], p1[order], p2[order], win[order]
        win_off = np.concatenate(([0], np.cumsum(np.bincount(win, minlength=n_win)))).astype(np.int64)

        geno = count_and_decide(np.ascontiguousarray(codes[vcf_rows]), p1, p2, win_off, lr_thres)
        log.warning("Using an average recombination rates of 3. Please change it according or use R/qtl package to generate genetic map.")
        lines = ['id,,,' + ",".join(str(s) for s in samples), 'pheno,,' + ',0' * num_samples]
        text = np.array(["NA", "0", "1", "2"])
        for w, (c, start, end) in enumerate(table):
            chrid = the_genome.chrs_ids[c]
            cm_mid = the_genome.estimated_cM_distance(chrid + "," + str(int(round(np.mean([start, end])))))
            if win_off[w + 1] == win_off[w]:
                calls = ',NA' * num_samples
            else:
                calls = "".join("," + t for t in text[geno[w].astype(np.int64) + 1])
            lines.append("%s,%s,%s%s" % ("%s:%s-%s" % (chrid, start, end), chrid, cm_mid, calls))
        log.info("done!")
        return np.array(lines, dtype=str)

    @staticmethod
    def write_output_genotype_cross(outfile_str, output_file):
        log.info("writing file: %s" % output_file)
        with open(output_file, 'w') as fh:
            for line in outfile_str:
                fh.write("%s\n" % line)
        log.info("done!")


def potatoCrossGenotyper(args):
    """entry point of ``snpmatch genotype_cross``"""
    global genome
    if args.get('father') is not None:
        die(FATHER_REFUSED)
    genome = genomes.Genome(args['genome'])
    log.info("loading database files")
    g = snp_genotype.Genotype(args['hdf5File'], args['hdf5accFile'])
    log.info("done!")
    crossgenotyper = GenotypeCross(g, args['parents'], args['binLen'], args['father'], args['logDebug'])
    if args.get('hmm'):
        outfile_str = crossgenotyper.genotype_cross_hmm(args['inFile'])
    else:
        outfile_str = crossgenotyper.genotype_cross(args['inFile'], args['lr_thres'])
    crossgenotyper.write_output_genotype_cross(outfile_str, args['outFile'])
