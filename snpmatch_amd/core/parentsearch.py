"""
``snpmatch parentsearch``: which two accessions of the database are the parents of a RECOMBINANT sample -- an F2, a backcross, a RIL
with residual heterozygosity -- asked of EVERY pair of accessions, genome window by genome window.

Such a sample is a mosaic along the genome: in one stretch it is parent A, in the next the F1 of A and B, in the next parent B.
``cross`` follows the reference (``CrossIdentifier``, core/csmatch.py:106-186): it crosses in silico the ten accessions that match best
on their own and guesses the parents of an F2 from the accessions that win "clean" windows; ``f1search`` scores every pair, but as a
whole-genome F1.  Neither finds the parents of a mosaic in a panel that holds relatives of it: each parent matches the sample in
its own stretches only, and the whole-genome F1 of the true pair is wrong wherever the sample is homozygous.

Here the matched rows are grouped by genome window (``csmatch._window_segments``) and the sample's hard calls are scored against
every pair of candidates in one device call (``Genotype.parent_counts`` -> ``engine.parent_counts`` -> ``snpm_panel_parent_counts``):
per pair (a, b) and window, over the n rows where the F1 of a and b is informative and the sample has a class, hA / hB / hF rows
carry the sample's class in a, in b, in their F1; a window with ``--min_win_sites`` rows or more adds max(hA, hB, hF) to the pair's
score and n to its total, and counts as A, as B or -- hF strictly the largest -- as AB.  Four exact int32 matrices.  The pairs a < b
with ``n >= --min_sites`` are ranked by score / n with ``f1search.shortlist`` (exact, ties to the larger n); for the ``--top`` pairs
the per-window counts and states are recomputed on the host from the two columns (``window_tracks``).

The hard-call screen is the result here: there is no re-scoring with PL weights per window (the caveat of ``f1search`` applies).
The reference has no such command: the files and thresholds are this package's own.

  <prefix>.parentsearch.json          matched rows, windows, the best single accession, the shortlist with score, n, fraction, the
                                      windows taken as A / B / AB / unused, and ``in_top10_route``: whether the best pair is among
                                      the 45 the reference's route would have crossed
  <prefix>.parentsearch.npz           accessions (the candidates), score, n_tot, w_first, w_het (int32 [n, n]), win_off, win_chr
  <prefix>.parentsearch.windows.tsv   chromosome, window, pair, n, hA, hB, hF, state (A / B / AB / NA) for the shortlisted pairs
"""
import json
import logging

import numpy as np

from . import _select, csmatch, f1search, genomes, parsers, snp_genotype, snpmatch

log = logging.getLogger(__name__)

TOP = f1search.TOP
MIN_SITES = f1search.MIN_SITES
MIN_WIN_SITES = 5           # default of --min_win_sites: rows below which a window is not used for a pair
STATES = ("A", "B", "AB", "NA")


def _canonical(col):
    col = np.asarray(col).astype(np.int64)
    return np.where(col < 0, -1, np.where(col > 2, 3, col))


def window_tracks(col_a, col_b, classes, win_off, min_win_sites=MIN_WIN_SITES, a_first_on_tie=True):
    """Per window the counts (n, hA, hB, hF) and the state of ONE pair, from the two gathered DB columns (int8 calls of the matched
    rows, in window order) and the sample's classes: int64 [n_win, 4] and int8 [n_win] (index into STATES).  ``a_first_on_tie``:
    whether a window with hA == hB >= hF goes to A (the pair's a has the smaller position in the candidate list)."""
    x, y, s = _canonical(col_a), _canonical(col_b), np.asarray(classes).astype(np.int64)
    f1 = np.where((x == 0) & (y == 0), 0, np.where((x == 1) & (y == 1), 1, np.where((x >= 0) & (y >= 0) & (x != y), 2, -1)))
    ni = (f1 >= 0) & (s <= 2)
    win_off = np.asarray(win_off, dtype=np.int64)
    per_row = np.stack([ni, ni & (x == s), ni & (y == s), ni & (f1 == s)], axis=1).astype(np.int64)
    sums = np.concatenate([np.zeros((1, 4), dtype=np.int64), np.cumsum(per_row, axis=0)])
    counts = sums[win_off[1:]] - sums[win_off[:-1]]
    n, ha, hb, hf = counts.T
    state = np.where(n < int(min_win_sites), 3, np.where(hf > np.maximum(ha, hb), 2, np.where((ha > hb) | ((ha == hb) & bool(a_first_on_tie)), 0, 1)))
    return counts, state.astype(np.int8)


class ParentSearch(object):
    """The single-accession result of ``Genotyper``, the matched rows by genome window, the four matrices of every pair of candidate
    accessions, the shortlist and its window tracks.  ``acc_ix``: the candidate accessions (None: all); ``run_search=False`` leaves
    the steps to the caller."""

    def __init__(self, inputs, g, genome_id, binLen, output_id="parentsearch", top=TOP, min_sites=MIN_SITES, min_win_sites=MIN_WIN_SITES,
                 acc_ix=None, run_search=True):
        assert type(inputs) is parsers.ParseInputs, "provide a parsers class"
        top, min_sites, min_win_sites = int(top), int(min_sites), int(min_win_sites)
        if not 1 <= top <= f1search.MAX_TOP:
            raise ValueError("--top must be 1 .. %d, got %d" % (f1search.MAX_TOP, top))
        if min_sites < 0:
            raise ValueError("--min_sites must not be negative, got %d" % min_sites)
        if min_win_sites < 1:
            raise ValueError("--min_win_sites must be 1 or more, got %d" % min_win_sites)
        if int(binLen) < 1:
            raise ValueError("--binLength must be 1 or more, got %d" % int(binLen))
        inputs.filter_chr_names()
        self.inputs, self.g, self.output_id = inputs, g, output_id
        self.genome, self.binLen = genomes.Genome(genome_id), int(binLen)
        self.top, self.min_sites, self.min_win_sites = top, min_sites, min_win_sites
        self.acc_ix = None if acc_ix is None else np.asarray(acc_ix, dtype=np.int64).reshape(-1)
        if self.acc_ix is not None and len(np.unique(self.acc_ix)) != len(self.acc_ix):
            raise ValueError("a candidate accession is listed twice: a line crossed with itself is no pair")
        if run_search:
            self.search()
            self.write_outputs()

    def search(self):
        # 1. every accession on its own: the existing genotyper
        self.result = snpmatch.Genotyper(self.inputs, self.g, self.output_id, run_genotyper=False).genotyper()
        # 2. the matched rows in window order
        self.db_rows, self.sample_rows, self.win_off, self.win_chr = csmatch._window_segments(self.genome, self.g.g, self.inputs, self.binLen)
        self.db_rows = np.asarray(self.db_rows, dtype=np.int64)
        self.win_off = np.asarray(self.win_off, dtype=np.int64)
        # 3. every pair of candidates, window by window, against the hard calls: one device call
        self.classes = f1search.hard_classes(self.inputs.gt)[self.sample_rows]
        self.score, self.n_tot, self.w_first, self.w_het = self.g.parent_counts(self.classes, self.win_off, self.min_win_sites, self.acc_ix, self.db_rows)
        # 4. the shortlist, in DB accession indices
        self.cand = np.arange(len(self.g.accessions)) if self.acc_ix is None else self.acc_ix
        self.listed = f1search.shortlist(self.score, self.n_tot, self.top, self.min_sites)
        self.pairs = [(int(self.cand[a]), int(self.cand[b]), h, n) for a, b, h, n in self.listed]
        # 5. the window tracks of the shortlisted pairs, from their columns
        self.tracks = []
        members = sorted(set(m for a, b, _, _ in self.pairs for m in (a, b)))
        cols = self._gather(members)
        for (pa, pb, _, _), (a, b, _, _) in zip(self.listed, self.pairs):
            self.tracks.append(window_tracks(cols[a], cols[b], self.classes, self.win_off, self.min_win_sites, pa <= pb))
        log.info("parentsearch: %d matched rows in %d windows, %d candidate accessions, %d pairs shortlisted", len(self.db_rows), len(self.win_off) - 1,
                 len(self.cand), len(self.pairs))
        return self.pairs

    def _gather(self, members):
        """the calls of the listed accessions at the matched rows, {accession: int8 [rows]}"""
        if not members:
            return {}
        snps = self.g.g.snps
        rows = self.db_rows
        order = np.argsort(rows, kind="stable")                 # (HDF5-backed matrices want increasing rows)
        back = np.empty_like(order)
        back[order] = np.arange(len(order))
        uniq, inverse = np.unique(rows[order], return_inverse=True)
        block = np.asarray(snps[uniq, :] if len(uniq) else np.zeros((0, len(self.g.accessions)), dtype=np.int8))
        return {m: np.asarray(block[:, m])[inverse][back] for m in members}

    def summary(self):
        res, names = self.result, [str(n) for n in self.g.accessions]
        if not hasattr(res, 'probabilies'):
            res.get_probabilities()
        singles = np.asarray(res.probabilies[:len(names)], dtype=float)
        route = np.argsort(-singles)[0:10]                      # the accessions match_insilico_f1s would cross
        n_win = len(self.win_off) - 1
        out = {"matched_rows": int(len(self.db_rows)), "windows": int(n_win), "windows_with_rows": int(np.count_nonzero(np.diff(self.win_off))),
               "bin_length": self.binLen, "candidates": int(len(self.cand)), "top": self.top, "min_sites": self.min_sites,
               "min_win_sites": self.min_win_sites,
               "class_rows": {k: int(np.count_nonzero(self.classes == c)) for k, c in (("ref", 0), ("alt", 1), ("het", 2), ("none", f1search.NO_CLASS))},
               "best_single": None, "best_pair": None, "shortlist": [], "in_top10_route": None}
        if len(singles) and not np.all(np.isnan(singles)):
            k = int(np.nanargmax(singles))
            out["best_single"] = {"accession": names[k], "score": float(res.scores[k]), "ninfo": int(res.ninfo[k]), "fraction": float(singles[k])}
        for (pa, pb, _, _), (a, b, h, n) in zip(self.listed, self.pairs):
            as_a, as_b, as_ab = int(self.w_first[pa, pb]), int(self.w_first[pb, pa]), int(self.w_het[pa, pb])
            out["shortlist"].append({"acc_1": names[a], "acc_2": names[b], "score": int(h), "n": int(n), "fraction": h / float(n),
                                     "windows_A": as_a, "windows_B": as_b, "windows_AB": as_ab, "windows_unused": int(n_win - as_a - as_b - as_ab)})
        if self.pairs:
            out["best_pair"] = out["shortlist"][0]
            out["in_top10_route"] = bool(self.pairs[0][0] in route and self.pairs[0][1] in route)
        return out

    def write_outputs(self):
        names = np.asarray(self.g.accessions).astype("U")
        stats = self.summary()
        np.savez(self.output_id + ".parentsearch.npz", accessions=names[self.cand], score=self.score, n_tot=self.n_tot, w_first=self.w_first,
                 w_het=self.w_het, win_off=self.win_off, win_chr=np.asarray(self.win_chr, dtype=np.int64))
        chrs = [str(c) for c in self.genome.chrs]
        with open(self.output_id + ".parentsearch.windows.tsv", "w") as out:
            out.write("chr\twindow\tpair\tn\thA\thB\thF\tstate\n")
            for (a, b, _, _), (counts, state) in zip(self.pairs, self.tracks):
                pair = "%sx%s" % (names[a], names[b])
                for w, ((n, ha, hb, hf), st) in enumerate(zip(counts.tolist(), state.tolist())):
                    out.write("%s\t%d\t%s\t%d\t%d\t%d\t%d\t%s\n" % (chrs[int(self.win_chr[w])], w, pair, n, ha, hb, hf, STATES[st]))
        with open(self.output_id + ".parentsearch.json", "w") as out:
            json.dump(stats, out, indent=1, sort_keys=True)
            out.write("\n")
        self.stats = stats
        return stats


def potatoParentSearch(args):
    """entry point of ``snpmatch parentsearch``"""
    given = lambda key, default: default if args.get(key) is None else args[key]      # noqa: E731
    inputs = snpmatch.parse_inputs_once(args['inFile'], args.get('logDebug', False))
    log.info("loading genotype files!")
    g = snp_genotype.Genotype(args['hdf5File'], args.get('hdf5accFile'))
    acc_ix, _ = _select.accessions_of(g, args)
    search = ParentSearch(inputs, g, given('genome', "athaliana_tair10"), int(given('binLen', 300000)), args['outFile'], int(given('top', TOP)),
                          int(given('min_sites', MIN_SITES)), int(given('min_win_sites', MIN_WIN_SITES)), acc_ix)
    log.info("finished!")
    return search.stats
