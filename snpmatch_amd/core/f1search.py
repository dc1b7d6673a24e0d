"""
``snpmatch f1search``: which two accessions of the database are the parents of a sample that is an F1 (or a 1:1 mixture of two
lines) -- asked of EVERY pair of accessions, not of the ten that match best on their own.

``cross`` follows the reference: ``CrossIdentifier.match_insilico_f1s`` (core/csmatch.py:106-129) crosses in silico the ten
accessions with the highest single match fraction, 45 pairs.  Each parent of an F1 matches the sample only where the two parents
agree, so in a panel that holds relatives of either parent ten other lines can out-rank both, and the true pair is never tried.
Here the hard calls of the sample are scored against the in-silico F1 of all n (n - 1) / 2 pairs in one device call
(``Genotype.f1_counts`` -> ``engine.f1_counts`` -> ``snpm_panel_f1_counts``): two exact int32 matrices, ``hits`` and ``ninfo``.
With the one-hot weights of a hard-called sample they ARE the reference's score and numinfo of every pair.

The search on top of the counts is host work: pairs a < b with ``ninfo >= --min_sites`` are ranked by ``hits / ninfo`` (compared
exactly, as integers), ties to the larger ``ninfo``, then to the smaller (a, b); the first ``--top`` pairs are the shortlist.  For a
sample with PL weights the hard-call counts are a screen, not the reference's score: the shortlist is re-scored with the real
weights through ``Query.f1_pairs`` (``snpm_query_f1_pairs``, numpy's summation order), called once on the distinct members, and
likelihood and LRT come from ``GenotyperOutput.calculate_likelihoods`` over the single-accession result plus the shortlisted pairs
-- the way the reference appends its F1 rows.

The reference has no such command: the files and ``--min_sites`` are this package's own, and the threshold is a user setting, not a
claim.

  <prefix>.f1search.scores.txt   the eight columns of ``scores.txt``: the accessions, then the ``--top`` pairs as ``AxB``
  <prefix>.f1search.npz          accessions (the candidates), hits, ninfo (int32 [n, n]), class_rows (matched rows of class ref, alt,
                                 het, none)
  <prefix>.f1search.json         matched rows, the best single accession and the best pair with their fractions, the shortlist with
                                 hard counts and exact scores, and ``in_top10_route``: whether the best pair is among the 45 the
                                 reference's route would have tried
"""
import functools
import itertools
import json
import logging

import numpy as np

from . import _select, parsers, snp_genotype, snpmatch
from ._select import hard_classes  # noqa: F401  (the name tests and tools import)

log = logging.getLogger(__name__)

TOP = 10                    # default of --top: pairs of the shortlist
MAX_TOP = 16                # ... at most: the members of 16 pairs fit the 32 accessions of one snpm_query_f1_pairs call
MIN_SITES = 100             # default of --min_sites: informative rows below which a pair is not ranked
NO_CLASS = _select.NO_CLASS


def _better(p, q):
    """pairs (h, n, a, b): a higher h / n first (h1 n2 against h2 n1, exact), then the larger n, then the smaller (a, b)"""
    left, right = p[0] * q[1], q[0] * p[1]
    if left != right:
        return -1 if left > right else 1
    if p[1] != q[1]:
        return -1 if p[1] > q[1] else 1
    return -1 if (p[2], p[3]) < (q[2], q[3]) else (1 if (p[2], p[3]) > (q[2], q[3]) else 0)


def shortlist(hits, ninfo, top=TOP, min_sites=MIN_SITES):
    """The ``top`` best pairs a < b of the two count matrices as a list of (a, b, hits, ninfo): pairs with ``ninfo >= min_sites``
    (and at least one informative row) ranked by hits / ninfo, descending and exact; ties to the larger ninfo, then the smaller
    (a, b).  The candidates of the exact ranking are found in fp64: division is monotone, so a pair of the exact first ``top``
    cannot lie below the ``top``-th largest rounded fraction."""
    top = int(top)
    if not 1 <= top <= MAX_TOP:
        raise ValueError("top must be 1 .. %d (the members of the shortlist go through one call of %d accessions), got %d" % (MAX_TOP, 2 * MAX_TOP, top))
    hits, ninfo = np.asarray(hits), np.asarray(ninfo)
    assert hits.ndim == 2 and hits.shape == ninfo.shape and hits.shape[0] == hits.shape[1], "hits / ninfo: two square matrices"
    a, b = np.triu_indices(hits.shape[0], k=1)
    h, n = hits[a, b].astype(np.int64), ninfo[a, b].astype(np.int64)
    keep = n >= max(int(min_sites), 1)
    a, b, h, n = a[keep], b[keep], h[keep], n[keep]
    if len(a) > top:
        frac = h / n.astype(np.float64)
        cut = np.partition(frac, len(frac) - top)[len(frac) - top]
        near = frac >= cut
        a, b, h, n = a[near], b[near], h[near], n[near]
    rows = sorted(zip(h.tolist(), n.tolist(), a.tolist(), b.tolist()), key=functools.cmp_to_key(_better))[:top]
    return [(a_, b_, h_, n_) for h_, n_, a_, b_ in rows]


class F1Search(object):
    """The single-accession result of ``Genotyper``, the hard-call counts of every pair of candidate accessions, the shortlist and
    its exact scores.  ``acc_ix``: the candidate accessions (None: all); ``run_search=False`` leaves the steps to the caller."""

    def __init__(self, inputs, g, output_id="f1search", top=TOP, min_sites=MIN_SITES, acc_ix=None, run_search=True):
        assert type(inputs) is parsers.ParseInputs, "provide a parsers class"
        top, min_sites = int(top), int(min_sites)
        if not 1 <= top <= MAX_TOP:
            raise ValueError("--top must be 1 .. %d, got %d" % (MAX_TOP, top))
        if min_sites < 0:
            raise ValueError("--min_sites must not be negative, got %d" % min_sites)
        self.inputs, self.g, self.output_id, self.top, self.min_sites = inputs, g, output_id, top, min_sites
        self.acc_ix = None if acc_ix is None else np.asarray(acc_ix, dtype=np.int64).reshape(-1)
        if self.acc_ix is not None and len(np.unique(self.acc_ix)) != len(self.acc_ix):
            raise ValueError("a candidate accession is listed twice: a line crossed with itself is no pair")
        if run_search:
            self.search()
            self.write_outputs()

    def search(self):
        # 1. every accession on its own: the existing genotyper
        self.result = snpmatch.Genotyper(self.inputs, self.g, self.output_id, run_genotyper=False).genotyper()
        # 2. the matched rows
        self.db_rows, self.sample_rows = self.g.get_positions_idxs(self.inputs.chrs, self.inputs.pos, _parsed=self.inputs)
        # 3. every pair of candidates against the hard calls, one device call
        self.classes = hard_classes(self.inputs.gt)[self.sample_rows]
        self.hits, self.ninfo = self.g.f1_counts(self.classes, self.acc_ix, self.db_rows)
        # 4. the shortlist, in DB accession indices
        cand = np.arange(len(self.g.accessions)) if self.acc_ix is None else self.acc_ix
        self.pairs = [(int(cand[a]), int(cand[b]), h, n) for a, b, h, n in shortlist(self.hits, self.ninfo, self.top, self.min_sites)]
        # 5. the shortlist with the sample's real weights: one call on the distinct members, the listed pairs picked out
        self.pair_scores, self.pair_ninfo = self._rescore([(a, b) for a, b, _, _ in self.pairs])
        log.info("f1search: %d matched rows, %d candidate accessions, %d pairs shortlisted", len(self.db_rows), len(cand), len(self.pairs))
        return self.pairs

    def _rescore(self, pairs):
        if not pairs:
            return np.zeros(0, dtype=np.float64), np.zeros(0, dtype=np.int64)
        members = sorted(set(itertools.chain.from_iterable(pairs)))
        query = self.g.panel().query(self.db_rows, self.inputs.wei[self.sample_rows, ])
        score, ninfo = query.f1_pairs(np.array(members, dtype=np.int32))
        query.free()
        at = {pair: k for k, pair in enumerate(itertools.combinations(members, 2))}
        pick = [at[(a, b) if a < b else (b, a)] for a, b in pairs]
        return np.asarray(score, dtype=np.float64)[pick], np.asarray(ninfo, dtype=np.int64)[pick]

    def summary(self):
        res, names = self.result, [str(n) for n in self.g.accessions]
        if not hasattr(res, 'probabilies'):
            res.get_probabilities()
        singles = np.asarray(res.probabilies[:len(names)], dtype=float)
        route = np.argsort(-singles)[0:10]                      # the accessions match_insilico_f1s would cross
        out = {"matched_rows": int(len(self.db_rows)), "candidates": int(len(names) if self.acc_ix is None else len(self.acc_ix)),
               "top": self.top, "min_sites": self.min_sites,
               "class_rows": {k: int(np.count_nonzero(self.classes == c)) for k, c in (("ref", 0), ("alt", 1), ("het", 2), ("none", NO_CLASS))},
               "best_single": None, "best_pair": None, "shortlist": [], "in_top10_route": None}
        if len(singles) and not np.all(np.isnan(singles)):
            k = int(np.nanargmax(singles))
            out["best_single"] = {"accession": names[k], "score": float(res.scores[k]), "ninfo": int(res.ninfo[k]), "fraction": float(singles[k])}
        for (a, b, h, n), s, ni in zip(self.pairs, self.pair_scores.tolist(), self.pair_ninfo.tolist()):
            out["shortlist"].append({"acc_1": names[a], "acc_2": names[b], "hits": int(h), "ninfo": int(n), "hard_fraction": h / float(n),
                                     "score": float(s), "numinfo": int(ni), "fraction": (s / ni if ni > 0 else None)})
        if self.pairs:
            out["best_pair"] = out["shortlist"][0]
            out["in_top10_route"] = bool(self.pairs[0][0] in route and self.pairs[0][1] in route)
        return out

    def write_outputs(self):
        names = np.asarray(self.g.accessions).astype("U")
        stats = self.summary()
        res = self.result
        if self.pairs:                      # as match_insilico_f1s appends its F1 rows; likelihoods over accessions and pairs together
            res.scores = np.append(res.scores, self.pair_scores)
            res.ninfo = np.append(res.ninfo, self.pair_ninfo)
            res.accs = np.append(res.accs, [names[a] + "x" + names[b] for a, b, _, _ in self.pairs])
        res.print_out_table(self.output_id + ".f1search.scores.txt", _frame=False)
        np.savez(self.output_id + ".f1search.npz", accessions=names if self.acc_ix is None else names[self.acc_ix], hits=self.hits, ninfo=self.ninfo,
                 class_rows=np.array([stats["class_rows"][k] for k in ("ref", "alt", "het", "none")], dtype=np.int64))
        with open(self.output_id + ".f1search.json", "w") as out:
            json.dump(stats, out, indent=1, sort_keys=True)
            out.write("\n")
        self.stats = stats
        return stats


def potatoF1Search(args):
    """entry point of ``snpmatch f1search``"""
    given = lambda key, default: default if args.get(key) is None else args[key]      # noqa: E731
    top, min_sites = int(given('top', TOP)), int(given('min_sites', MIN_SITES))
    if not 1 <= top <= MAX_TOP:
        raise ValueError("--top must be 1 .. %d, got %d" % (MAX_TOP, top))
    if min_sites < 0:
        raise ValueError("--min_sites must not be negative, got %d" % min_sites)
    inputs = snpmatch.parse_inputs_once(args['inFile'], args.get('logDebug', False))
    log.info("loading genotype files!")
    g = snp_genotype.Genotype(args['hdf5File'], args.get('hdf5accFile'))
    acc_ix, _ = _select.accessions_of(g, args)
    search = F1Search(inputs, g, args['outFile'], top, min_sites, acc_ix)
    log.info("finished!")
    return search.stats
