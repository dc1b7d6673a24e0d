"""
``snpmatch power``: with n random SNPs and a call error rate e, which accessions of the database does ``inbred`` identify uniquely, which
does it confuse, and with whom -- for EVERY accession and a whole ladder of marker counts at once.  The reference answers the question
one accession and one n at a time (``simulate`` writes a sample file, ``inbred`` is run on it); here a trial is one device call
(``Genotype.sim_counts`` -> ``engine.sim_counts`` -> ``snpm_panel_sim_counts``): the sample simulated from every accession -- its calls
at the trial's markers with errors injected by a counter-based hash -- scored against every accession, exact int32 ``score`` / ``ninfo``
per group of markers.  The host draws the marker ladder, sums the groups up to the nested levels and applies the likelihood test of
``inbred`` (likeliTest / calculate_likelihoods, core/snpmatch.py:40-55, :106-117 of the reference) to every row of a level's matrix.

The ladder of a trial: ONE permutation of the candidate rows from ``np.random.default_rng(seed)`` (the trials draw one after the other
from the same generator); its first n_1 rows are level 1, the next n_2 - n_1 rows complete level 2, and so on.  The rows are sorted
ascending inside a group and the groups concatenated, so no row is staged twice and the cumulative sum over the groups gives the levels.
Trial t injects its errors under the hash seed ``seed + t``.

Differences from the reference's ``simulateSNPs`` (core/simulate.py:26-53), on purpose:
  * one marker set per trial is shared by all accessions, and a sample has a call where its accession has one (0, 1 or 2): the
    reference draws exactly n rows from that accession's informative rows
  * errors are Bernoulli per call (rate e): the reference changes exactly int(e * n) calls
  * a DB row with a code other than 0 / 1 / 2 gives no sample call
  * F1 samples (``--f1``) are not part of ``power``

  <prefix>.power.tsv    trial, level, n_markers, accession, n_sites, score_self, correct, n_ambiguous, unique, best_other,
                        best_other_ratio -- one line per trial, level and accession
  <prefix>.power.json   the summary: per level the fraction of (accession, trial) that is correct / unique, per accession the smallest
                        level at which it is unique in every trial, the pairs still confused at the largest level
  <prefix>.power.npz    accessions, levels, and score / ninfo [n_levels, n, n] (cumulative) of the last trial
"""
import json
import logging

import numpy as np

from . import _select, snp_genotype

log = logging.getLogger(__name__)

LR_THRES = 3.841            # default of --lr_thres: the reference's lr_thres (core/snpmatch.py:22)
P_MATCH = 0.99999999        # likeliTest's p (core/snpmatch.py:41)
MAX_LEVELS = 64             # groups of one ``sim_counts`` call


def parse_levels(text):
    """``-n 100,1000,10000`` as a strictly increasing list of positive marker counts"""
    levels = [int(t) for t in str(text).split(",") if t.strip()]
    if not levels or any(n <= 0 for n in levels) or any(b <= a for a, b in zip(levels, levels[1:])):
        raise ValueError("-n takes marker counts in strictly increasing order, e.g. 100,1000,10000: got %r" % (text,))
    if len(levels) > MAX_LEVELS:
        raise ValueError("at most %d levels per run: got %d" % (MAX_LEVELS, len(levels)))
    return levels


def draw_ladder(n_rows, levels, rng, pool=None):
    """The marker ladder of one trial.  ``pool``: the candidate DB rows (None: 0 .. n_rows - 1).  Returns ``(rows, grp_off)``: the rows
    of level i are ``rows[:grp_off[i + 1]]``, sorted ascending inside each group.  A level above the number of candidates is cut to it."""
    pool = np.arange(n_rows, dtype=np.int64) if pool is None else np.asarray(pool, dtype=np.int64)
    perm = rng.permutation(len(pool))
    grp_off = np.array([0] + [min(int(n), len(pool)) for n in levels], dtype=np.int64)
    groups = [np.sort(pool[perm[lo:hi]]) for lo, hi in zip(grp_off[:-1], grp_off[1:])]
    return (np.concatenate(groups) if groups else np.zeros(0, dtype=np.int64)), grp_off


def likelihoods(score, ninfo):
    """likeliTest and calculate_likelihoods(amin="calc") over every ROW of [n, m] count matrices: ``(lik, lrt)`` fp64 [n, m].  lik is
    nan where ninfo or score is 0 and the sentinel 1 where score == ninfo > 0; lrt = lik / the row's smallest lik, nan where that is
    not positive (get_fraction)."""
    y, n = np.asarray(score, dtype=np.float64), np.asarray(ninfo, dtype=np.float64)
    assert (y <= n).all(), "provided y is greater than n"
    with np.errstate(divide="ignore", invalid="ignore"):
        ps = y / n
        lik = y * np.log(ps / P_MATCH) + (n - y) * np.log((1 - ps) / (1 - P_MATCH))
        lik = np.where((n > 0) & (y > 0), lik, np.nan)
        lik = np.where((n > 0) & (y == n), 1.0, lik)
        top = np.nanmin(np.where(np.isnan(lik), np.inf, lik), axis=1, keepdims=True)
        top = np.where(np.isinf(top), np.nan, top)
        lrt = np.where(top > 0, lik / top, np.nan)
    return lik, lrt


def level_report(score, ninfo, lr_thres=LR_THRES):
    """What ``inbred`` would say about the sample of every accession at one level.  score / ninfo [n, n] (sample a in row a).  Returns a
    dict of arrays [n]: n_sites, score_self, correct (the likelihood of (a, a) is the row's minimum), n_ambiguous (accessions with
    ratio below lr_thres), unique (correct and n_ambiguous == 1), best_other (index of the best other accession, -1 without one),
    best_other_ratio -- and ``lrt`` [n, n]."""
    score, ninfo = np.asarray(score), np.asarray(ninfo)
    n = len(score)
    lik, lrt = likelihoods(score, ninfo)
    diag = np.arange(n)
    filled = np.where(np.isnan(lik), np.inf, lik)
    self_lik = lik[diag, diag]
    correct = ~np.isnan(self_lik) & (self_lik == filled.min(axis=1))
    with np.errstate(invalid="ignore"):
        n_amb = (lrt < lr_thres).sum(axis=1)
    others = filled.copy()
    others[diag, diag] = np.inf
    best = others.argmin(axis=1) if n > 1 else np.full(n, -1)
    has = np.isfinite(others[diag, best]) if n > 1 else np.zeros(n, dtype=bool)
    best = np.where(has, best, -1)
    ratio = np.where(has, lrt[diag, np.maximum(best, 0)], np.nan)
    return dict(n_sites=ninfo[diag, diag].astype(np.int64), score_self=score[diag, diag].astype(np.int64), correct=correct,
                n_ambiguous=n_amb.astype(np.int64), unique=correct & (n_amb == 1), best_other=best.astype(np.int64),
                best_other_ratio=ratio, lrt=lrt)


class Power(object):
    """The study of one database: ``trials`` ladders of ``levels`` markers, errors at ``err_rate``."""

    def __init__(self, g, levels, err_rate=0.001, trials=3, seed=1, lr_thres=LR_THRES, acc_ix=None, snp_ix=None):
        if not 0.0 <= err_rate <= 1.0:
            raise ValueError("the error rate must lie in 0 .. 1: got %r" % (err_rate,))
        if trials < 1:
            raise ValueError("--trials must be 1 or more")
        self.g, self.levels, self.err_rate, self.trials, self.seed, self.lr_thres = g, list(levels), float(err_rate), int(trials), int(seed), float(lr_thres)
        self.acc_ix = None if acc_ix is None else np.asarray(acc_ix, dtype=np.int64)
        self.names = np.asarray(g.accessions)[self.acc_ix] if self.acc_ix is not None else np.asarray(g.accessions)
        self.pool = None if snp_ix is None else np.asarray(snp_ix, dtype=np.int64)
        self.n_rows = len(g.g.positions) if self.pool is None else len(self.pool)
        self.reports = []           # [trial][level] -> level_report
        self.markers = None         # markers of every level (the same in every trial)
        self.score = self.ninfo = None

    def run(self):
        rng = np.random.default_rng(self.seed)
        for t in range(self.trials):
            rows, grp_off = draw_ladder(len(self.g.g.positions), self.levels, rng, self.pool)
            self.markers = grp_off[1:].tolist()
            score, ninfo = self.g.sim_counts(grp_off, self.err_rate, self.seed + t, self.acc_ix, rows)
            self.score, self.ninfo = np.cumsum(score, axis=0, dtype=np.int32), np.cumsum(ninfo, axis=0, dtype=np.int32)
            self.reports.append([level_report(self.score[i], self.ninfo[i], self.lr_thres) for i in range(len(self.levels))])
        return self

    def summary(self):
        n_lev, names = len(self.levels), [str(s) for s in self.names]
        correct = np.array([[r["correct"] for r in trial] for trial in self.reports])        # [trial, level, accession]
        unique = np.array([[r["unique"] for r in trial] for trial in self.reports])
        always = unique.all(axis=0)                                                         # [level, accession]
        first = [next((self.levels[i] for i in range(n_lev) if always[i, a]), None) for a in range(len(names))]
        confused = {}
        for t, trial in enumerate(self.reports):
            with np.errstate(invalid="ignore"):
                a, b = np.nonzero(trial[-1]["lrt"] < self.lr_thres)
            for i, j in zip(a.tolist(), b.tolist()):
                if i != j:
                    confused.setdefault((i, j), []).append(t)
        return dict(levels=self.levels, n_markers=self.markers, trials=self.trials, err_rate=self.err_rate, seed=self.seed, lr_thres=self.lr_thres,
                    accessions=len(names), candidate_rows=int(self.n_rows),
                    fraction_correct=[float(correct[:, i].mean()) for i in range(n_lev)],
                    fraction_unique=[float(unique[:, i].mean()) for i in range(n_lev)],
                    unique_from_level=dict(zip(names, first)),
                    never_unique=[nm for nm, f in zip(names, first) if f is None],
                    confused_at_largest_level=[dict(sample=names[i], taken_for=names[j], trials=ts) for (i, j), ts in sorted(confused.items())])

    def write(self, prefix):
        names = [str(s) for s in self.names]
        with open(prefix + ".power.tsv", "w") as out:
            out.write("trial\tlevel\tn_markers\taccession\tn_sites\tscore_self\tcorrect\tn_ambiguous\tunique\tbest_other\tbest_other_ratio\n")
            for t, trial in enumerate(self.reports):
                for lev, m, r in zip(self.levels, self.markers, trial):
                    for a, nm in enumerate(names):
                        other = names[r["best_other"][a]] if r["best_other"][a] >= 0 else "NA"
                        out.write("%d\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%s\t%r\n" % (t, lev, m, nm, r["n_sites"][a], r["score_self"][a], r["correct"][a],
                                                                                 r["n_ambiguous"][a], r["unique"][a], other, float(r["best_other_ratio"][a])))
        stats = self.summary()
        with open(prefix + ".power.json", "w") as out:
            json.dump(stats, out, indent=1)
        np.savez(prefix + ".power.npz", accessions=np.asarray(names).astype("U"), levels=np.asarray(self.levels, dtype=np.int64),
                 n_markers=np.asarray(self.markers, dtype=np.int64), score=self.score, ninfo=self.ninfo)
        return stats


def potatoPower(args):
    g = snp_genotype.Genotype(args['hdf5File'], args.get('hdf5accFile'))
    acc_ix, _ = _select.accessions_of(g, args)
    # --sites: any site list (chr, pos), e.g. the <prefix>.markers.tsv of the markers command
    snp_ix = _select.rows_of(g, args) if args.get('bed') or args.get('sitesFile') else None
    study = Power(g, parse_levels(args['levels']), args.get('err_rate', 0.001), args.get('trials', 3), args.get('seed', 1),
                  args.get('lr_thres', LR_THRES), acc_ix, snp_ix)
    log.info("power of %d accessions, levels %s, %d trials", len(study.names), study.levels, study.trials)
    stats = study.run().write(args['outFile'])
    log.info("unique at the largest level: %.3f", stats["fraction_unique"][-1])
    return stats
