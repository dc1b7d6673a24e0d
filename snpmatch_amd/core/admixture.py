"""
``snpmatch admixture``: the ancestry proportions of every accession of the database under the model of STRUCTURE (Pritchard et al.
2000), FRAPPE (Tang et al. 2005) and ADMIXTURE (Alexander et al. 2009) -- every accession a mixture ``q`` of K ancestral populations,
every population with its own alt frequency ``f`` at every SNP -- fitted by joint EM on the device, and, with ``-i``, the proportions
of samples under the fitted frequencies: a sample that matches no accession is "0.7 of cluster 2 and 0.3 of cluster 5".  It writes the
two-column population file that ``sitestats``, ``ld`` and ``pca`` take as ``--pops``.  After the curation chain ``sitestats`` -> ``ld``
-> ``kinship`` -> ``pca``: hand it ``--sites x.pruned.tsv``.  The reference has no such command; the files are this package's own.

The model is a DIPLOID one: a call with dosage g (0 ref, 2 alt, 1 het) has likelihood ``p^g (1 - p)^(2 - g)`` with ``p = sum_k q_k
f_k``, which assumes Hardy-Weinberg proportions within every ancestral population.  Selfing lines violate that assumption: their
calls are almost all homozygous.  For homozygous calls the diploid log-likelihood is exactly TWICE the haploid one (one allele per
call), and the EM updates are the same -- the factor 2 cancels in both ratios -- so the estimates are those of the haploid model and
only the likelihood (and anything derived from its absolute value) is doubled; the rare het calls enter as one allele of each kind.

The rows.  Exactly those of ``pca``: of the selected DB rows (all, ``--bed`` or ``--sites``) a row is used when ``pca.standardise``
keeps it -- no "other" call, at least one call, minor allele frequency >= ``--min_maf`` and > 0, missing fraction <= ``--max_missing``
among the analysed accessions.

The fit.  A restart r starts from ``numpy.random.default_rng(seed + r)``: Q from ``dirichlet(ones(K))`` per accession, F from
``uniform(0.1, 0.9)``.  Iterations run in device calls of 20 (``Genotype.admix`` -> ``engine.admix`` -> ``snpm_panel_admix``) until
``ll_t - ll_{t-1} < tol |ll_t|`` for a t inside the block, or ``--max_iter``; the final likelihood is one evaluating call; the restart
with the highest final likelihood wins.  Components are put in CANONICAL ORDER, by descending ``sum_i q_ik`` (the lower index on a
tie), so the files do not depend on label switching.

Samples (``-i``): the hard calls of every sample at the used rows its file has records for; EM on q alone with F fixed, on the host
(R x K per iteration).

  <prefix>.admixture.Q.tsv     accession, population (with --pops), Q1 .. QK, cluster = the component of the largest proportion
  <prefix>.admixture.pops.tsv  accession and K<cluster>: the --pops file of sitestats / ld / pca
  <prefix>.admixture.npz       accessions, Q [n, K], F [R, K], chr / pos of the rows used, p, the likelihood trace, seeds
  <prefix>.admixture.json      the settings, rows selected / used / dropped per rule, iterations, converged, the likelihood of every
                               restart, cluster sizes, with --pops the population x cluster table
  <prefix>.ancestry.tsv        with -i: sample, n_sites, Q1 .. QK, cluster
"""
import json
import logging

import numpy as np

from . import _select, pca, snp_genotype

log = logging.getLogger(__name__)

MAX_K = 16
EPS = 1e-6
BLOCK = 20                      # iterations per device call
NO_CLASS = 0xFF


def random_start(seed, n, R, K):
    """(Q [n, K], F [R, K]) of a restart: ``default_rng(seed)``, Q from dirichlet(ones(K)) per accession, then F from uniform(0.1, 0.9)"""
    rng = np.random.default_rng(int(seed))
    return rng.dirichlet(np.ones(int(K)), size=int(n)), rng.uniform(0.1, 0.9, size=(int(R), int(K)))


def canonical_order(Q):
    """the permutation of the components by descending ``sum_i q_ik``, the lower index on a tie"""
    return np.argsort(-np.asarray(Q, dtype=np.float64).sum(axis=0), kind="stable")


def run_em(admix, Q, F, max_iter=2000, tol=1e-7, block=BLOCK):
    """``admix(Q, F, n_iter, update_q, update_f) -> (Q, F, loglik)`` in calls of ``block`` iterations until ``ll_t - ll_{t-1} < tol
    |ll_t|`` for a t inside a block (the block is finished: Q and F are those at its end) or ``max_iter`` iterations; then one
    evaluating call.  Returns (Q, F, trace, final likelihood, converged): ``trace[t]`` the likelihood at the start of iteration t."""
    trace = []
    converged = False
    while len(trace) < int(max_iter) and not converged:
        n = min(int(block), int(max_iter) - len(trace))
        Q, F, ll = admix(Q, F, n, True, True)
        first = len(trace)
        trace.extend(float(x) for x in ll)
        for t in range(max(first, 1), len(trace)):
            if trace[t] - trace[t - 1] < float(tol) * abs(trace[t]):
                converged = True
    final = float(admix(Q, F, 1, False, False)[2][0])
    return Q, F, np.array(trace), final, converged


def fit(admix, n, R, K, seed=1, restarts=1, max_iter=2000, tol=1e-7):
    """the best of ``restarts`` runs of ``run_em`` from ``random_start(seed + r)``, its components in canonical order: a dict of Q, F,
    trace, loglik, converged, iterations, restart, and per restart the final likelihood, iterations and converged"""
    best, runs = None, []
    for r in range(int(restarts)):
        Q, F = random_start(int(seed) + r, n, R, K)
        Q, F, trace, final, converged = run_em(admix, Q, F, max_iter, tol)
        runs.append({"seed": int(seed) + r, "loglik": final, "iterations": int(len(trace)), "converged": bool(converged)})
        log.info("restart %d (seed %d): %d iterations, log-likelihood %.6f%s", r, int(seed) + r, len(trace), final, "" if converged else " (not converged)")
        if best is None or final > best["loglik"]:
            best = {"Q": Q, "F": F, "trace": trace, "loglik": final, "converged": bool(converged), "iterations": int(len(trace)), "restart": r}
    order = canonical_order(best["Q"])
    best["Q"], best["F"] = np.ascontiguousarray(best["Q"][:, order]), np.ascontiguousarray(best["F"][:, order])
    best["runs"] = runs
    return best


def sample_ancestry(classes, F, max_iter=2000, tol=1e-7):
    """EM on q alone with F [R, K] fixed, for every sample of ``classes`` uint8 [n_samples, R] (0 ref, 1 alt, 2 het, anything else no
    call), from q = 1 / K: per iteration ``q'_k = q_k c_k / sum_k q_k c_k`` with ``c_k = sum_s u f_sk + v (1 - f_sk)``, u = g / p, v =
    (2 - g) / pbar over the called rows, until the likelihood gains less than ``tol`` of itself.  Returns (q fp64 [n_samples, K], nan
    for a sample without a call; n_sites int64 [n_samples])."""
    F = np.asarray(F, dtype=np.float64)
    R, K = F.shape
    classes = np.asarray(classes, dtype=np.uint8).reshape(-1, R)
    out = np.full((len(classes), K), np.nan)
    n_sites = np.zeros(len(classes), dtype=np.int64)
    for s, cls in enumerate(classes):
        at = np.flatnonzero(cls <= 2)
        n_sites[s] = len(at)
        if not len(at):
            continue
        g = np.array([0.0, 2.0, 1.0])[cls[at]]
        f, fb = F[at], 1.0 - F[at]
        q = np.full(K, 1.0 / K)
        last = -np.inf
        for _ in range(int(max_iter)):
            p, pbar = f @ q, fb @ q
            ll = float(np.sum(g * np.log(p) + (2.0 - g) * np.log(pbar)))
            w = q * ((g / p) @ f + ((2.0 - g) / pbar) @ fb)
            q = w / w.sum()
            if ll - last < float(tol) * abs(ll):
                break
            last = ll
        out[s] = q
    return out, n_sites


def sample_classes(g, used, samples, chrs, pos, gt):
    """uint8 [n_samples, R]: the hard call of every sample column of ``gt`` at the used rows its records match, NO_CLASS elsewhere"""
    db_rows, rec_rows = g.get_positions_idxs(chrs, pos)
    db_rows, rec_rows = np.asarray(db_rows, dtype=np.int64), np.asarray(rec_rows, dtype=np.int64)
    where = np.full(len(g.g.positions), -1, dtype=np.int64)
    where[used] = np.arange(len(used))
    at = where[db_rows]
    hit = at >= 0
    classes = np.full((len(samples), len(used)), NO_CLASS, dtype=np.uint8)
    for s in range(len(samples)):
        classes[s, at[hit]] = _select.hard_classes(gt[:, s])[rec_rows[hit]]
    return classes


def write_outputs(prefix, names, pop_of, pop_names, res, settings):
    Q, K = res["Q"], res["Q"].shape[1]
    cluster = np.argmax(Q, axis=1)
    with open(prefix + ".admixture.Q.tsv", "w") as out:
        out.write("accession" + ("\tpopulation" if pop_of else "") + "".join("\tQ%d" % (k + 1) for k in range(K)) + "\tcluster\n")
        for i, name in enumerate(names):
            out.write(name + ("\t" + pop_of[i] if pop_of else "") + "".join("\t%r" % float(x) for x in Q[i]) + "\tK%d\n" % (cluster[i] + 1))
    with open(prefix + ".admixture.pops.tsv", "w") as out:
        out.write("# accession\tcluster (K = %d)\n" % K)
        for i, name in enumerate(names):
            out.write("%s\tK%d\n" % (name, cluster[i] + 1))
    np.savez(prefix + ".admixture.npz", accessions=np.asarray(names).astype("U"), populations=np.asarray(pop_of if pop_of else []).astype("U"), Q=Q, F=res["F"],
             chr=res["chr"], pos=res["pos"], p=res["p"], trace=res["trace"], seeds=np.array([r["seed"] for r in res["runs"]], dtype=np.int64))
    stats = dict(settings)
    stats.update(accessions=len(names), rows_selected=int(res["selected"]), rows_used=int(res["R"]), rows_dropped=res["dropped"], iterations=res["iterations"],
                 converged=res["converged"], loglik=res["loglik"], restart=res["restart"], restarts=res["runs"],
                 cluster_sizes={"K%d" % (k + 1): int(np.count_nonzero(cluster == k)) for k in range(K)})
    if pop_of:
        stats["population_by_cluster"] = {name: {"K%d" % (k + 1): int(sum(1 for i, q in enumerate(pop_of) if q == name and cluster[i] == k)) for k in range(K)}
                                          for name in pop_names}
    with open(prefix + ".admixture.json", "w") as out:
        json.dump(stats, out, indent=1, sort_keys=True)
        out.write("\n")
    return stats


def write_ancestry(prefix, samples, q, n_sites):
    K = q.shape[1]
    with open(prefix + ".ancestry.tsv", "w") as out:
        out.write("sample\tn_sites" + "".join("\tQ%d" % (k + 1) for k in range(K)) + "\tcluster\n")
        for s, name in enumerate(samples):
            if n_sites[s] == 0:
                out.write("%s\t0" % name + "\tNA" * (K + 1) + "\n")
                log.warning("sample %s has no called row among the rows used: no ancestry", name)
                continue
            out.write("%s\t%d" % (name, n_sites[s]) + "".join("\t%r" % float(x) for x in q[s]) + "\tK%d\n" % (int(np.argmax(q[s])) + 1))


def analyse(g, acc_ix, n_acc, rows, min_maf, max_missing, K, seed=1, restarts=1, max_iter=2000, tol=1e-7):
    """the row filter of ``pca`` and the fit: the dict of ``fit`` plus selected, R, rows, p, dropped"""
    counts = g.site_counts(acc_ix, rows)[0]
    keep, _, p, dropped = pca.standardise(counts, n_acc, min_maf, max_missing)
    used = np.asarray(rows, dtype=np.int64)[keep]
    R = int(len(used))
    if R == 0:
        raise ValueError("no row is left after the filters: %d selected, dropped %s" % (len(rows), ", ".join("%s %d" % kv for kv in dropped.items())))
    res = fit(lambda Q, F, n_iter, update_q, update_f: g.admix(Q, F, n_iter, acc_ix, used, update_q, update_f), n_acc, R, K, seed, restarts, max_iter, tol)
    res.update(selected=len(rows), R=R, rows=used, p=p[keep], dropped=dropped)
    return res


def potatoAdmixture(args):
    """entry point of ``snpmatch admixture``"""
    _select.one_row_option(args)
    given = lambda key, default: default if args.get(key) is None else args[key]      # noqa: E731
    min_maf, max_missing, K = float(given('min_maf', 0.05)), float(given('max_missing', 0.1)), int(args['K'])
    seed, restarts, max_iter, tol = int(given('seed', 1)), int(given('restarts', 1)), int(given('max_iter', 2000)), float(given('tol', 1e-7))
    if not 0.0 <= min_maf <= 0.5:
        raise ValueError("--min_maf must be 0 .. 0.5, got %r" % min_maf)
    if not 0.0 <= max_missing <= 1.0:
        raise ValueError("--max_missing must be 0 .. 1, got %r" % max_missing)
    if not 1 <= K <= MAX_K:
        raise ValueError("-K must be 1 .. %d, got %d" % (MAX_K, K))
    if restarts < 1 or max_iter < 1 or not tol >= 0.0:
        raise ValueError("--restarts and --max_iter must be at least 1 and --tol not negative")
    g = snp_genotype.Genotype(args['hdf5File'], args.get('hdf5accFile'))
    names, acc_ix, pop_of, pop_names = pca.analysed_accessions(g, args)
    if len(names) < 2:
        raise ValueError("the admixture model needs at least 2 accessions, got %d" % len(names))
    if K > len(names):
        raise ValueError("-K must not exceed the number of accessions: K = %d, %d accessions" % (K, len(names)))
    rows = _select.rows_of(g, args)
    log.info("admixture: %d accessions, %d selected rows, K = %d", len(names), len(rows), K)
    res = analyse(g, acc_ix, len(names), rows, min_maf, max_missing, K, seed, restarts, max_iter, tol)
    res["chr"], res["pos"] = _select.row_chromosomes(g, res["rows"]), np.asarray(g.g.positions)[res["rows"]].astype(np.int64)
    settings = {"K": K, "min_maf": min_maf, "max_missing": max_missing, "seed": seed, "max_iter": max_iter, "tol": tol, "populations": pop_names,
                "bed": args.get('bed'), "sites": args.get('sitesFile')}
    stats = write_outputs(args['outFile'], names, pop_of, pop_names, res, settings)
    log.info("%d of %d rows used; %d iterations, log-likelihood %.6f; cluster sizes %s", res["R"], len(rows), res["iterations"], res["loglik"], stats["cluster_sizes"])
    if args.get('inFile'):
        samples, chrs, pos, gt = _select.read_samples(args['inFile'], args.get('logDebug', False))
        q, n_sites = sample_ancestry(sample_classes(g, res["rows"], samples, chrs, pos, gt), res["F"], max_iter, tol)
        write_ancestry(args['outFile'], samples, q, n_sites)
        stats["samples_placed"] = int(np.count_nonzero(n_sites > 0))
    return stats
