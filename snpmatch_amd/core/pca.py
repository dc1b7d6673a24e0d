"""
``snpmatch pca``: the population structure of the database -- the genotype relationship matrix (GRM) of its accessions, its principal
components and the SNP loadings -- and, with ``-i``, samples projected onto those axes: when ``inbred`` reports that a sample matches
no accession, this says which part of the collection it belongs to.  The end of the curation chain ``sitestats`` (MAF, missingness)
-> ``ld`` (pruning) -> ``kinship`` (duplicates): hand it ``--sites x.pruned.tsv``.  The reference has no such command
(``calc_kinship_mat`` is the count form ``kinship`` serves); the files are this package's own.

The rows.  Of the selected DB rows (all, ``--bed`` or ``--sites``) a row is used when, among the analysed accessions, it has no
"other" call (not biallelic), at least one call, a minor allele frequency >= ``--min_maf`` and > 0, and a missing fraction <=
``--max_missing`` (``standardise``; the counts are the exact ones of ``Genotype.site_counts``).  With dosage 0 / 2 / 1 for ref /
alt / het and ``p`` the alt frequency, a call becomes ``(dosage - 2 p) / sqrt(2 p (1 - p))`` -- the standardisation of Patterson
et al. 2006 / Price et al. 2006 -- and a missing call 0, i.e. the row's mean.  ``Z`` [R rows, n accessions] is that matrix.

The matrix.  ``gram = Z' Z`` is made on the device in fp64 (``Genotype.gram`` -> ``engine.gram`` -> ``snpm_panel_gram``), ``G = gram
/ R`` is the GRM, ``numpy.linalg.eigh`` decomposes it on the host (n is about a thousand), the raw loadings ``Z V`` are one more
device call (``Genotype.loadings``).  A component's sign is fixed: its entry of largest magnitude is positive.

Projection.  A sample's hard calls at the used rows its file has records for (the matched rows ``m``) are standardised with the
PANEL's ``p``; a record without a call is the mean, as in the panel.  ``coord_c = (R / |m|) sum_{s in m} t(s) load[s][c] / (R
lambda_c)``: a panel accession put through it with every row matched lands on its own eigenvector entry.  A sample that was NOT part
of the decomposition lands shrunk towards the origin -- the known shrinkage of PCA projection (Lee et al. 2010), stronger for the
later components and for few accessions; no correction is applied, so read a projected sample against the clusters, not against a
single accession, and judge it by its ``n_sites``.

  <prefix>.pca.tsv         accession, population (with --pops), PC1 .. PCk: the eigenvector entries
  <prefix>.pca.npz         accessions, populations, eigenvalues, explained, eigenvectors [n, k], chr / pos of the rows used, p and the
                           class table of those rows, loadings [R, k] (raw: Z V), grm with --keep_grm
  <prefix>.pca.json        the settings, rows selected / used / dropped per rule, trace, eigenvalues, explained, and per component
                           the ten rows of largest absolute loading
  <prefix>.projection.tsv  with -i: sample, n_sites, PC1 .. PCk, the three nearest accessions by Euclidean distance over the k
                           coordinates, with --pops the population of the nearest centroid
"""
import json
import logging

import numpy as np

from . import _select, sitestats, snp_genotype

log = logging.getLogger(__name__)

MAX_COMPONENTS = 32
NO_CLASS = 0xFF
DROP_RULES = ("other_code", "no_call", "maf", "missing")
TOP_LOADINGS = 10


def standardise(counts, n_listed, min_maf=0.05, max_missing=0.1):
    """``counts`` int [rows, 4]: c0, c1, c2, ninfo of every row among the ``n_listed`` analysed accessions (one group of
    ``Genotype.site_counts``).  With n = c0 + c1 + c2 and p = (2 c1 + c2) / (2 n) a row is kept when ninfo == n (no "other" code),
    n > 0, min(p, 1 - p) >= min_maf and > 0, and (n_listed - n) / n_listed <= max_missing; the two fractions are single divisions
    of integers (the minor allele count over 2 n, the missing calls over n_listed), so a row exactly at a threshold is kept.
    Returns (keep bool [rows], tab fp64 [rows, 4], p fp64 [rows], dropped): the table of a kept row is ((0 - 2p) r, (2 - 2p) r,
    (1 - 2p) r, 0) with r = 1 / sqrt(2 p (1 - p)), of a dropped row zeros; p is nan where n == 0; ``dropped`` counts the rows by the
    FIRST rule of DROP_RULES they fail."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1, 4)
    n_listed = int(n_listed)
    n = c[:, 0] + c[:, 1] + c[:, 2]
    alt = 2 * c[:, 1] + c[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        p = alt.astype(np.float64) / (2 * n).astype(np.float64)
        maf = np.minimum(alt, 2 * n - alt).astype(np.float64) / (2 * n).astype(np.float64)
    missing = (n_listed - n).astype(np.float64) / float(max(n_listed, 1))
    fails = [c[:, 3] != n, n == 0, ~((maf >= float(min_maf)) & (maf > 0)), ~(missing <= float(max_missing))]
    keep = np.ones(len(c), dtype=bool)
    dropped = {}
    for name, bad in zip(DROP_RULES, fails):
        dropped[name] = int(np.count_nonzero(keep & bad))
        keep &= ~bad
    tab = np.zeros((len(c), 4), dtype=np.float64)
    pk = p[keep]
    r = 1.0 / np.sqrt(2.0 * pk * (1.0 - pk))
    tab[keep, 0], tab[keep, 1], tab[keep, 2] = (0.0 - 2.0 * pk) * r, (2.0 - 2.0 * pk) * r, (1.0 - 2.0 * pk) * r
    return keep, tab, p, dropped


def decompose(gram, n_rows, k):
    """``G = gram / n_rows`` and its ``k`` largest eigenpairs (``numpy.linalg.eigh``): (eigenvalues [k] descending, eigenvectors
    [n, k] of unit length, explained [k] = eigenvalue / trace(G), trace).  The sign of a vector is fixed so that its entry of largest
    absolute value is positive, the lowest index on a tie."""
    G = np.asarray(gram, dtype=np.float64) / float(n_rows)
    n = len(G)
    if not 1 <= int(k) <= n:
        raise ValueError("components must be 1 .. %d, got %d" % (n, k))
    w, v = np.linalg.eigh(G)
    order = np.argsort(-w, kind="stable")[:int(k)]
    w, v = w[order], v[:, order].copy()
    for c in range(v.shape[1]):
        if v[np.argmax(np.abs(v[:, c])), c] < 0:
            v[:, c] = -v[:, c]
    trace = float(np.trace(G))
    with np.errstate(divide="ignore", invalid="ignore"):
        explained = w / trace
    return w, v, explained, trace


def project(classes, tab_rows, load, eigenvalues, R, matched=None):
    """Coordinates of samples on the axes of a decomposition.  ``classes`` uint8 [n_samples, R]: the hard call of every sample at
    every used row (0 ref, 1 alt, 2 het, NO_CLASS none); ``tab_rows`` fp64 [R, 4] the class table of those rows; ``load`` fp64
    [R, k] the raw loadings Z V; ``eigenvalues`` [k] of G = Z' Z / R; ``matched`` bool [n_samples, R] or [R]: the rows the sample
    has a record for (default: all) -- a matched row without a call counts as the row's mean (value 0), like a missing call of the
    panel.  ``coord_c = (R / |m|) sum_{s in m} t(s) load[s][c] / (R lambda_c)``.  Returns (coord fp64 [n_samples, k], nan for a
    sample without a called matched row; n_sites int64 [n_samples], the matched rows with a call)."""
    classes = np.asarray(classes, dtype=np.uint8).reshape(-1, int(R))
    tab_rows, load = np.asarray(tab_rows, dtype=np.float64), np.asarray(load, dtype=np.float64)
    lam = np.asarray(eigenvalues, dtype=np.float64)
    matched = np.ones(classes.shape, dtype=bool) if matched is None else np.broadcast_to(np.asarray(matched, dtype=bool), classes.shape)
    called = matched & (classes <= 2)
    t = np.where(called, tab_rows[np.arange(int(R))[None, :], np.minimum(classes, 3)], 0.0)
    n_matched, n_sites = matched.sum(axis=1).astype(np.int64), called.sum(axis=1).astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        coord = (t @ load) / (n_matched[:, None].astype(np.float64) * lam[None, :])
    coord[n_sites == 0] = np.nan
    return coord, n_sites


def nearest(coord, ref, count=3):
    """indices of the ``count`` rows of ``ref`` nearest to ``coord`` (Euclidean, the lower index on a tie) and their distances"""
    d = np.sqrt(((np.asarray(ref) - np.asarray(coord)[None, :]) ** 2).sum(axis=1))
    order = np.argsort(d, kind="stable")[:count]
    return order, d[order]


def centroids(vec, pop_of, pop_names):
    return np.stack([vec[[i for i, q in enumerate(pop_of) if q == name]].mean(axis=0) for name in pop_names])


def top_loadings(load, chrs, pos, count=TOP_LOADINGS):
    out = []
    for c in range(load.shape[1]):
        order = np.argsort(-np.abs(load[:, c]), kind="stable")[:count]
        out.append([{"chr": str(chrs[r]), "pos": int(pos[r]), "loading": float(load[r, c])} for r in order.tolist()])
    return out


def analysed_accessions(g, args):
    """(names, acc_ix or None, population of each or None, population names) from --pops, -a or neither"""
    pop_names, pops, _ = sitestats.populations_of(g, args)
    if pops is None:
        return [str(a) for a in np.asarray(g.accessions).tolist()], None, None, []
    acc_ix = np.concatenate([pops[name] for name in pop_names]).astype(np.int64)
    if len(set(acc_ix.tolist())) != len(acc_ix):
        raise ValueError("an accession is listed twice (%s)" % (args.get('popFile') or args.get('accFile')))
    names = [str(a) for a in np.asarray(g.accessions)[acc_ix].tolist()]
    if args.get('popFile'):
        return names, acc_ix, [name for name in pop_names for _ in range(len(pops[name]))], pop_names
    return names, acc_ix, None, []


def write_outputs(prefix, names, pop_of, res, settings, keep_grm=False):
    k = res["vec"].shape[1]
    with open(prefix + ".pca.tsv", "w") as out:
        out.write("accession" + ("\tpopulation" if pop_of else "") + "".join("\tPC%d" % (c + 1) for c in range(k)) + "\n")
        for i, name in enumerate(names):
            out.write(name + ("\t" + pop_of[i] if pop_of else "") + "".join("\t%r" % float(x) for x in res["vec"][i]) + "\n")
    extra = {"grm": res["gram"] / float(res["R"])} if keep_grm else {}
    np.savez(prefix + ".pca.npz", accessions=np.asarray(names).astype("U"), populations=np.asarray(pop_of if pop_of else []).astype("U"),
             eigenvalues=res["eigenvalues"], explained=res["explained"], eigenvectors=res["vec"], chr=res["chr"], pos=res["pos"], p=res["p"],
             table=res["tab"], loadings=res["load"], **extra)
    stats = dict(settings)
    stats.update(accessions=len(names), rows_selected=int(res["selected"]), rows_used=int(res["R"]), rows_dropped=res["dropped"], trace=res["trace"],
                 eigenvalues=[float(x) for x in res["eigenvalues"]], explained=[float(x) for x in res["explained"]],
                 top_loadings=top_loadings(res["load"], res["chr"], res["pos"]))
    with open(prefix + ".pca.json", "w") as out:
        json.dump(stats, out, indent=1, sort_keys=True)
        out.write("\n")
    return stats


def analyse(g, acc_ix, n_acc, rows, min_maf, max_missing, k):
    """the two device calls around the host's decomposition: a dict of R, the rows used, p, tab, gram, eigenvalues, explained, vec, load"""
    counts = g.site_counts(acc_ix, rows)[0]
    keep, tab, p, dropped = standardise(counts, n_acc, min_maf, max_missing)
    used = np.asarray(rows, dtype=np.int64)[keep]
    R = int(len(used))
    if R == 0:
        raise ValueError("no row is left after the filters: %d selected, dropped %s" % (len(rows), ", ".join("%s %d" % kv for kv in dropped.items())))
    tab = np.ascontiguousarray(tab[keep])
    gram = g.gram(tab, acc_ix, used)
    w, vec, explained, trace = decompose(gram, R, k)
    load = g.loadings(tab, vec, acc_ix, used)
    return {"selected": len(rows), "R": R, "rows": used, "p": p[keep], "tab": tab, "gram": gram, "eigenvalues": w, "explained": explained, "vec": vec,
            "load": load, "trace": trace, "dropped": dropped}


def project_samples(g, res, samples, chrs, pos, gt):
    """(coord, n_sites) of every sample column of ``gt`` at the used rows its records match"""
    db_rows, rec_rows = g.get_positions_idxs(chrs, pos)
    db_rows, rec_rows = np.asarray(db_rows, dtype=np.int64), np.asarray(rec_rows, dtype=np.int64)
    where = np.full(len(g.g.positions), -1, dtype=np.int64)
    where[res["rows"]] = np.arange(res["R"])
    at = where[db_rows]
    hit = at >= 0
    matched = np.zeros(res["R"], dtype=bool)
    matched[at[hit]] = True
    classes = np.full((len(samples), res["R"]), NO_CLASS, dtype=np.uint8)
    for s in range(len(samples)):
        classes[s, at[hit]] = _select.hard_classes(gt[:, s])[rec_rows[hit]]
    return project(classes, res["tab"], res["load"], res["eigenvalues"], res["R"], matched)


def write_projection(prefix, samples, coord, n_sites, names, vec, pop_of, pop_names):
    k = vec.shape[1]
    cents = centroids(vec, pop_of, pop_names) if pop_of else None
    with open(prefix + ".projection.tsv", "w") as out:
        out.write("sample\tn_sites" + "".join("\tPC%d" % (c + 1) for c in range(k)) + "\tnearest_1\tnearest_2\tnearest_3" + ("\tpopulation" if pop_of else "") + "\n")
        for s, name in enumerate(samples):
            if n_sites[s] == 0:
                out.write("%s\t0" % name + "\tNA" * (k + 3 + (1 if pop_of else 0)) + "\n")
                log.warning("sample %s has no matched row among the rows used: not projected", name)
                continue
            near, _ = nearest(coord[s], vec, 3)
            near = [names[i] for i in near.tolist()] + ["NA"] * (3 - len(near))
            line = "%s\t%d" % (name, n_sites[s]) + "".join("\t%r" % float(x) for x in coord[s]) + "".join("\t" + a for a in near)
            if pop_of:
                line += "\t" + pop_names[int(nearest(coord[s], cents, 1)[0][0])]
            out.write(line + "\n")


def potatoPCA(args):
    """entry point of ``snpmatch pca``"""
    _select.one_row_option(args)
    given = lambda key, default: default if args.get(key) is None else args[key]      # noqa: E731
    min_maf, max_missing, k = float(given('min_maf', 0.05)), float(given('max_missing', 0.1)), int(given('components', 10))
    if not 0.0 <= min_maf <= 0.5:
        raise ValueError("--min_maf must be 0 .. 0.5, got %r" % min_maf)
    if not 0.0 <= max_missing <= 1.0:
        raise ValueError("--max_missing must be 0 .. 1, got %r" % max_missing)
    g = snp_genotype.Genotype(args['hdf5File'], args.get('hdf5accFile'))
    names, acc_ix, pop_of, pop_names = analysed_accessions(g, args)
    if len(names) < 2:
        raise ValueError("a principal component analysis needs at least 2 accessions, got %d" % len(names))
    if not 1 <= k <= min(MAX_COMPONENTS, len(names)):
        raise ValueError("--components must be 1 .. %d (min(%d, accessions)), got %d" % (min(MAX_COMPONENTS, len(names)), MAX_COMPONENTS, k))
    rows = _select.rows_of(g, args)
    log.info("pca: %d accessions, %d selected rows, %d components", len(names), len(rows), k)
    res = analyse(g, acc_ix, len(names), rows, min_maf, max_missing, k)
    res["chr"], res["pos"] = _select.row_chromosomes(g, res["rows"]), np.asarray(g.g.positions)[res["rows"]].astype(np.int64)
    settings = {"min_maf": min_maf, "max_missing": max_missing, "components": k, "populations": pop_names, "bed": args.get('bed'), "sites": args.get('sitesFile')}
    stats = write_outputs(args['outFile'], names, pop_of, res, settings, bool(args.get('keep_grm')))
    log.info("%d of %d rows used; PC1 %.3f, PC2 %.3f of the trace", res["R"], len(rows), stats["explained"][0], stats["explained"][1] if k > 1 else 0.0)
    if args.get('inFile'):
        samples, chrs, pos, gt = _select.read_samples(args['inFile'], args.get('logDebug', False))
        coord, n_sites = project_samples(g, res, samples, chrs, pos, gt)
        write_projection(args['outFile'], samples, coord, n_sites, names, res["vec"], pop_of, pop_names)
        stats["projected"] = int(np.count_nonzero(n_sites > 0))
    return stats
