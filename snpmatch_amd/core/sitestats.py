"""
``snpmatch sitestats``: per-SNP allele counts, allele frequencies and missingness of a database, in the whole panel or per
subpopulation, counted on the resident panel in one streaming pass however many populations are asked for
(``Genotype.site_counts`` -> ``engine.site_counts`` -> ``snpm_panel_site_counts``) -- what a curator needs to choose the markers
worth genotyping on: the MAF and missingness filters of a marker set, per-population frequencies of admixed material.

The reference has the method (``Genotype.get_af_snps``, core/snp_genotype.py:119-175) but no such command: the three files and the
thresholds below are this package's own.

  <prefix>.sitestats.npz   chr, pos (of the rows), populations (names), n_listed (accessions per population), counts int32
                           [G, n, 4] (c0, c1, c2, ninfo), af and maf fp64 [G, n] (alt frequency (2 c1 + c2) / (2 ninfo) and its
                           fold; nan where ninfo <= --min_informative), nind int64 [G, n]
  <prefix>.sitestats.json  per population: rows, rows without an informative accession, rows monomorphic among the informative
                           accessions, rows the reference's ``_polarize_snps`` would flip (alt in more than half of the listed
                           accessions), and a histogram of maf in 10 bins over [0, 0.5]
  <prefix>.sites.tsv       only with --min_maf / --max_missing: chr, pos and per population maf and missing fraction
                           (1 - ninfo / listed accessions) of the rows that pass in EVERY population (a nan maf does not pass)
"""
import json
import logging

import numpy as np

from . import _select, snp_genotype
from ._select import read_populations, row_chromosomes  # noqa: F401  (the names tests and tools import)

log = logging.getLogger(__name__)


def populations_of(g, args):
    """(names, index arrays or None, accessions listed per population) from --pops, -a or neither (all accessions)"""
    if args.get('popFile') and args.get('accFile'):
        raise ValueError("give either -a / --accessions or --pops, not both")
    if args.get('popFile'):
        pairs = read_populations(args['popFile'])
        found = _select.indices_of(g, [a for a, _ in pairs], "population file", args['popFile'])
        pops = {}
        for (_, pop), ix in zip(pairs, found):
            pops.setdefault(pop, []).append(ix)
        names = list(pops)
        return names, {name: np.array(pops[name], dtype=np.int64) for name in names}, [len(pops[name]) for name in names]
    acc_ix, _ = _select.accessions_of(g, args)
    if acc_ix is not None:
        return ["listed"], {"listed": acc_ix}, [len(acc_ix)]
    return ["all"], None, [len(g.accessions)]


def summary(names, n_listed, counts, maf):
    out = {}
    for k, name in enumerate(names):
        c = counts[k].astype(np.int64)
        ninfo = c[:, 3]
        other = ninfo - c[:, 0] - c[:, 1] - c[:, 2]
        top = np.maximum(np.maximum(c[:, 0], c[:, 1]), np.maximum(c[:, 2], other))
        known = maf[k][~np.isnan(maf[k])]
        out[name] = {
            "accessions": int(n_listed[k]),
            "rows": int(len(c)),
            "no_informative": int(np.count_nonzero(ninfo == 0)),
            "monomorphic": int(np.count_nonzero((ninfo > 0) & (top == ninfo))),
            "polarised": int(np.count_nonzero(c[:, 1] > float(n_listed[k]) / 2)),
            "maf_histogram": [int(v) for v in np.histogram(known, bins=10, range=(0.0, 0.5))[0]],
        }
    return out


def passing_rows(n_listed, counts, maf, min_maf=None, max_missing=None):
    """bool [n]: rows that pass the thresholds in EVERY population; (keep, missing fraction [G, n])"""
    listed = np.maximum(np.asarray(n_listed, dtype=np.float64), 1.0)[:, None]
    missing = 1.0 - counts[:, :, 3].astype(np.float64) / listed
    keep = np.ones(counts.shape[1], dtype=bool)
    if min_maf is not None:
        with np.errstate(invalid="ignore"):
            keep &= (maf >= float(min_maf)).all(axis=0)              # a nan maf compares false
    if max_missing is not None:
        keep &= (missing <= float(max_missing)).all(axis=0)
    return keep, missing


def write_outputs(prefix, names, n_listed, chrs, pos, counts, min_informative=0, min_maf=None, max_missing=None):
    af = snp_genotype.af_from_counts(counts, min_informative, 1, False)
    maf = snp_genotype.af_from_counts(counts, min_informative, 1, True)
    np.savez(prefix + ".sitestats.npz", chr=chrs, pos=pos, populations=np.asarray(names).astype("U"), n_listed=np.asarray(n_listed, dtype=np.int64),
             counts=counts, af=af, maf=maf, nind=counts[:, :, 3].astype(np.int64))
    stats = summary(names, n_listed, counts, maf)
    with open(prefix + ".sitestats.json", "w") as out:
        json.dump({"populations": names, "min_informative": int(min_informative), "stats": stats}, out, indent=1, sort_keys=True)
        out.write("\n")
    n_pass = None
    if min_maf is not None or max_missing is not None:
        keep, missing = passing_rows(n_listed, counts, maf, min_maf, max_missing)
        with open(prefix + ".sites.tsv", "w") as out:
            out.write("chr\tpos" + "".join("\tmaf_%s\tmissing_%s" % (n, n) for n in names) + "\n")
            for r in np.flatnonzero(keep).tolist():
                out.write("%s\t%d" % (chrs[r], pos[r]) + "".join("\t%r\t%r" % (float(maf[k, r]), float(missing[k, r])) for k in range(len(names))) + "\n")
        n_pass = int(keep.sum())
    return stats, n_pass


def potatoSiteStats(args):
    g = snp_genotype.Genotype(args['hdf5File'], args.get('hdf5accFile'))
    names, pops, n_listed = populations_of(g, args)
    rows = _select.rows_of(g, args)
    snp_ix = rows if args.get('bed') else None
    log.info("site statistics of %d population(s) over %d rows", len(names), len(rows))
    counts = g.site_counts(pops, snp_ix)
    pos = np.asarray(g.g.positions)[rows].astype(np.int64)
    stats, n_pass = write_outputs(args['outFile'], names, n_listed, row_chromosomes(g, rows), pos, counts, args.get('min_informative', 0) or 0,
                                  args.get('min_maf'), args.get('max_missing'))
    if n_pass is not None:
        log.info("%d of %d rows pass in every population", n_pass, len(rows))
    return stats
