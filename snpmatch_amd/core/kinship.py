"""
``snpmatch kinship``: relatedness of every pair of accessions of a database, counted on the resident panel in one device call
(``Genotype.kinship_counts`` -> ``engine.kinship_counts`` -> ``snpm_panel_kinship_counts``), and the list of near-identical pairs --
the "indistinguishable lines" that ``inbred`` reports as ambiguous top hits -- that a curator wants before a DB ships.

The reference has the method (``Genotype.kinship_given_snps``, core/snp_genotype.py:256-289) but no such command: the two files and
the two thresholds below are this package's own.

  <prefix>.kinship.npz     accessions, ninfo, same, diff (int32 [n, n]) and kinship = (same - diff) / ninfo (fp64, nan for 0 / 0)
  <prefix>.duplicates.tsv  acc_1, acc_2, same, diff, ninfo, identity, kinship for every pair a < b (in the order of the accession
                           list) with same + diff >= min_sites and identity = same / (same + diff) >= min_identity; sorted by
                           identity (highest first), then by the two names; identity and kinship with ``repr`` precision
"""
import logging

import numpy as np

from . import _select, snp_genotype
from ._select import read_accession_list  # noqa: F401  (the name tests and tools import)

log = logging.getLogger(__name__)

MIN_IDENTITY = 0.99         # default of --min_identity: homozygous identity from which a pair is listed as duplicates
MIN_SITES = 100             # default of --min_sites: rows at which both accessions are homozygous, below which a pair is not judged


def duplicate_pairs(names, ninfo, same, diff, min_identity=MIN_IDENTITY, min_sites=MIN_SITES):
    """rows of the duplicates table: (name_a, name_b, same, diff, ninfo, identity, kinship) for a < b"""
    names = [str(n) for n in names]
    same, diff, ninfo = (np.asarray(m, dtype=np.int64) for m in (same, diff, ninfo))
    hom = same + diff
    a, b = np.triu_indices(len(names), k=1)
    keep = hom[a, b] >= max(int(min_sites), 1)
    a, b = a[keep], b[keep]
    identity = same[a, b] / hom[a, b].astype(np.float64)
    keep = identity >= float(min_identity)
    a, b, identity = a[keep], b[keep], identity[keep]
    kin = snp_genotype.kinship_from_counts(ninfo[a, b], same[a, b], diff[a, b])
    rows = [(names[i], names[j], int(same[i, j]), int(diff[i, j]), int(ninfo[i, j]), float(f), float(k))
            for i, j, f, k in zip(a.tolist(), b.tolist(), identity.tolist(), kin.tolist())]
    rows.sort(key=lambda r: (-r[5], r[0], r[1]))
    return rows


def write_outputs(prefix, names, ninfo, same, diff, min_identity=MIN_IDENTITY, min_sites=MIN_SITES):
    kin = snp_genotype.kinship_from_counts(ninfo, same, diff)
    np.savez(prefix + ".kinship.npz", accessions=np.asarray(names).astype("U"), ninfo=ninfo, same=same, diff=diff, kinship=kin)
    rows = duplicate_pairs(names, ninfo, same, diff, min_identity, min_sites)
    with open(prefix + ".duplicates.tsv", "w") as out:
        out.write("acc_1\tacc_2\tsame\tdiff\tninfo\tidentity\tkinship\n")
        for r in rows:
            out.write("%s\t%s\t%d\t%d\t%d\t%r\t%r\n" % r)
    return rows


def potatoKinship(args):
    g = snp_genotype.Genotype(args['hdf5File'], args.get('hdf5accFile'))
    acc_ix, names = _select.accessions_of(g, args)
    snp_ix = _select.rows_of(g, args) if args.get('bed') else None
    log.info("kinship of %d accessions over %s rows", len(names), "all" if snp_ix is None else len(snp_ix))
    ninfo, same, diff = g.kinship_counts(acc_ix, snp_ix)
    rows = write_outputs(args['outFile'], names, ninfo, same, diff, args.get('min_identity', MIN_IDENTITY), args.get('min_sites', MIN_SITES))
    log.info("%d near-identical pairs", len(rows))
    return rows
