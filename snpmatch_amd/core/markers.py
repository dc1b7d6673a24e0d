"""
``snpmatch markers``: a small set of SNPs that separates EVERY pair of accessions of a database -- the list to genotype with an
amplicon or KASP panel so that a seed stock's identity can be checked -- chosen on the resident panel, all rounds in one device call
(``Genotype.marker_select`` -> ``engine.marker_select`` -> ``snpm_panel_marker_select``).  ``power`` says that random sets of n SNPs
confuse these pairs; this command says which SNPs to take so that no pair is confused.  The candidates come from ``sitestats
--min_maf / --max_missing`` (``<prefix>.sites.tsv``), from ``ld`` (``<prefix>.pruned.tsv``) or from ``--bed``; the pairs it reports
as unresolved are the duplicates of ``kinship`` and the shared segments of ``ibd``.

A SNP separates two accessions when both calls are homozygous and different; hets and missing calls never separate.  Every pair
must be separated by --depth chosen SNPs.  The choice is the textbook greedy set cover -- per round the SNP that separates the most
pairs still in need, the first such SNP in the candidate order on a tie -- which is NOT optimal: a smaller set may exist.  What it
guarantees: every pair the candidates can separate --depth times is separated that often unless --max_markers stopped the loop,
and when it stops for lack of gain the pairs left are exactly those the candidates cannot tell apart.  With --min_dist_bp a chosen
SNP excludes every candidate closer than that on its chromosome (unlinked markers).  The reference has nothing like it: the files
are this package's own.  To check a chosen set by hand, hand ``<prefix>.markers.tsv`` to ``power --sites``.

  <prefix>.markers.tsv    order, chr, pos, gain (pairs in need the SNP separated when it was picked), remaining (units of need left
                          after the pick: the sum over all pairs), in pick order; a site list for --sites of ld / power / markers
  <prefix>.markers.json   accessions, pairs, depth, candidates, markers, remaining, stop_reason (0 all pairs resolved, 1 max_markers
                          reached, 2 no candidate with gain), unresolved_pairs and the first 1000 of them by name with their need
  <prefix>.markers.npz    accessions, rows / chr / pos of the candidates, chosen (positions in them), gain_at, need, first_gain (the
                          pairs every candidate separates)
"""
import json
import logging

import numpy as np

from . import _select, snp_genotype

log = logging.getLogger(__name__)

STOP_REASONS = ("all pairs resolved", "max_markers reached", "no candidate with gain")
UNRESOLVED_LISTED = 1000


def coordinates(g, rows, min_dist):
    """one int64 per DB row of ``rows``: its position, every chromosome shifted behind the end of the previous one plus
    ``min_dist`` -- two rows of different chromosomes are never closer than ``min_dist``, so chromosomes do not exclude each other"""
    rows = np.asarray(rows, dtype=np.int64)
    regions = np.asarray(g.g.chr_regions).astype(np.int64)
    positions = np.asarray(g.g.positions)
    which = np.searchsorted(regions[:, 1], rows, side="right")
    ends = np.array([int(positions[last - 1]) if last > first else 0 for first, last in regions.tolist()], dtype=np.int64)
    offset = np.concatenate([[0], np.cumsum(ends + int(min_dist))[:-1]]).astype(np.int64)
    return positions[rows].astype(np.int64) + offset[which] if len(rows) else np.zeros(0, dtype=np.int64)


def unresolved_pairs(names, need, limit=UNRESOLVED_LISTED):
    """(count, the first ``limit``) of the pairs a < b with need > 0, as dicts acc_1 / acc_2 / need, in index order"""
    a, b = np.nonzero(np.triu(need, k=1))
    return int(len(a)), [{"acc_1": str(names[i]), "acc_2": str(names[j]), "need": int(need[i, j])} for i, j in zip(a[:limit].tolist(), b[:limit].tolist())]


def write_outputs(prefix, names, rows, chrs, pos, result, settings):
    names = [str(n) for n in names]
    chosen, gain_at = result["chosen"], result["gain_at"]
    total = settings["depth"] * (len(names) * (len(names) - 1) // 2)
    left = total - np.cumsum(gain_at.astype(np.int64))
    with open(prefix + ".markers.tsv", "w") as out:
        out.write("order\tchr\tpos\tgain\tremaining\n")
        for k, r in enumerate(chosen.tolist()):
            out.write("%d\t%s\t%d\t%d\t%d\n" % (k + 1, chrs[r], pos[r], gain_at[k], left[k]))
    n_unresolved, listed = unresolved_pairs(names, result["need"])
    stats = dict(settings)
    stats.update(accessions=len(names), pairs=len(names) * (len(names) - 1) // 2, candidates=int(len(rows)), markers=int(result["n_chosen"]),
                 remaining=int(result["remaining"]), stop_reason=int(result["stop_reason"]), stop_reason_text=STOP_REASONS[result["stop_reason"]],
                 unresolved_pairs=n_unresolved, unresolved=listed)
    with open(prefix + ".markers.json", "w") as out:
        json.dump(stats, out, indent=1, sort_keys=True)
        out.write("\n")
    np.savez(prefix + ".markers.npz", accessions=np.asarray(names).astype("U"), rows=rows, chr=chrs, pos=pos, chosen=chosen, gain_at=gain_at,
             need=result["need"], first_gain=result["first_gain"])
    return stats


def potatoMarkers(args):
    """entry point of ``snpmatch markers``"""
    _select.one_row_option(args)
    given = lambda key, default: default if args.get(key) is None else args[key]      # noqa: E731
    depth, min_dist = int(given('depth', 1)), int(given('min_dist_bp', 0))
    max_markers = None if args.get('max_markers') is None else int(args['max_markers'])
    if not 1 <= depth <= 255:
        raise ValueError("--depth must be 1 .. 255, got %d" % depth)
    if min_dist < 0:
        raise ValueError("--min_dist_bp must not be negative, got %d" % min_dist)
    if max_markers is not None and max_markers < 1:
        raise ValueError("--max_markers must be at least 1, got %d" % max_markers)
    g = snp_genotype.Genotype(args['hdf5File'], args.get('hdf5accFile'))
    acc_ix, names = _select.accessions_of(g, args, distinct=True)
    rows = _select.rows_of(g, args)
    coord = coordinates(g, rows, min_dist) if min_dist > 0 else None
    log.info("markers: %d accessions, %d candidate rows, depth %d", len(names), len(rows), depth)
    result = g.marker_select(depth, max_markers, coord, min_dist, None, acc_ix, rows)
    chrs, pos = _select.row_chromosomes(g, rows), np.asarray(g.g.positions)[rows].astype(np.int64)
    settings = {"depth": depth, "max_markers": max_markers, "min_dist_bp": min_dist}
    stats = write_outputs(args['outFile'], names, rows, chrs, pos, result, settings)
    log.info("%d markers, %d units of need left (%s), %d unresolved pairs", stats["markers"], stats["remaining"], stats["stop_reason_text"], stats["unresolved_pairs"])
    return stats
