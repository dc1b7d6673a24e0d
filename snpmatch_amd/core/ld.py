"""
``snpmatch ld``: linkage disequilibrium between neighbouring SNPs of a database and pruning of a marker set by it -- the step after
the MAF / missingness filter of ``sitestats``: markers in tight LD carry the same information, inflate the counts of the binomial
test and waste rows of a shared marker set.  r2 of every row with each of the ``--band`` rows after it on its chromosome is
computed on the resident panel (``Genotype.ld_band`` -> ``engine.ld_band`` -> ``snpm_panel_ld_band``), chromosome by chromosome:
pairs never span chromosomes, and host memory is one chromosome's band.

The reference names the capability (``calculate_ld``, core/snp_genotype.py:291-295, :348-358) but neither form runs, and it has no
such command: the files and the thresholds below are this package's own, and the thresholds are user settings, not claims.

  <prefix>.pruned.tsv   chr, pos of the rows kept by the greedy prune (``snpm_ld_prune``): in row order a row is kept unless an
                        earlier KEPT row of its band has r2 > --r2 with it; an undefined r2 never prunes
  <prefix>.ld.json      rows, rows kept, pairs with a defined r2, and the mean r2 per offset d = 1 .. band: the decay curve
  <prefix>.ld.npz       only with --keep_r2: chr, pos, r2 fp64 [rows, band] (nan: undefined, past the chromosome's end, or
                        further apart than --window_bp), keep
"""
import json
import logging

import numpy as np

from . import _select, snp_genotype
from ._select import read_sites, rows_of_sites  # noqa: F401  (the names tests and tools import)

log = logging.getLogger(__name__)


def mask_window(r2, pos, window_bp):
    """r2 [n, band] with the pairs whose rows lie more than ``window_bp`` apart set to nan (in place)"""
    n, band = r2.shape
    for d in range(1, min(band, n - 1) + 1):
        far = pos[d:] - pos[:n - d] > window_bp
        r2[:n - d, d - 1][far] = np.nan
    return r2


def potatoLD(args):
    from .. import engine
    _select.one_row_option(args)
    given = lambda key, default: default if args.get(key) is None else args[key]      # noqa: E731
    band, min_n, threshold = int(given('band', 50)), int(given('min_n', 2)), float(given('r2', 0.2))
    if not 1 <= band <= engine.LD_MAX_BAND:
        raise ValueError("--band must be 1 .. %d, got %d" % (engine.LD_MAX_BAND, band))
    if min_n < 1:
        raise ValueError("--min_n must be at least 1, got %d" % min_n)
    g = snp_genotype.Genotype(args['hdf5File'], args.get('hdf5accFile'))
    accs, _ = _select.accessions_of(g, args, distinct=True)
    rows = _select.rows_of(g, args)
    positions = np.asarray(g.g.positions)
    total, defined = np.zeros(band, dtype=np.float64), np.zeros(band, dtype=np.int64)
    kept_rows, kept_flags, bands = [], [], []
    for first, last in np.asarray(g.g.chr_regions).tolist():
        mine = rows[(rows >= first) & (rows < last)]
        if not len(mine):
            continue
        r2 = g.ld_band(band, accs, mine, min_n=min_n, counts=False)[1]
        if args.get('window_bp') is not None:
            mask_window(r2, positions[mine].astype(np.int64), int(args['window_bp']))
        keep = engine.ld_prune(r2, None, threshold)
        known = ~np.isnan(r2)
        total += np.where(known, r2, 0.0).sum(axis=0)
        defined += known.sum(axis=0)
        kept_rows.append(mine)
        kept_flags.append(keep)
        if args.get('keep_r2'):
            bands.append(r2)
    rows = np.concatenate(kept_rows) if kept_rows else np.zeros(0, dtype=np.int64)
    keep = np.concatenate(kept_flags) if kept_flags else np.zeros(0, dtype=bool)
    chrs, pos = _select.row_chromosomes(g, rows), positions[rows].astype(np.int64)
    with open(args['outFile'] + ".pruned.tsv", "w") as out:
        out.write("chr\tpos\n")
        for r in np.flatnonzero(keep).tolist():
            out.write("%s\t%d\n" % (chrs[r], pos[r]))
    stats = {"rows": int(len(rows)), "rows_kept": int(keep.sum()), "pairs_defined": int(defined.sum()), "band": band, "r2_threshold": threshold,
             "min_n": min_n, "window_bp": args.get('window_bp'),
             "mean_r2_by_offset": [float(total[d] / defined[d]) if defined[d] else None for d in range(band)]}
    with open(args['outFile'] + ".ld.json", "w") as out:
        json.dump(stats, out, indent=1, sort_keys=True)
        out.write("\n")
    if args.get('keep_r2'):
        np.savez(args['outFile'] + ".ld.npz", chr=chrs, pos=pos, r2=np.concatenate(bands) if bands else np.zeros((0, band)), keep=keep)
    log.info("%d of %d rows kept at r2 <= %g within %d rows", stats["rows_kept"], stats["rows"], threshold, band)
    return stats
