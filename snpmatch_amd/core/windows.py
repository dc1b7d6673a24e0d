"""
``snpmatch windows``: a look along the genome -- per genome window the heterozygosity of every accession of a database and the
mismatch of listed pairs of accessions, counted on the resident panel (``Genotype.genome_window_counts`` -> ``engine.window_counts``
-> ``snpm_panel_window_counts``), chromosome by chromosome.  The follow-up of ``kinship``: ``<prefix>.duplicates.tsv`` goes straight
into ``--pairs`` and the answer is WHERE two near-identical lines differ -- a shared segment, an introgression, a mislabelled seed
batch -- and in which windows two candidate parents of a ``cross`` cannot be told apart; the het track shows where a line is not
inbred.

The reference has the two methods (``Genotype.calculate_heterozygosity_windows`` / ``mismatch_between_accs``,
core/snp_genotype.py:297-345) but no such command: the files and the threshold below are this package's own, and the threshold is a
user setting, not a claim.

  <prefix>.windows.npz       chr, start, end, n_rows (DB rows in the window), accessions, counts int32 [windows, accessions, 4]
                             (c0, c1, c2, ninfo), het fp64 [windows, accessions] (c2 / ninfo, nan where ninfo <= --min_sites) and,
                             with --pairs, pairs [n, 2] (names), pair_counts int32 [n, windows, 4] (n, eq, hom_same, hom_diff),
                             mismatch fp64 [n, windows] (1 - eq / n, nan where the pair shares no call)
  <prefix>.het_windows.tsv   one line per window, indexed ``Chr1,1,300000`` as the reference's frame is, one column per accession,
                             ``repr`` precision
  <prefix>.pair_windows.tsv  with --pairs: acc_1, acc_2, chr, start, end, n, eq, mismatch, hom_same, hom_diff per pair and window
  <prefix>.windows.json      the windows, the windows without rows, per accession the windows judged (ninfo > --min_sites) and its
                             mean het over them, per pair the windows judged (n > --min_sites) and those among them with mismatch 0
"""
import json
import logging

import numpy as np

from . import _select, genomes, snp_genotype

log = logging.getLogger(__name__)

MIN_SITES = 5               # default of --min_sites: the reference's y_min of np_get_fraction


def read_pairs(path):
    """(name_1, name_2) of the first two columns of a text file (blanks or tabs); empty lines, # lines and a header line that begins
    with ``acc_1`` (``<prefix>.duplicates.tsv`` of ``kinship``) are skipped"""
    pairs = []
    with open(path) as fh:
        for n, line in enumerate(fh, 1):
            line = line.strip()
            if not line or line.startswith("#") or line.startswith("acc_1"):
                continue
            fields = line.split()
            if len(fields) < 2:
                raise ValueError("%s line %d: expected two accession names, got %r" % (path, n, line))
            pairs.append((fields[0], fields[1]))
    return pairs


def summary(table, names, counts, het, pair_names, pair_counts, mismatch, min_sites):
    n_rows = table[4] - table[3]
    out = {"windows": int(len(n_rows)), "windows_without_rows": int(np.count_nonzero(n_rows == 0)), "min_sites": int(min_sites), "accessions": {}, "pairs": []}
    judged = counts[:, :, 3] > min_sites
    for k, name in enumerate(names):
        vals = het[judged[:, k], k]
        out["accessions"][name] = {"windows_judged": int(judged[:, k].sum()), "mean_het": float(vals.mean()) if len(vals) else None}
    for i, (a, b) in enumerate(pair_names):
        ok = pair_counts[i, :, 0] > min_sites
        out["pairs"].append({"acc_1": a, "acc_2": b, "windows_judged": int(ok.sum()), "windows_identical": int(np.count_nonzero(mismatch[i][ok] == 0.0))})
    return out


def write_outputs(prefix, genome, table, names, counts, pair_names=None, pair_counts=None, min_sites=MIN_SITES):
    chr_ix, start, end, first, last = table
    chrs = np.asarray(genome.chrs)[chr_ix].astype("U") if len(chr_ix) else np.zeros(0, dtype="U1")
    het = snp_genotype.het_from_counts(counts, min_sites)
    arrays = dict(chr=chrs, start=start, end=end, n_rows=last - first, accessions=np.asarray(names).astype("U"), counts=counts, het=het)
    mismatch = None
    if pair_names is not None:
        mismatch = snp_genotype.mismatch_from_counts(pair_counts)
        arrays.update(pairs=np.asarray(pair_names).astype("U").reshape(-1, 2), pair_counts=pair_counts, mismatch=mismatch)
    np.savez(prefix + ".windows.npz", **arrays)
    with open(prefix + ".het_windows.tsv", "w") as out:
        out.write("window" + "".join("\t" + n for n in names) + "\n")
        for w in range(len(start)):
            out.write("%s,%d,%d" % (chrs[w], start[w], end[w]) + "".join("\t%r" % float(v) for v in het[w]) + "\n")
    if pair_names is not None:
        with open(prefix + ".pair_windows.tsv", "w") as out:
            out.write("acc_1\tacc_2\tchr\tstart\tend\tn\teq\tmismatch\thom_same\thom_diff\n")
            for i, (a, b) in enumerate(pair_names):
                for w in range(len(start)):
                    n, eq, same, diff = (int(v) for v in pair_counts[i, w])
                    out.write("%s\t%s\t%s\t%d\t%d\t%d\t%d\t%r\t%d\t%d\n" % (a, b, chrs[w], start[w], end[w], n, eq, float(mismatch[i, w]), same, diff))
    stats = summary(table, names, counts, het, pair_names or [], pair_counts, mismatch, min_sites)
    with open(prefix + ".windows.json", "w") as out:
        json.dump(stats, out, indent=1, sort_keys=True)
        out.write("\n")
    return stats


def potatoWindows(args):
    given = lambda key, default: default if args.get(key) is None else args[key]      # noqa: E731
    bin_len, min_sites = int(given('binLen', 300000)), int(given('min_sites', MIN_SITES))
    if bin_len < 1:
        raise ValueError("-b / --window_size must be at least 1, got %d" % bin_len)
    if min_sites < 0:
        raise ValueError("--min_sites must not be negative, got %d" % min_sites)
    if args.get('pairs_only') and not args.get('pairsFile'):
        raise ValueError("--pairs_only needs --pairs")
    g = snp_genotype.Genotype(args['hdf5File'], args.get('hdf5accFile'))
    genome = genomes.Genome(given('genome', "athaliana_tair10"))
    acc_ix, names = _select.accessions_of(g, args)
    pair_names = pairs = None
    if args.get('pairsFile'):
        pair_names = read_pairs(args['pairsFile'])
        if not pair_names:
            raise ValueError("the pair list %s names no pair" % args['pairsFile'])
        where = {}
        for k, name in enumerate(names):
            where.setdefault(str(name), k)
        unknown = [n for pair in pair_names for n in pair if n not in where]
        if unknown:
            raise ValueError("accessions of the pair list that are not among the selected accessions: %s" % ", ".join(list(dict.fromkeys(unknown))[:10]))
        if args.get('pairs_only'):          # the columns are the pairs' members, in the order they are first named
            members = list(dict.fromkeys(n for pair in pair_names for n in pair))
            picked = np.array([where[n] for n in members], dtype=np.int64)
            acc_ix, names = picked if acc_ix is None else acc_ix[picked], members
            where = {n: k for k, n in enumerate(members)}
        pairs = np.array([[where[a], where[b]] for a, b in pair_names], dtype=np.int64)
    log.info("windows of %d bp: %d accessions, %d pairs", bin_len, len(names), 0 if pairs is None else len(pairs))
    table, counts, pair_counts = g.genome_window_counts(genome, bin_len, acc_ix, pairs)
    stats = write_outputs(args['outFile'], genome, table, [str(n) for n in names], counts, pair_names, pair_counts, min_sites)
    log.info("%d windows, %d without rows", stats["windows"], stats["windows_without_rows"])
    return stats
