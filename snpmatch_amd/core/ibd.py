"""
``snpmatch ibd``: for EVERY pair of accessions of a database, where along the genome the two are identical -- shared haplotype
segments, identity by descent -- counted on the resident panel, one device call per chromosome (``Genotype.ibd_counts`` ->
``engine.ibd_counts`` -> ``snpm_panel_ibd_counts``).  ``kinship`` lists the pairs that are near-identical genome-wide and ``windows``
looks along the genome for the pairs it is handed; this command finds the pairs that differ genome-wide but share a stretch of one
chromosome -- an introgression, a recent common parent, a mixed seed batch -- and says where two candidate parents of
``parentsearch`` / ``genotype_cross`` cannot be told apart and where ``mosaic`` may switch between accessions for nothing.

Per pair and genome window: n = DB rows where both calls are homozygous, d = rows among them where the two differ (hets and missing
calls count nowhere: the panel is inbred, a het call neither makes nor breaks identity).  A window is *used* with n >=
--min_win_sites, *shared* when used and d <= --max_diff * n, a *break* when used and not shared.  Along a chromosome a run is a
maximal set of shared windows without a break between them; unused windows neither break a run nor count in it; a run is reported
with --min_run shared windows or more.  The reference has nothing like it: the files and thresholds are this package's own.

  <prefix>.ibd.npz           accessions, w_used, w_shared, n_shared, d_shared, run_max, n_runs, w_in_runs (int32 [n, n]; summed over
                             the chromosomes, run_max their maximum), win_chr, win_start, win_end, win_rows (the window table) and
                             per chromosome c used_bits_<c> / shared_bits_<c> (uint32 [n, n, ceil(windows of c / 32)]: window w of
                             the chromosome is bit w % 32 of word w // 32)
  <prefix>.ibd.pairs.tsv     acc_1, acc_2, w_used, w_shared, run_max, n_runs, w_in_runs, d_shared, n_shared of every pair a < b with
                             a reported run, sorted by w_in_runs (most first), then by the two names
  <prefix>.ibd.segments.tsv  acc_1, acc_2, chr, start, end, windows (spanned), shared_windows of every reported run of those pairs
  <prefix>.ibd.json          the settings, the windows per chromosome, the pairs with a run, the longest run with its pair
"""
import json
import logging

import numpy as np

from . import _select, genomes, snp_genotype

log = logging.getLogger(__name__)

BIN_LEN = 100000            # default of -b
MIN_WIN_SITES = 20          # default of --min_win_sites
MAX_DIFF = 0.001            # default of --max_diff
MIN_RUN = 5                 # default of --min_run
COUNT_NAMES = ("w_used", "w_shared", "n_shared", "d_shared", "run_max", "n_runs", "w_in_runs")


def unpack_bits(words, n_win=None):
    """uint32 words (window w is bit w % 32 of word w // 32) as booleans, one per window"""
    words = np.ascontiguousarray(words, dtype="<u4").reshape(-1)
    flags = np.unpackbits(words.view(np.uint8), bitorder="little").astype(bool)
    return flags if n_win is None else flags[:n_win]


def runs_from_bits(used, shared, min_run=1):
    """The reported runs of ONE cell from its two bitsets (uint32 words of ``engine.ibd_counts``): int64 [n_runs, 3] --
    first_window, last_window, n_shared -- in window order.  The used windows are taken out in order; among them a run is a maximal
    stretch of shared ones."""
    u, s = unpack_bits(used), unpack_bits(shared)
    idx = np.flatnonzero(u)
    flag = np.concatenate([[False], s[idx], [False]]).astype(np.int8)
    edge = np.diff(flag)
    lo, hi = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1) - 1        # positions in idx of a run's first and last window
    keep = hi - lo + 1 >= int(min_run)
    return np.stack([idx[lo[keep]], idx[hi[keep]], (hi - lo + 1)[keep]], axis=1).astype(np.int64) if len(idx) else np.zeros((0, 3), dtype=np.int64)


def genome_ibd(g, genome, bin_len, min_win_sites=MIN_WIN_SITES, max_diff_ppm=1000, min_run=MIN_RUN, acc_ix=None):
    """One ``Genotype.ibd_counts`` call per chromosome of ``genome`` (``Genome.get_window_rows``: the rows of a chromosome are a
    range), runs never cross a chromosome end.  Returns ``(table, counts, bits)``: the window table (chr_ix, start, end, first,
    last), the seven matrices summed over the chromosomes (run_max: their maximum) and per chromosome (used_bits, shared_bits).
    A chromosome without DB rows keeps zero bitsets."""
    table = genome.get_window_rows(g.g, bin_len)
    chr_ix, first, last = table[0], table[3], table[4]
    n_acc = len(g.accessions) if acc_ix is None else np.asarray(acc_ix).size
    counts = {name: np.zeros((n_acc, n_acc), dtype=np.int32) for name in COUNT_NAMES}
    bits = []
    for c in range(len(genome.chrs)):
        w = np.flatnonzero(chr_ix == c)
        if not len(w) or last[w[-1]] <= first[w[0]]:
            bits.append(tuple(np.zeros((n_acc, n_acc, (len(w) + 31) // 32), dtype=np.uint32) for _ in range(2)))
            continue
        r0, r1 = int(first[w[0]]), int(last[w[-1]])
        got = g.ibd_counts(np.append(first[w], r1) - r0, min_win_sites, max_diff_ppm, min_run, acc_ix, range(r0, r1))
        for name in COUNT_NAMES:
            if name == "run_max":
                np.maximum(counts[name], got[name], out=counts[name])
            else:
                counts[name] += got[name]
        bits.append((got["used_bits"], got["shared_bits"]))
    return table, counts, bits


def pair_rows(names, counts):
    """rows of the pair table: (name_a, name_b, w_used, w_shared, run_max, n_runs, w_in_runs, d_shared, n_shared, a, b) for a < b with
    a reported run, most windows in runs first, then by name"""
    a, b = np.triu_indices(len(names), k=1)
    keep = counts["n_runs"][a, b] > 0
    rows = [(str(names[i]), str(names[j])) + tuple(int(counts[k][i, j]) for k in ("w_used", "w_shared", "run_max", "n_runs", "w_in_runs", "d_shared", "n_shared")) + (i, j)
            for i, j in zip(a[keep].tolist(), b[keep].tolist())]
    rows.sort(key=lambda r: (-r[6], r[0], r[1]))
    return rows


def write_outputs(prefix, genome, table, names, counts, bits, settings):
    chr_ix, start, end, first, last = table
    names = [str(n) for n in names]
    arrays = dict(accessions=np.asarray(names).astype("U"), win_chr=chr_ix, win_start=start, win_end=end, win_rows=last - first)
    arrays.update(counts)
    for c, (used, shared) in enumerate(bits):
        arrays["used_bits_%s" % genome.chrs[c]], arrays["shared_bits_%s" % genome.chrs[c]] = used, shared
    np.savez(prefix + ".ibd.npz", **arrays)
    pairs = pair_rows(names, counts)
    with open(prefix + ".ibd.pairs.tsv", "w") as out:
        out.write("acc_1\tacc_2\tw_used\tw_shared\trun_max\tn_runs\tw_in_runs\td_shared\tn_shared\n")
        for r in pairs:
            out.write("%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % r[:9])
    longest = None
    with open(prefix + ".ibd.segments.tsv", "w") as out:
        out.write("acc_1\tacc_2\tchr\tstart\tend\twindows\tshared_windows\n")
        for r in pairs:
            i, j = r[9], r[10]
            for c, (used, shared) in enumerate(bits):
                w = np.flatnonzero(chr_ix == c)
                for w_lo, w_hi, n_shared in runs_from_bits(used[i, j], shared[i, j], settings["min_run"]).tolist():
                    out.write("%s\t%s\t%s\t%d\t%d\t%d\t%d\n" % (r[0], r[1], genome.chrs[c], start[w[w_lo]], end[w[w_hi]], w_hi - w_lo + 1, n_shared))
                    if longest is None or n_shared > longest["shared_windows"]:
                        longest = {"acc_1": r[0], "acc_2": r[1], "chr": str(genome.chrs[c]), "start": int(start[w[w_lo]]), "end": int(end[w[w_hi]]),
                                   "windows": w_hi - w_lo + 1, "shared_windows": n_shared}
    stats = dict(settings)
    stats.update(accessions=len(names), windows=int(len(chr_ix)), windows_per_chr={str(genome.chrs[c]): int(np.count_nonzero(chr_ix == c)) for c in range(len(genome.chrs))},
                 pairs_with_a_run=len(pairs), longest_run=longest)
    with open(prefix + ".ibd.json", "w") as out:
        json.dump(stats, out, indent=1, sort_keys=True)
        out.write("\n")
    return stats


def potatoIBD(args):
    """entry point of ``snpmatch ibd``"""
    given = lambda key, default: default if args.get(key) is None else args[key]      # noqa: E731
    bin_len, min_win_sites, min_run = int(given('binLen', BIN_LEN)), int(given('min_win_sites', MIN_WIN_SITES)), int(given('min_run', MIN_RUN))
    max_diff = float(given('max_diff', MAX_DIFF))
    if bin_len < 1:
        raise ValueError("-b / --window_size must be at least 1, got %d" % bin_len)
    if min_win_sites < 1:
        raise ValueError("--min_win_sites must be at least 1, got %d" % min_win_sites)
    if min_run < 1:
        raise ValueError("--min_run must be at least 1, got %d" % min_run)
    if not 0.0 <= max_diff <= 1.0:          # (also refuses nan)
        raise ValueError("--max_diff is a fraction of the homozygous rows, 0 .. 1: got %r" % max_diff)
    max_diff_ppm = int(round(max_diff * 1e6))
    g = snp_genotype.Genotype(args['hdf5File'], args.get('hdf5accFile'))
    genome = genomes.Genome(given('genome', "athaliana_tair10"))
    acc_ix, names = _select.accessions_of(g, args)
    log.info("ibd: windows of %d bp, %d accessions", bin_len, len(names))
    table, counts, bits = genome_ibd(g, genome, bin_len, min_win_sites, max_diff_ppm, min_run, acc_ix)
    settings = {"window_size": bin_len, "min_win_sites": min_win_sites, "max_diff": max_diff, "max_diff_ppm": max_diff_ppm, "min_run": min_run}
    stats = write_outputs(args['outFile'], genome, table, names, counts, bits, settings)
    log.info("%d windows, %d pairs with a run", stats["windows"], stats["pairs_with_a_run"])
    return stats
