"""
``snpmatch mixture``: is the sample ONE accession of the database, or reads of TWO accessions in unequal proportion -- seed of a
second line in the batch, two plants in one tube, DNA carried over on a plate -- and if so, which two and how much of each.

Neither ``inbred`` (a weak, ambiguous top hit) nor ``f1search`` (hard calls against an exact 50:50 heterozygote) sees a 15 %
admixture.  What separates the cases is the allele balance of the reads, the FORMAT ``AD`` field, which no other reader of the
package looks at.  The model: a pool of accession a (major) with a fraction alpha of accession b.  At a row where a has the
homozygous call ca and b the call cb the expected alt-read fraction is ``f = (1 - alpha) ca + alpha cb``, with a read error e
``f' = f (1 - 2 e) + e``, so the log-likelihood of every (a, b, alpha) is a function of eight read sums per ordered pair,

    T[w][ca][cb][a][b] = sum over rows where a has call ca and b has call cb of the sample's alt (w = 0) or ref (w = 1) reads
    LL(a, b, alpha) = sum over ca, cb of T[0] log f' + T[1] log(1 - f')

and the table of ALL ordered pairs is one device call (``Genotype.mix_counts`` -> ``engine.mix_counts`` ->
``snpm_panel_mix_counts``).  Rows where either accession is het, "other" or missing do not count for that pair, as in ``kinship``.
The fit on top (``fit_pairs``) is host numpy: every ordered pair, every alpha of a grid on [0, 0.5]; alpha = 0 is "a alone on these
rows".  Pairs with ``--min_reads`` reads or more are ranked by LL(alpha_hat) per read; the verdict for the best pair is ``single``
when twice its gain over alpha = 0 stays below ``snpmatch.lr_thres``, else ``mixture`` -- or ``mixture_or_f1`` from alpha_hat 0.4 on:
allele balance cannot tell a 50:50 pool from an F1, ``f1search`` names the parents of that case.

The reference has no such command: the files, the options and the thresholds are this package's own.

  <prefix>.mixture.json         rows matched and dropped per rule, the best single accession, the shortlist with alpha_hat, llr and
                                reads, the verdict
  <prefix>.mixture.npz          accessions (the candidates), table (int32 [2, 2, 2, n, n]), alpha, ll, llr (fp64 [n, n]), reads
                                (int64 [n, n]) of every ordered pair
  <prefix>.mixture.scores.txt   the shortlist as a table
"""
import json
import logging
import zipfile

import numpy as np

from . import _select, _vcf, snp_genotype, snpmatch

log = logging.getLogger(__name__)

ERR = 0.01                  # default of --err: probability that a read shows the other allele
GRID = 0.01                 # default of --grid: step of alpha on [0, 0.5]
MAX_DEPTH = 15              # default of --max_depth: rows with more reads are dropped (collapsed repeats; 4 bit slices per count)
MIN_READS = 200             # default of --min_reads: reads below which an ordered pair is not ranked
TOP = 10                    # default of --top: ordered pairs of the shortlist
MAX_TOP = 1000
F1_ALPHA = 0.4              # alpha_hat from which the verdict is mixture_or_f1
FIT_BLOCK_BYTES = 64 << 20  # the largest temporary of fit_pairs


# ------------------------------------------------------------------------------------------------ the sample's reads
def _allele_depths(keys, text):
    """(ref, alt) reads of one sample column given the FORMAT keys, or None: a FORMAT without AD, an entry that ends before its AD
    subfield, an AD that does not hold exactly two integers (``.`` entries, more alleles)"""
    for key, val in zip(keys, text.split(":")):
        if key == "AD":
            parts = val.split(",")
            if len(parts) != 2:
                return None
            try:
                r, a = int(parts[0]), int(parts[1])
            except ValueError:
                return None
            return (r, a) if r >= 0 and a >= 0 else None
    return None


def read_allele_depths(path, sample=0):
    """The allele depths of one sample column of a VCF: dict with ``chr`` (text), ``pos``, ``ref``, ``alt`` (int64 [n]) of the records
    that have ONE ALT allele, a FORMAT with ``AD`` holding two integers for the sample, and at least one read -- whether or not GT
    was called -- plus ``sample`` (its name), ``records`` (data lines read) and ``dropped`` (records left out, per rule).  ``sample``:
    the index of the column or its name.  A file that cannot carry read counts is refused: a BED file, an ``.npz`` cache of parsed
    calls, a VCF in which no record's FORMAT has AD."""
    name = str(path)
    if name.endswith(".npz"):
        raise ValueError("%s: the .npz cache of a parsed sample keeps GT and PL, not the read counts (FORMAT AD): give the VCF itself" % name)
    if name.endswith(".bed"):
        raise ValueError("%s: a BED file holds genotype calls, not read counts: mixture needs a VCF with FORMAT AD" % name)
    if not (name.endswith(".vcf") or name.endswith(".vcf.gz")):
        raise ValueError("%s: mixture reads a VCF (.vcf / .vcf.gz) with FORMAT AD" % name)
    names, column = None, None
    chrom, pos, ref, alt = [], [], [], []
    records = any_ad = 0
    dropped = {"multi_allelic": 0, "no_ad": 0, "zero_depth": 0}
    with _vcf._open(name) as fh:
        for line in fh:
            if line.startswith("#"):
                if line.startswith("#CHROM"):
                    names = line.rstrip("\n").split("\t")[9:]
                    column = _sample_column(names, sample, name)
                continue
            rec = line.rstrip("\n").split("\t")
            if len(rec) < 8:
                continue
            if column is None:
                raise ValueError("%s: no #CHROM line before the records" % name)
            records += 1
            keys = rec[8].split(":") if len(rec) > 8 else []
            any_ad |= "AD" in keys
            if rec[4] == "." or "," in rec[4]:
                dropped["multi_allelic"] += 1
                continue
            depths = _allele_depths(keys, rec[9 + column]) if len(rec) > 9 + column else None
            if depths is None:
                dropped["no_ad"] += 1
                continue
            if depths[0] + depths[1] < 1:
                dropped["zero_depth"] += 1
                continue
            chrom.append(rec[0])
            pos.append(int(rec[1]))
            ref.append(depths[0])
            alt.append(depths[1])
    if names is None:
        raise ValueError("%s: no #CHROM line" % name)
    if records and not any_ad:
        raise ValueError("%s: no record's FORMAT carries AD (allele depths): the caller must write it (GATK and bcftools call -a AD do)" % name)
    return {"sample": names[column], "records": records, "dropped": dropped, "chr": np.array(chrom, dtype="U"),
            "pos": np.array(pos, dtype=np.int64), "ref": np.array(ref, dtype=np.int64), "alt": np.array(alt, dtype=np.int64)}


def _sample_column(names, sample, path):
    text = str(sample)
    if text in names:
        return names.index(text)
    try:
        k = int(text)
    except ValueError:
        raise ValueError("%s has no sample column named %s (it has: %s)" % (path, text, ", ".join(names[:10])))
    if not 0 <= k < len(names):
        raise ValueError("%s has %d sample columns: --sample %d is outside" % (path, len(names), k))
    return k


# ------------------------------------------------------------------------------------------------ the fit
def alpha_grid(step):
    """alpha = 0, step, 2 step, ... 0.5: ``step`` must divide 0.5 (to 1e-9) and be 0.0005 or more"""
    step = float(step)
    n = int(round(0.5 / step)) if step > 0 else 0
    if n < 1 or n > 1000 or abs(n * step - 0.5) > 1e-9:
        raise ValueError("--grid must divide 0.5 and lie in 0.0005 .. 0.5, got %r" % step)
    return np.arange(n + 1) * (0.5 / n)


def _log_terms(err, grid):
    """log f' and log(1 - f') per alpha and pair of calls: fp64 [n_alpha, 2 (alt, ref), 2, 2]"""
    out = np.zeros((len(grid), 2, 2, 2))
    for k, alpha in enumerate(np.asarray(grid, dtype=np.float64).tolist()):
        for ca in (0, 1):
            for cb in (0, 1):
                f = (1.0 - alpha) * ca + alpha * cb
                fe = f * (1.0 - 2.0 * err) + err
                out[k, 0, ca, cb], out[k, 1, ca, cb] = np.log(fe), np.log(1.0 - fe)
    return out


def fit_pairs(table, err, grid):
    """The model fitted to every ORDERED pair (a major, b minor) of a table [2, 2, 2, n, n] of ``mix_counts``, on the host: LL(a, b,
    alpha) for every alpha of ``grid`` (ascending, grid[0] == 0), in blocks of accession rows so that a temporary stays below 64 MB.
    Returns a dict of [n, n] arrays -- ``alpha`` (alpha_hat: the first alpha of the largest LL), ``ll`` (LL(alpha_hat)), ``llr``
    (LL(alpha_hat) - LL(0)), ``reads`` (int64: the sum of the eight cells) -- and, from the diagonal, ``single_ll`` and
    ``single_reads`` [n]: every accession on its own over the rows where it is homozygous."""
    table = np.asarray(table)
    assert table.ndim == 5 and table.shape[:3] == (2, 2, 2) and table.shape[3] == table.shape[4], "table: [2, 2, 2, n, n]"
    grid = np.asarray(grid, dtype=np.float64).reshape(-1)
    assert len(grid) >= 1 and grid[0] == 0.0 and 0.0 < err < 0.5, "grid starts at alpha = 0; 0 < err < 0.5"
    n, n_alpha = table.shape[3], len(grid)
    coef = _log_terms(float(err), grid).reshape(n_alpha, 8)
    alpha, ll, llr, single_ll = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n)), np.zeros(n)
    reads = table.astype(np.int64).sum(axis=(0, 1, 2))
    block = max(1, int(FIT_BLOCK_BYTES // (8 * max(n_alpha, 8) * max(n, 1))))
    for a0 in range(0, n, block):
        a1 = min(n, a0 + block)
        cells = table[:, :, :, a0:a1, :].reshape(8, -1).astype(np.float64)
        lls = (coef @ cells).reshape(n_alpha, a1 - a0, n)
        best = np.argmax(lls, axis=0)
        top = np.take_along_axis(lls, best[None], axis=0)[0]
        alpha[a0:a1], ll[a0:a1], llr[a0:a1] = grid[best], top, top - lls[0]
        single_ll[a0:a1] = lls[0][np.arange(a1 - a0), np.arange(a0, a1)]
    return {"alpha": alpha, "ll": ll, "llr": llr, "reads": reads, "single_ll": single_ll, "single_reads": reads.diagonal().copy()}


def shortlist(fit, min_reads=MIN_READS, top=TOP):
    """the ``top`` best ordered pairs (a, b), a != b, with ``reads >= min_reads``: ranked by LL(alpha_hat) / reads, descending; ties
    to the lower (a, b)"""
    reads, ll = fit["reads"], fit["ll"]
    n = reads.shape[0]
    keep = (reads >= max(int(min_reads), 1)) & ~np.eye(n, dtype=bool)
    a, b = np.nonzero(keep)                                          # row-major: ascending (a, b)
    per_read = ll[a, b] / reads[a, b]
    order = np.argsort(-per_read, kind="stable")[:int(top)]
    return [(int(a[k]), int(b[k])) for k in order]


def best_single(fit, min_reads=MIN_READS):
    """the accession with the highest LL per read on its own among those with ``min_reads`` reads or more, or None"""
    reads, ll = fit["single_reads"], fit["single_ll"]
    keep = np.flatnonzero(reads >= max(int(min_reads), 1))
    if not len(keep):
        return None
    return int(keep[np.argmax(ll[keep] / reads[keep])])


def verdict_of(fit, pairs):
    """``single`` / ``mixture`` / ``mixture_or_f1`` from the best pair of the shortlist; ``no_call`` without one"""
    if not pairs:
        return "no_call"
    a, b = pairs[0]
    if 2.0 * fit["llr"][a, b] < snpmatch.lr_thres:
        return "single"
    return "mixture_or_f1" if fit["alpha"][a, b] >= F1_ALPHA else "mixture"


# ------------------------------------------------------------------------------------------------ the command
def _options(args):
    given = lambda key, default: default if args.get(key) is None else args[key]      # noqa: E731
    err, step = float(given('err', ERR)), float(given('grid', GRID))
    max_depth, min_reads, top = int(given('max_depth', MAX_DEPTH)), int(given('min_reads', MIN_READS)), int(given('top', TOP))
    if not 0.0 < err < 0.5:
        raise ValueError("--err must lie between 0 and 0.5, got %r" % err)
    if not 1 <= max_depth <= 255:
        raise ValueError("--max_depth must be 1 .. 255 (the counts travel as bytes), got %d" % max_depth)
    if min_reads < 1:
        raise ValueError("--min_reads must be 1 or more, got %d" % min_reads)
    if not 1 <= top <= MAX_TOP:
        raise ValueError("--top must be 1 .. %d, got %d" % (MAX_TOP, top))
    return err, alpha_grid(step), step, max_depth, min_reads, top


def _save_npz(path, **arrays):
    """``np.savez`` with a fixed time stamp per member: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED, allowZip64=True) as zf:
        for name, value in arrays.items():
            with zf.open(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), "w", force_zip64=True) as fh:
                np.lib.format.write_array(fh, np.asanyarray(value), allow_pickle=False)


class Mixture(object):
    """the reads of one sample against the candidate accessions ``acc_ix`` (None: all) over the DB rows ``sel_rows`` (None: all):
    the matched rows, the table, the fit, the shortlist and the verdict"""

    def __init__(self, reads, g, err=ERR, grid=None, max_depth=MAX_DEPTH, min_reads=MIN_READS, top=TOP, acc_ix=None, sel_rows=None):
        self.reads, self.g, self.err, self.max_depth, self.min_reads, self.top = reads, g, err, max_depth, min_reads, top
        self.grid = alpha_grid(GRID) if grid is None else np.asarray(grid, dtype=np.float64)
        self.acc_ix = None if acc_ix is None else np.asarray(acc_ix, dtype=np.int64).reshape(-1)
        db_rows, rec_rows = g.get_positions_idxs(reads["chr"], reads["pos"])
        self.rows = {"records": int(reads["records"]), "with_reads": int(len(reads["pos"])), "matched": int(len(db_rows))}
        self.rows.update({"dropped_" + k: int(v) for k, v in reads["dropped"].items()})
        if sel_rows is not None:
            keep = np.isin(db_rows, sel_rows)
            db_rows, rec_rows = db_rows[keep], rec_rows[keep]
        self.rows["dropped_not_selected"] = self.rows["matched"] - int(len(db_rows))
        alt, ref = reads["alt"][rec_rows], reads["ref"][rec_rows]
        keep = alt + ref <= max_depth
        self.rows["dropped_too_deep"] = int(len(keep) - np.count_nonzero(keep))
        self.db_rows, self.alt, self.ref = db_rows[keep], alt[keep].astype(np.uint8), ref[keep].astype(np.uint8)
        self.rows["used"] = int(len(self.db_rows))
        self.table = g.mix_counts(self.alt, self.ref, self.acc_ix, self.db_rows)
        self.fit = fit_pairs(self.table, err, self.grid)
        self.pairs = shortlist(self.fit, min_reads, top)
        self.single = best_single(self.fit, min_reads)
        self.verdict = verdict_of(self.fit, self.pairs)
        names = np.asarray(g.accessions).astype("U")
        self.names = names if self.acc_ix is None else names[self.acc_ix]
        log.info("mixture: %d rows used, %d candidate accessions, verdict %s", self.rows["used"], len(self.names), self.verdict)

    def summary(self):
        fit, names = self.fit, self.names.tolist()
        out = {"sample": self.reads["sample"], "rows": self.rows, "candidates": len(names), "err": self.err, "grid": float(self.grid[1] - self.grid[0]) if len(self.grid) > 1 else 0.0,
               "max_depth": self.max_depth, "min_reads": self.min_reads, "top": self.top, "reads_used": int(self.alt.astype(np.int64).sum() + self.ref.astype(np.int64).sum()),
               "best_single": None, "shortlist": [], "best_pair": None, "verdict": self.verdict, "lr_thres": snpmatch.lr_thres}
        if self.single is not None:
            k = self.single
            out["best_single"] = {"accession": names[k], "ll": float(fit["single_ll"][k]), "reads": int(fit["single_reads"][k]),
                                  "ll_per_read": float(fit["single_ll"][k] / fit["single_reads"][k])}
        for a, b in self.pairs:
            out["shortlist"].append({"major": names[a], "minor": names[b], "alpha": float(fit["alpha"][a, b]), "ll": float(fit["ll"][a, b]),
                                     "llr": float(fit["llr"][a, b]), "reads": int(fit["reads"][a, b]), "ll_per_read": float(fit["ll"][a, b] / fit["reads"][a, b])})
        if self.pairs:
            out["best_pair"] = out["shortlist"][0]
        if self.verdict == "mixture_or_f1":
            out["note"] = "allele balance cannot tell a 50:50 pool from an F1: f1search names the parents of an F1"
        return out

    def write_outputs(self, prefix):
        stats = self.summary()
        with open(prefix + ".mixture.json", "w") as out:
            json.dump(stats, out, indent=1, sort_keys=True)
            out.write("\n")
        fit = self.fit
        _save_npz(prefix + ".mixture.npz", accessions=self.names, table=self.table, alpha=fit["alpha"], ll=fit["ll"], llr=fit["llr"], reads=fit["reads"])
        with open(prefix + ".mixture.scores.txt", "w") as out:
            out.write("major\tminor\talpha\tll\tllr\treads\tll_per_read\n")
            for p in stats["shortlist"]:
                out.write("%s\t%s\t%.4f\t%r\t%r\t%d\t%r\n" % (p["major"], p["minor"], p["alpha"], p["ll"], p["llr"], p["reads"], p["ll_per_read"]))
        self.stats = stats
        return stats


def potatoMixture(args):
    """entry point of ``snpmatch mixture``"""
    err, grid, _, max_depth, min_reads, top = _options(args)
    _select.one_row_option(args)
    given = args.get('sample')
    reads = read_allele_depths(args['inFile'], 0 if given is None else given)
    log.info("loading genotype files!")
    g = snp_genotype.Genotype(args['hdf5File'], args.get('hdf5accFile'))
    acc_ix, _ = _select.accessions_of(g, args, distinct=True)
    sel_rows = _select.rows_of(g, args) if args.get('bed') or args.get('sitesFile') else None
    mix = Mixture(reads, g, err, grid, max_depth, min_reads, top, acc_ix, sel_rows)
    mix.write_outputs(args['outFile'])
    log.info("finished!")
    return mix.stats
