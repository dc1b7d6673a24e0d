"""
Which accessions, which rows: the selection every panel command makes from ``-a / --accessions``, ``--pops``, ``--bed`` and
``--sites`` before it asks the resident panel anything, and the small readers the commands share.  The commands re-export the names
they were first written in (``kinship.read_accession_list``, ``ld.read_sites``, ...).
"""
import numpy as np

from . import parsers, snpmatch

NO_CLASS = 0xFF


def read_accession_list(path):
    """accession names, one per line (text after the first blank or tab of a line is ignored; empty lines and # lines are skipped)"""
    names = []
    with open(path) as fh:
        for line in fh:
            line = line.strip()
            if line and not line.startswith("#"):
                names.append(line.split()[0])
    return names


def read_populations(path):
    """(accession, population) pairs of a two-column text file (blanks or tabs; # lines and empty lines are skipped)"""
    pairs = []
    with open(path) as fh:
        for n, line in enumerate(fh, 1):
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            fields = line.split()
            if len(fields) < 2:
                raise ValueError("%s line %d: expected an accession and a population, got %r" % (path, n, line))
            pairs.append((fields[0], fields[1]))
    return pairs


def read_sites(path):
    """(chromosome names, positions) of a ``<prefix>.sites.tsv`` as ``sitestats`` writes it: a header line that names the columns
    ``chr`` and ``pos``, tab-separated rows"""
    with open(path) as fh:
        header = fh.readline().rstrip("\n").split("\t")
        if "chr" not in header or "pos" not in header:
            raise ValueError("%s: the header must name the columns chr and pos, got %r" % (path, header))
        ci, pi = header.index("chr"), header.index("pos")
        chrs, pos = [], []
        for n, line in enumerate(fh, 2):
            fields = line.rstrip("\n").split("\t")
            if fields == [""]:
                continue
            if len(fields) <= max(ci, pi):
                raise ValueError("%s line %d: expected %d columns, got %r" % (path, n, len(header), line))
            chrs.append(fields[ci])
            pos.append(int(fields[pi]))
    return chrs, np.asarray(pos, dtype=np.int64)


def rows_of_sites(g, chrs, pos):
    """the DB rows of the listed sites, ascending; a site that is not in the database is an error"""
    regions = np.asarray(g.g.chr_regions)
    rows = np.zeros(len(pos), dtype=np.int64)
    names = np.asarray(chrs)
    for name in dict.fromkeys(chrs):
        which = g.get_chr_ind(name)
        if which is None:
            raise ValueError("chromosome %s of the site list is not in the database" % name)
        first, last = int(regions[which][0]), int(regions[which][1])
        db_pos = np.asarray(g.g.positions[first:last])
        mine = np.flatnonzero(names == name)
        at = np.searchsorted(db_pos, pos[mine])
        found = (at < len(db_pos)) & (db_pos[np.minimum(at, max(len(db_pos) - 1, 0))] == pos[mine]) if len(db_pos) else np.zeros(len(mine), dtype=bool)
        if not found.all():
            raise ValueError("sites not in the database: %s" % ", ".join("%s:%d" % (name, p) for p in pos[mine][~found][:10].tolist()))
        rows[mine] = first + at
    return np.unique(rows)


def row_chromosomes(g, rows):
    """the chromosome name of each of the given DB rows"""
    regions = np.asarray(g.g.chr_regions)
    which = np.searchsorted(regions[:, 1], rows, side="right")
    return np.asarray(g.chrs).astype("U")[which] if len(rows) else np.zeros(0, dtype="U1")


def hard_classes(gt):
    """The sample's class per entry of its GT column, uint8: 0 ref, 1 alt, 2 het, 0xFF none -- ``parseGT`` of the text, i.e. the
    column in which the reference's ``ParseInputs.get_wei_from_GT`` puts its 1 (weights are [ref, het, alt]: class 1 is column 2,
    class 2 column 1).  As there, the separator is the one of the FIRST entry, a text that is not recognised (``1/2``, the other
    separator) counts as ref, and -1 (``./.``) -- or any other code of a purely numeric column -- has no class."""
    codes = parsers.parseGT(np.asarray(gt))
    out = np.full(len(codes), NO_CLASS, dtype=np.uint8)
    known = (codes >= 0) & (codes <= 2)
    out[known] = codes[known].astype(np.uint8)
    return out


def read_samples(inFile, logDebug=False):
    """(samples, chrs, pos, gt [n_records, n_samples]) of the input: every sample column of a VCF, the one sample of any other file"""
    if inFile.endswith(".vcf") or inFile.endswith(".vcf.gz"):
        calls = parsers.import_vcf_file(inFile, logDebug, samples_to_load=None)
        gt = np.asarray(calls['gt'])
        return [str(s) for s in calls['samples']], np.asarray(calls['chr']), np.asarray(calls['pos']), gt.reshape(len(calls['pos']), -1)
    inputs = snpmatch.parse_inputs_once(inFile, logDebug)
    return [str(inFile).split("/")[-1]], inputs.chrs, inputs.pos, np.asarray(inputs.gt).reshape(-1, 1)


def indices_of(g, names, what, path):
    """the DB index of every name of a list read from ``path`` (``what``: "accession list" / "population file"); an empty list and
    a name the database does not hold are refused"""
    if not names:
        raise ValueError("the %s %s names no accession" % (what, path))
    found = g.get_matching_accs_ix(names)
    missing = [w for w, ix in zip(names, found) if ix is None]
    if missing:
        raise ValueError("accessions not in the database: %s" % ", ".join(missing[:10]))
    return found


def accessions_of(g, args, distinct=False):
    """``(acc_ix, names)`` from -a / --accessions: the DB indices (int64) and the names of the listed accessions in the order of the
    list, or None and the names of every accession of the database without a list.  ``distinct``: a list that names an accession
    twice is refused (a scan whose columns must differ)."""
    path = args.get('accFile')
    if not path:
        return None, g.accessions.tolist()
    wanted = read_accession_list(path)
    found = indices_of(g, wanted, "accession list", path)
    if distinct and len(set(found)) != len(found):
        raise ValueError("the accession list %s names an accession twice" % path)
    return np.array(found, dtype=np.int64), wanted


def one_row_option(args):
    """--bed and --sites exclude each other; a command that wants the refusal before it opens the database calls this first"""
    if args.get('bed') and args.get('sitesFile'):
        raise ValueError("give either --bed or --sites, not both")


def rows_of(g, args):
    """the DB rows (int64, ascending) from --sites (a site list), --bed (a region) or neither (every row)"""
    one_row_option(args)
    if args.get('sitesFile'):
        return rows_of_sites(g, *read_sites(args['sitesFile']))
    if args.get('bed'):
        return np.asarray(g.determine_snp_ix_given_bed(args['bed']), dtype=np.int64)
    return np.arange(len(g.g.positions), dtype=np.int64)
