"""
Genome description and window segmentation for ``cross``.

``Genome(ref_json)`` (interface of the reference's core/genomes.py:16-127) loads chromosome names and
lengths from a genome id shipped under ``snpmatch_amd/resources/genomes`` or from a JSON file with
``ref_chrs`` / ``ref_chrlen``.  ``get_bins_genome(g, binLen)`` and ``get_bins_arrays(chrs, pos, binLen)``
yield, chromosome after chromosome in genome order, one ``(chr_ix, [start, end], [indices])`` triple per
window ``[1 + k*binLen, (k+1)*binLen]`` -- indices into the DB rows and into the sample respectively.

Positions of one chromosome are sorted in every real input, so the members of all windows of a
chromosome come from two ``searchsorted`` calls.  Inputs that are not sorted (or hold positions < 1) go
through ``_scan_windows``, which walks position by position with the control flow of the reference
(core/genomes.py:111-127) so that its behaviour on such inputs is reproduced as well.
"""
import json
import logging
import os.path
from glob import glob

import numpy as np

log = logging.getLogger(__name__)

_GENOME_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'resources', 'genomes')
_MISMATCH = "Please change default --genome option"


def _bare(names):
    """lower-case chromosome names without 'chr'"""
    return np.char.replace(np.char.lower(np.array(names, dtype="str")), "chr", "")


def _scan_windows(chr_len, positions, bin_len, first_index):
    cursor = 0
    for lo in range(1, int(chr_len), bin_len):
        hi = lo + bin_len - 1
        members = []
        k = cursor
        while k < len(positions):
            p = positions[k]
            k += 1
            if p < lo:
                continue            # (the reference does not advance its index here either)
            if p > hi:
                break
            members.append(cursor + first_index)
            cursor += 1
        yield ([lo, hi], members)


def get_bins_echr(real_chrlen, chr_pos, binLen, rel_ix):
    """windows of one chromosome: ([start, end], [rel_ix + index of every position inside])"""
    chr_pos = np.asarray(chr_pos)
    binLen = int(binLen)
    unsorted = len(chr_pos) > 0 and (chr_pos[0] < 1 or bool(np.any(np.diff(chr_pos) < 0)))
    if unsorted:
        for w in _scan_windows(real_chrlen, chr_pos, binLen, rel_ix):
            yield w
        return
    starts = np.arange(1, int(real_chrlen), binLen, dtype=np.int64)
    first = np.searchsorted(chr_pos, starts, side="left") + rel_ix
    last = np.searchsorted(chr_pos, starts + (binLen - 1), side="right") + rel_ix
    for s, a, b in zip(starts.tolist(), first.tolist(), last.tolist()):
        yield ([s, s + binLen - 1], list(range(a, b)))


class Genome(object):

    def __init__(self, ref_json):
        shipped = os.path.join(_GENOME_DIR, str(ref_json) + '.json')
        path = shipped if os.path.exists(shipped) else ref_json
        assert os.path.exists(path), "Reference json file missing: %s" % path
        with open(path) as fh:
            self.json = json.load(fh)
        self.chrs = np.array(self.json['ref_chrs'], dtype="str")
        self.chrlen = np.array(self.json['ref_chrlen'], dtype=int)
        self.chrs_ids = _bare(self.chrs)

    def get_genome_ids(self):
        return sorted(os.path.basename(f)[:-len(".json")] for f in glob(os.path.join(_GENOME_DIR, '*.json')))

    def get_chr_ind(self, echr):
        """index of a chromosome name (or of every name in an array) in this genome; None if unknown"""
        def lookup(name):
            hit = np.flatnonzero(self.chrs_ids == _bare([name])[0])
            return int(hit[0]) if len(hit) == 1 else None
        if isinstance(echr, (bytes, np.bytes_)):
            echr = echr.decode()
        if isinstance(echr, str):
            return lookup(echr)
        return np.array([lookup(str(e)) for e in np.asarray(echr)], dtype="int8")

    def estimated_cM_distance(self, snp_position):
        """genetic position in cM of 'chr1,150000' (or of the middle of 'chr1,1,300000'): the chromosome's mean recombination
        rate (``recomb_rates`` of the genome JSON, cM per Mb; 3 for every chromosome when the file has none) times the
        physical position in Mb (interface of the reference's core/genomes.py:53-70)"""
        if "recomb_rates" in self.json.keys():
            rates = self.json['recomb_rates']
        else:
            log.warning("Average recombination rates were missing in genome file. Add rates for each chromosome as an array in genome json file under 'recomb_rates' key. Using default rate of 3")
            rates = np.repeat(3, len(self.chrs_ids))
        assert isinstance(snp_position, str), "expected a string!"
        parts = snp_position.split(",")
        assert len(parts) >= 2, "input should be 'chr1,1000' or 'chr1,1000,2000'"
        where = int(parts[1]) if len(parts) == 2 else (int(parts[1]) + int(parts[2])) / 2
        return rates[self.get_chr_ind(str(parts[0]))] * where / 1000000

    def _check(self, ids, what):
        assert len(ids) <= len(self.chrs_ids), _MISMATCH
        shared = np.intersect1d(ids, self.chrs_ids)
        assert len(shared) > 0, _MISMATCH
        if len(shared) < len(self.chrs_ids):
            log.warning("Some reference contigs are missing in " + what)

    def get_bins_genome(self, g, binLen):
        """windows over the DB: ``g`` exposes ``chrs``, ``chr_regions`` (row range per chromosome), ``positions``"""
        db_ids = _bare(g.chrs)
        self._check(db_ids, "genotype hdf5 file")
        positions = np.asarray(g.positions)
        row0 = 0
        for chr_ix, cid in enumerate(self.chrs_ids):
            where = np.flatnonzero(db_ids == cid)
            if len(where):
                row0, row1 = int(g.chr_regions[where[0]][0]), int(g.chr_regions[where[0]][1])
                here = positions[row0:row1]
            else:
                here = positions[:0]            # chromosome absent from the DB: windows without members
            for span, members in get_bins_echr(self.chrlen[chr_ix], here, binLen, row0):
                yield (chr_ix, span, members)

    def get_bins_arrays(self, g_chrs, g_snppos, binLen):
        """windows over a sample given as parallel chromosome / position arrays"""
        ids = _bare(g_chrs)
        self._check(np.unique(ids), "given SNPs")
        g_snppos = np.asarray(g_snppos)
        for chr_ix, cid in enumerate(self.chrs_ids):
            mine = np.flatnonzero(ids == cid)
            offset = int(mine[0]) if len(mine) else 0
            for span, members in get_bins_echr(self.chrlen[chr_ix], g_snppos[mine], binLen, offset):
                yield (chr_ix, span, members)

    def get_window_rows(self, g, binLen):
        """The windows of ``get_bins_genome(g, binLen)`` as arrays, in its order, without the member lists: ``(chr_ix, start, end,
        first, last)``, int64 [n_windows] each -- window k of the genome covers positions start[k] .. end[k] of chromosome
        chr_ix[k] and holds the DB rows first[k] .. last[k] - 1 (two ``searchsorted`` calls per chromosome).  The windows of a
        chromosome follow each other in the rows: ``first[k + 1] == last[k]``.  A chromosome that the DB does not have gives
        windows without rows (first == last == 0); DB rows past the last window of their chromosome, and rows of a chromosome
        this genome does not have, are in no window.  The positions of a chromosome must be sorted and >= 1 (the member lists of
        ``get_bins_genome`` also serve other inputs)."""
        db_ids = _bare(g.chrs)
        self._check(db_ids, "genotype hdf5 file")
        positions, binLen = np.asarray(g.positions), int(binLen)
        parts = []
        for chr_ix, cid in enumerate(self.chrs_ids):
            starts = np.arange(1, int(self.chrlen[chr_ix]), binLen, dtype=np.int64)
            where = np.flatnonzero(db_ids == cid)
            if len(where):
                row0, row1 = int(g.chr_regions[where[0]][0]), int(g.chr_regions[where[0]][1])
                here = positions[row0:row1]
                if len(here) and (here[0] < 1 or bool(np.any(np.diff(here) < 0))):
                    raise ValueError("the positions of chromosome %s are not sorted (or below 1): its windows are not row ranges" % self.chrs[chr_ix])
                first = np.searchsorted(here, starts, side="left").astype(np.int64) + row0
                last = np.searchsorted(here, starts + (binLen - 1), side="right").astype(np.int64) + row0
            else:
                first = last = np.zeros(len(starts), dtype=np.int64)
            parts.append((np.full(len(starts), chr_ix, dtype=np.int64), starts, starts + (binLen - 1), first, last))
        return tuple(np.concatenate([p[k] for p in parts]) if parts else np.zeros(0, dtype=np.int64) for k in range(5))

    def window_table(self, binLen):
        """(chr_ix, start, end) of every window of the genome, in iteration order"""
        return [(c, s, s + int(binLen) - 1) for c in range(len(self.chrs_ids))
                for s in range(1, int(self.chrlen[c]), int(binLen))]
