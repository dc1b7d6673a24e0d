"""
``snpmatch mosaic``: a sample painted as a MOSAIC of the accessions of the database -- which accession it copies at every matched
SNP -- for samples made of more than two sources: MAGIC lines, multi-parent RILs, admixed or outcrossed field samples, a stock
whose tray was mixed up half-way through a crossing scheme.  ``inbred`` assumes one accession for the whole genome and reports
several weak hits for such a sample; ``cross`` / ``f1search`` assume an F1 of two, ``parentsearch`` two parents along the genome.

The model is the copying model of Li & Stephens with a uniform switch cost, as a Viterbi path with integer costs (so that device,
numpy twin and a brute-force DP agree bit for bit): the states are ALL the candidate accessions; a matched SNP costs
``cost[sample class][DB code]`` in the accession the path is in, a change of accession costs ``--switch_cost``, a chromosome is a
chain of its own.  ``include/snpmatch_hip.h`` (``snpm_panel_mosaic``) states the recurrence and its tie rules.  One device call
(``Genotype.mosaic`` -> ``engine.mosaic`` -> ``snpm_panel_mosaic``) paints every sample of the input on every chromosome.

The steps, after ``f1search``: the sample is intersected with the DB (``get_positions_idxs``), its hard calls become classes
(``f1search.hard_classes``), the matched rows -- in DB order -- are cut into chains at chromosome boundaries, the device paints,
and the states are run-length encoded into segments.  A multi-sample VCF is a batch on its shared records, read the way
``pairsnp-batch`` reads its cohort; a sample without a call at a record has no class there (0xFF: the record costs it nothing).

The cost table of the flags: equal codes 0, homozygous against the other homozygous ``--mismatch``, heterozygous against
homozygous either way ``--het_cost``, the DB's "other" code ``--mismatch``.

The reference has no such command: the files and the parameters are this package's own.

  <prefix>.mosaic.segments.tsv   sample, chr, first_pos, last_pos, accession, sites, cost, short: a line per segment, ``cost`` the
                                 mismatch cost inside it; ``short`` is 1 for a segment of fewer than ``--min_seg_sites`` sites
                                 (flagged, not dropped)
  <prefix>.mosaic.json           per sample: the accessions by their share of the matched sites, the total cost, the switches, the
                                 best SINGLE accession with its cost (what the mosaic gains over ``inbred``), and the parameters
  <prefix>.mosaic.npz            samples, state (int32 [n_samples, n_rows]: indices into ``columns``), chain_cost, chain_off, rows
                                 (DB rows), columns (DB accession indices), accessions (their names)
"""
import json
import logging

import numpy as np

from . import _select, f1search, snp_genotype
from ._select import read_samples  # noqa: F401  (the name tests and tools import)

log = logging.getLogger(__name__)

SWITCH_COST = 40            # default of --switch_cost
MISMATCH = 2                # default of --mismatch
HET_COST = 1                # default of --het_cost
MIN_SEG_SITES = 20          # default of --min_seg_sites
SWITCH_MAX = 1 << 20
NO_CLASS = f1search.NO_CLASS


def cost_table(mismatch=MISMATCH, het_cost=HET_COST):
    """cost [3, 4] uint8, [sample class 0 ref, 1 alt, 2 het][DB code 0, 1, 2, 3 = other]"""
    mismatch, het_cost = int(mismatch), int(het_cost)
    for name, v in (("--mismatch", mismatch), ("--het_cost", het_cost)):
        if not 0 <= v <= 15:
            raise ValueError("%s must be 0 .. 15, got %d" % (name, v))
    m, h = mismatch, het_cost
    return np.array([[0, m, h, m], [m, 0, h, m], [h, h, 0, m]], dtype=np.uint8)


def check_switch_cost(switch_cost):
    switch_cost = int(switch_cost)
    if not 1 <= switch_cost <= SWITCH_MAX:
        raise ValueError("--switch_cost must be 1 .. %d, got %d" % (SWITCH_MAX, switch_cost))
    return switch_cost


def chains_of(db_rows, chr_regions):
    """chain_off [n_chr + 1] of ascending DB rows: chain c holds the rows inside chromosome region c of the DB"""
    regions = np.asarray(chr_regions, dtype=np.int64).reshape(-1, 2)
    db_rows = np.asarray(db_rows, dtype=np.int64)
    off = np.searchsorted(db_rows, np.append(regions[:, 0], regions[-1, 1] if len(regions) else 0))
    off[0], off[-1] = 0, len(db_rows)
    return np.maximum.accumulate(off).astype(np.int64)


def segments_of(state, chain_off):
    """Run-length encoding of one sample's states: int64 [n_seg, 4] of (chain, first row, last row, state), rows as positions in
    the matched rows, in order; a segment never crosses a chain boundary"""
    state = np.asarray(state).reshape(-1)
    chain_off = np.asarray(chain_off, dtype=np.int64)
    out = []
    for c in range(len(chain_off) - 1):
        c0, c1 = int(chain_off[c]), int(chain_off[c + 1])
        if c1 <= c0:
            continue
        st = state[c0:c1]
        starts = np.append(0, np.flatnonzero(st[1:] != st[:-1]) + 1)
        ends = np.append(starts[1:], c1 - c0) - 1
        out.extend((c, c0 + int(a), c0 + int(b), int(st[a])) for a, b in zip(starts, ends))
    return np.array(out, dtype=np.int64).reshape(-1, 4)


def write_segments(path, samples, segs, seg_costs, chr_names, positions, acc_names, min_seg_sites=MIN_SEG_SITES):
    """``<prefix>.mosaic.segments.tsv``.  segs / seg_costs: per sample the array of ``segments_of`` and the cost inside every
    segment; positions: bp of every matched row; acc_names: the name of every state"""
    with open(path, "w") as out:
        out.write("sample\tchr\tfirst_pos\tlast_pos\taccession\tsites\tcost\tshort\n")
        for name, sg, costs in zip(samples, segs, seg_costs):
            for (c, k0, k1, st), cost in zip(np.asarray(sg).tolist(), np.asarray(costs).tolist()):
                sites = k1 - k0 + 1
                out.write("%s\t%s\t%d\t%d\t%s\t%d\t%d\t%d\n" % (name, chr_names[c], int(positions[k0]), int(positions[k1]), acc_names[st], sites,
                                                           cost, 1 if sites < int(min_seg_sites) else 0))


class Mosaic(object):
    """``samples`` [n_samples] names, ``chrs`` / ``pos`` [n_records] the shared records, ``gt`` [n_records, n_samples] genotype
    text.  ``acc_ix``: the candidate accessions (None: all); ``run=False`` leaves the steps to the caller."""

    def __init__(self, samples, chrs, pos, gt, g, output_id="mosaic", switch_cost=SWITCH_COST, mismatch=MISMATCH, het_cost=HET_COST,
                 min_seg_sites=MIN_SEG_SITES, acc_ix=None, run=True):
        self.samples = [str(s) for s in samples]
        self.chrs, self.pos = np.asarray(chrs), np.asarray(pos)
        self.gt = np.asarray(gt).reshape(len(self.pos), -1)
        assert self.gt.shape[1] == len(self.samples), "one genotype column per sample"
        self.g, self.output_id = g, output_id
        self.switch_cost = check_switch_cost(switch_cost)
        self.cost = cost_table(mismatch, het_cost)
        self.mismatch, self.het_cost, self.min_seg_sites = int(mismatch), int(het_cost), int(min_seg_sites)
        if self.min_seg_sites < 0:
            raise ValueError("--min_seg_sites must not be negative, got %d" % self.min_seg_sites)
        self.acc_ix = None if acc_ix is None else np.asarray(acc_ix, dtype=np.int64).reshape(-1)
        if run:
            self.paint()
            self.write_outputs()

    def paint(self):
        # 1. the matched rows, in DB order
        db_rows, rec_rows = self.g.get_positions_idxs(self.chrs, self.pos)
        order = np.argsort(db_rows, kind="stable")
        self.db_rows, self.rec_rows = np.asarray(db_rows, dtype=np.int64)[order], np.asarray(rec_rows, dtype=np.int64)[order]
        # 2. the hard calls of every sample at them
        self.classes = np.stack([f1search.hard_classes(self.gt[:, s])[self.rec_rows] for s in range(len(self.samples))]) if len(self.samples) \
            else np.zeros((0, len(self.db_rows)), dtype=np.uint8)
        # 3. a chain per chromosome of the DB
        self.chain_off = chains_of(self.db_rows, self.g.g.chr_regions)
        # 4. the one device call
        self.columns = np.arange(len(self.g.accessions), dtype=np.int64) if self.acc_ix is None else self.acc_ix
        self.state, self.chain_cost, self.col_cost = self.g.mosaic(self.classes, self.chain_off, self.cost, self.switch_cost, self.acc_ix, self.db_rows,
                                                                   want_col_cost=True)
        # 5. segments, and the cost inside each: the segments of a sample as chains over the accessions it uses, never switching
        self.segs, self.seg_costs = [], []
        for s in range(len(self.samples)):
            sg = segments_of(self.state[s], self.chain_off)
            costs = np.zeros(len(sg), dtype=np.int64)
            if len(sg):
                used, inv = np.unique(sg[:, 3], return_inverse=True)
                seg_off = np.append(sg[:, 1], len(self.db_rows))
                # (a segment ends where the next begins, or at a chain boundary that is the start of the next: rows between two
                # chains do not exist, so the starts and the row count are the offsets)
                _, _, cc = self.g.mosaic(self.classes[s], seg_off, self.cost, SWITCH_MAX, self.columns[used], self.db_rows, want_col_cost=True)
                costs = cc[0][np.arange(len(sg)), inv.reshape(-1)].astype(np.int64)
            self.segs.append(sg)
            self.seg_costs.append(costs)
        log.info("mosaic: %d samples, %d matched rows in %d chains, %d candidate accessions", len(self.samples), len(self.db_rows),
                 len(self.chain_off) - 1, len(self.columns))
        return self.state

    def summary(self):
        names = np.asarray(self.g.accessions).astype("U")[self.columns]
        n_rows = len(self.db_rows)
        out = {"parameters": {"switch_cost": self.switch_cost, "mismatch": self.mismatch, "het_cost": self.het_cost, "min_seg_sites": self.min_seg_sites,
                              "cost": self.cost.tolist()},
               "matched_rows": int(n_rows), "candidates": int(len(self.columns)), "chains": int(len(self.chain_off) - 1), "samples": {}}
        for s, name in enumerate(self.samples):
            sg = self.segs[s]
            counts = np.bincount(self.state[s], minlength=len(self.columns)) if n_rows else np.zeros(len(self.columns), dtype=np.int64)
            share = [{"accession": str(names[a]), "sites": int(counts[a]), "share": counts[a] / float(n_rows)}
                     for a in np.argsort(-counts, kind="stable") if counts[a] > 0]
            single = self.col_cost[s].sum(axis=0, dtype=np.int64)
            best = int(np.argmin(single)) if len(single) else None
            chains_used = len(np.unique(sg[:, 0])) if len(sg) else 0
            out["samples"][name] = {
                "classed_rows": int(np.count_nonzero(self.classes[s] != NO_CLASS)),
                "accessions": share, "total_cost": int(self.chain_cost[s].sum(dtype=np.int64)), "switches": int(len(sg) - chains_used),
                "segments": int(len(sg)), "short_segments": int(np.count_nonzero(sg[:, 2] - sg[:, 1] + 1 < self.min_seg_sites)) if len(sg) else 0,
                "best_single": None if best is None else {"accession": str(names[best]), "cost": int(single[best])}}
        return out

    def write_outputs(self):
        names = np.asarray(self.g.accessions).astype("U")[self.columns]
        chain_chr = np.asarray(self.g.chrs).astype("U")
        write_segments(self.output_id + ".mosaic.segments.tsv", self.samples, self.segs, self.seg_costs, chain_chr,
                       np.asarray(self.g.g.positions)[self.db_rows], names, self.min_seg_sites)
        self.stats = self.summary()
        with open(self.output_id + ".mosaic.json", "w") as out:
            json.dump(self.stats, out, indent=1, sort_keys=True)
            out.write("\n")
        np.savez(self.output_id + ".mosaic.npz", samples=np.array(self.samples, dtype="U"), state=self.state, chain_cost=self.chain_cost,
                 chain_off=self.chain_off, rows=self.db_rows, columns=self.columns, accessions=names)
        return self.stats


def potatoMosaic(args):
    """entry point of ``snpmatch mosaic``"""
    given = lambda key, default: default if args.get(key) is None else args[key]      # noqa: E731
    switch_cost = check_switch_cost(given('switch_cost', SWITCH_COST))
    mismatch, het_cost, min_seg = int(given('mismatch', MISMATCH)), int(given('het_cost', HET_COST)), int(given('min_seg_sites', MIN_SEG_SITES))
    cost_table(mismatch, het_cost)
    if min_seg < 0:
        raise ValueError("--min_seg_sites must not be negative, got %d" % min_seg)
    samples, chrs, pos, gt = read_samples(args['inFile'], args.get('logDebug', False))
    log.info("loading genotype files!")
    g = snp_genotype.Genotype(args['hdf5File'], args.get('hdf5accFile'))
    acc_ix, _ = _select.accessions_of(g, args)
    painted = Mosaic(samples, chrs, pos, gt, g, args['outFile'], switch_cost, mismatch, het_cost, min_seg, acc_ix)
    log.info("finished!")
    return painted.stats
