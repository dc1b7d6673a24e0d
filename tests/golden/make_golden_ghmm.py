#!/usr/bin/env python3
"""
Generate tests/golden/ghmm_*.npz by RUNNING THE UNMODIFIED REFERENCE ``GenotypeCross(...).genotype_cross_hmm(...)`` (SNPmatch
v5.0.1, looked for where make_golden_gcross.py looks for it) in the build container.  Run from the repo root:

    python tests/golden/make_golden_ghmm.py

How the reference is driven (nothing of it is modified or copied; the prelude is the one of make_golden_gcross.py, imported):
  * placeholder modules for ``allel``, ``h5py``, ``hmmlearn(.hmm)``;
  * ``parsers.import_vcf_file`` is replaced by a function that returns the prepared dict (``samples``, ``gt``, ``chr``, ``pos``,
    ``calldata/DP``);
  * ``g`` is duck-typed: ``accessions``, ``g_acc.snps`` / ``chromosomes`` / ``positions`` and the reference's own static
    ``Genotype.get_common_positions``;
  * ``genotype_cross.genome`` is a reference ``Genome`` built from a toy JSON file with BARE chromosome names ("1", "2", "3": the
    reference compares ``genome.chrs`` with ``genome.chrs_ids`` and finds no marker when the file says "Chr1");
  * the function's last two statements call ``pd.Series.append``, which pandas 2 no longer has: for the duration of the call a
    stand-in on the pandas side (``pd.concat([self, other], ignore_index=...)``) is installed, and removed afterwards.
``genotype_cross_hmm`` itself runs to its end this way: ``lines`` of every fixture are its return value.

It returns the states only.  The full ``omega`` of every chain, the transition matrix of every chromosome and the emission
matrices are recorded by a second pass that repeats by hand what lines 128-138 and 157-170 of the reference function do -- the
matched segregating markers, the low-coverage filter, the halved depths, one ``infer.IdentifyAncestryF2individual(...)`` per
(chromosome, kept sample) with the same arguments, ``.viterbi(parsers.parseGT(column))`` -- again with the reference's own classes
and functions; the states of that pass must equal the ones in ``lines``.

After the reference has spoken, this package's host layer runs on the same inputs with the numpy twin (tests/ghmm_twin.py) in the
place of the device call.  The generator ASSERTS that it reproduces the lines, that the twin's states and omega equal the
reference's bit for bit, and that the package's tables equal the reference's emission and transition probabilities bit for bit.
"""
import json
import os
import sys
import tempfile

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_gcross as base  # noqa: E402  (the prelude: placeholder modules, the reference on sys.path, logging off)
from make_golden_gcross import ACCESSIONS, CHR_LEN, PARENTS, CALL_TEXT, DuckGenotype, f2_sample, parental_calls, records  # noqa: E402

from snpmatch.core import genomes as ref_genomes  # noqa: E402
from snpmatch.core import genotype_cross as ref_gc  # noqa: E402
from snpmatch.core import infer as ref_infer  # noqa: E402
from snpmatch.core import parsers as ref_parsers  # noqa: E402
from snpmatch.core import snp_genotype as ref_sg  # noqa: E402

GENOME_RATES = {"ref_chrs": ["1", "2", "3"], "ref_chrlen": CHR_LEN, "recomb_rates": [3.4, 3.6, 4.25]}
GENOME_PLAIN = {"ref_chrs": ["1", "2", "3"], "ref_chrlen": CHR_LEN}
PAIRS = [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]


def make_panel(rng, per_chr=(160, 110, 60), p=(0.05, 0.5, 0.4, 0.05)):
    positions, regions, row = [], [], 0
    for n, length in zip(per_chr, CHR_LEN):
        positions.append(np.sort(rng.choice(np.arange(1, length + 1), size=n, replace=False)))
        regions.append((row, row + n))
        row += n
    snps = rng.choice(np.array([-1, 0, 1, 2], dtype=np.int8), size=(row, len(ACCESSIONS)), p=list(p))
    return snps, ["1", "2", "3"], regions, np.concatenate(positions).astype("i4")


def duck(panel):
    g = DuckGenotype(*panel)
    g.get_common_positions = ref_sg.Genotype.get_common_positions
    return g


def reference_genome(genome_json):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "toy_genome.json")
        with open(path, "w") as fh:
            json.dump(genome_json, fh)
        return ref_genomes.Genome(path)


def run_reference(panel, vcf, samples, gt, dp, genome_json):
    ref_gc.genome = reference_genome(genome_json)
    prepared = {"samples": np.array(samples, dtype="U"), "gt": gt, "chr": vcf[0], "pos": vcf[1], "calldata/DP": dp}
    ref_parsers.import_vcf_file = lambda **kw: prepared
    cross = ref_gc.GenotypeCross(duck(panel), PARENTS, 0, None, False)
    pd.Series.append = lambda self, other, ignore_index=False: pd.concat([self, other], ignore_index=ignore_index)
    try:
        lines = cross.genotype_cross_hmm("prepared.vcf")
    finally:
        del pd.Series.append
    return cross, np.array(list(lines), dtype="U")


def chain_level(cross, vcf, gt, dp, genome_json, min_na_per_sample=0.8):
    """omega, states, transition and emission matrices: lines 128-138 and 157-170 of the reference function, repeated by hand
    around the reference's own model class"""
    genome = ref_gc.genome
    g_chr_names = genome.chrs[pd.Series(cross.commonSNPsCHR, dtype=str).apply(genome.get_chr_ind)]
    seg = cross.g.get_common_positions(cross.commonSNPsCHR, cross.commonSNPsPOS, vcf[0], vcf[1])
    num_markers = seg[1].shape[0]
    samples_dp = dp[seg[1], :]
    kept = np.where((samples_dp <= 0).sum(axis=0) / float(num_markers) < min_na_per_sample)[0]
    samples_gt, samples_dp = gt[seg[1]][:, kept], samples_dp[:, kept] / 2
    rate = np.mean(np.array(genome.json['recomb_rates'])) if "recomb_rates" in genome.json.keys() else 3.5
    state = np.full((num_markers, len(kept)), -1, dtype=np.int8)
    omega = np.full((num_markers, len(kept), 3), np.nan)
    trans = np.full((len(genome.chrs_ids), 3, 3), np.nan)
    levels = np.unique(np.rint(samples_dp))
    emission = np.full((6, len(levels), 3, 4), np.nan)
    for k, (ec, eclen) in enumerate(zip(genome.chrs_ids, genome.chrlen)):
        rows = np.where(g_chr_names[seg[0]] == ec)[0]
        if len(rows) == 0:
            continue
        p1, p2 = cross.snpsP1[seg[0][rows]], cross.snpsP2[seg[0][rows]]
        for s in range(len(kept)):
            model = ref_infer.IdentifyAncestryF2individual(chromosome_size=eclen / 1000000, snps_p1=p1, snps_p2=p2, recomb_rate=rate,
                                                           base_error=0.036, sample_depth=samples_dp[rows, s])
            path, om = model.viterbi(ref_parsers.parseGT(samples_gt[rows, s]))
            state[rows, s], omega[rows, s] = np.array(path, dtype=int), om
            trans[k] = model.transition_prob.values
            for m in range(len(rows)):
                key = (PAIRS.index((int(p1[m]), int(p2[m]))), int(np.searchsorted(levels, np.rint(samples_dp[rows[m], s]))))
                seen = model.emission_prob[:, :, m]
                assert np.isnan(emission[key]).all() or np.array_equal(emission[key].view(np.uint64), seen.view(np.uint64).reshape(3, 4))
                emission[key] = seen
    assert not np.isnan(omega).any() and state.min() >= 0
    return {"kept": kept, "state": state, "omega": omega, "trans": trans, "depth_levels": levels, "emission": emission,
            "db_rows": seg[0], "vcf_rows": seg[1]}


def check_with_twin(name, panel, vcf, samples, gt, dp, genome_json, lines, ref):
    sys.path.insert(0, base.ROOT)
    sys.path.insert(0, os.path.join(base.ROOT, "tests"))
    import ghmm_twin
    from snpmatch_amd.core import genomes, genotype_cross, infer, parsers
    seen = {}

    def twin(*args):
        seen["state"], seen["omega"] = ghmm_twin.cross_hmm(*args)
        seen["args"] = args
        return seen["state"]

    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "toy_genome.json")
        with open(path, "w") as fh:
            json.dump(genome_json, fh)
        genotype_cross.genome = genomes.Genome(path)
    keep_reader, keep_step = parsers.import_vcf_calls, genotype_cross.viterbi_paths
    parsers.import_vcf_calls = lambda *a, **kw: {"samples": np.array(samples, dtype="U"), "chr": vcf[0], "pos": vcf[1],
                                                 "codes": parsers.gt_call_codes(gt), "calldata/DP": dp}
    genotype_cross.viterbi_paths = twin
    try:
        cross = genotype_cross.GenotypeCross(DuckGenotype(*panel), PARENTS, 0, None, False)
        mine = cross.genotype_cross_hmm("prepared.vcf")
    finally:
        parsers.import_vcf_calls, genotype_cross.viterbi_paths = keep_reader, keep_step
    assert list(mine) == list(lines), "%s: host layer + twin differ from the reference" % name
    # (panel chromosomes are in genome order in every fixture: the device order is the panel order)
    assert np.array_equal(seen["state"], ref["state"]), "%s: twin states differ" % name
    assert np.array_equal(seen["omega"].view(np.uint64), ref["omega"].view(np.uint64)), "%s: twin omega differs in its bits" % name
    codes, rank, pair, chain_off, logT, logI, logE = seen["args"]
    E, _, _ = infer.emission_tables(ref["depth_levels"], 0.036)
    have = ~np.isnan(ref["emission"])
    assert np.array_equal(E[have].view(np.uint64), ref["emission"][have].view(np.uint64)), "%s: emission tables differ" % name
    for k in range(len(chain_off) - 1):
        if chain_off[k + 1] - chain_off[k] >= 2:
            assert np.array_equal(logT[k].view(np.uint64), infer.log_transition(ref["trans"][k]).view(np.uint64)), "%s: transition differs" % name
    return seen


def write(name, panel, vcf, samples, gt, dp, genome_json):
    dp = np.asarray(dp, dtype=np.int32)
    cross, lines = run_reference(panel, vcf, samples, gt, dp, genome_json)
    ref = chain_level(cross, vcf, gt, dp, genome_json)
    states_in_lines = np.array([ln.split(",")[3:] for ln in lines[2:]], dtype=int).reshape(len(lines) - 2, len(ref["kept"]))
    assert np.array_equal(states_in_lines, ref["state"]), "%s: the chain-level pass differs from genotype_cross_hmm" % name
    seen = check_with_twin(name, panel, vcf, samples, gt, dp, genome_json, lines, ref)
    snps, chrs, regions, positions = panel
    out = os.path.join(HERE, name + ".npz")
    np.savez_compressed(out, panel=snps, positions=positions, chrs=np.array(chrs, dtype="U"), chr_regions=np.array(regions, dtype=np.int64),
                        accessions=ACCESSIONS, parents=np.array(PARENTS), vcf_chr=vcf[0], vcf_pos=vcf[1], vcf_gt=gt, vcf_dp=dp,
                        samples=np.array(samples, dtype="U"), genome_json=np.array(json.dumps(genome_json)), lines=lines,
                        kept=ref["kept"], state=ref["state"], omega=ref["omega"], trans=ref["trans"], depth_levels=ref["depth_levels"],
                        emission=ref["emission"], chain_off=np.asarray(seen["args"][3]))
    print("%-22s %6d bytes  %2d of %2d samples kept %4d markers in chains %s  states: %s  depth levels %d  pairs %s" % (
        name, os.path.getsize(out), len(ref["kept"]), len(samples), len(ref["state"]), np.diff(seen["args"][3]).tolist(),
        dict(zip(*np.unique(ref["state"], return_counts=True))), len(ref["depth_levels"]),
        np.unique(seen["args"][2]).tolist()))
    return ref


def depths(rng, shape, top=8):
    return rng.integers(0, top + 1, size=shape).astype(np.int32)


def main():
    rng = np.random.default_rng(20261018)
    panel = make_panel(rng)
    as_text = lambda calls: np.array([CALL_TEXT[int(v)] for v in calls], dtype="U3")      # noqa: E731

    # a. 16 F2-like individuals: recombination blocks, errors, no-calls, depths 0-8
    vcf = records(rng, panel, extra=45)
    one, two = parental_calls(panel, vcf[2])
    gt = np.stack([f2_sample(rng, vcf[0], one, two) for _ in range(16)], axis=1)
    write("ghmm_a_f2", panel, vcf, ["F2_%02d" % i for i in range(16)], gt, depths(rng, gt.shape), GENOME_RATES)

    # b. phasing: fully phased, 30 % of the calls with the other separator (both directions), unphased
    vcf = records(rng, panel, extra=45)
    one, two = parental_calls(panel, vcf[2])
    cols = [f2_sample(rng, vcf[0], one, two) for _ in range(4)]
    cols[0] = np.char.replace(cols[0], "/", "|")
    cols[1] = np.where(rng.random(len(cols[1])) < 0.3, np.char.replace(cols[1], "/", "|"), cols[1])
    cols[2] = np.where(rng.random(len(cols[2])) < 0.3, cols[2], np.char.replace(cols[2], "/", "|"))
    gt = np.stack(cols, axis=1)
    write("ghmm_b_phasing", panel, vcf, ["phased", "mixed_30_bar", "mixed_30_slash", "plain"], gt, depths(rng, gt.shape), GENOME_RATES)

    # c. multi-allelic calls sprinkled over 15 % of the calls
    vcf = records(rng, panel, extra=45)
    one, two = parental_calls(panel, vcf[2])
    cols = []
    for _ in range(5):
        col = f2_sample(rng, vcf[0], one, two).astype("U3")
        cols.append(np.where(rng.random(len(col)) < 0.15, rng.choice(np.array(["1/2", "0/2", "2/2", "1|2"]), size=len(col)), col))
    gt = np.stack(cols, axis=1)
    write("ghmm_c_multiallelic", panel, vcf, ["M%d" % i for i in range(5)], gt, depths(rng, gt.shape), GENOME_RATES)

    # d. heterozygous parents: a panel with 25 % heterozygous calls, all six ordered pairs among the markers
    het_panel = make_panel(rng, p=(0.05, 0.38, 0.32, 0.25))
    vcf = records(rng, het_panel, extra=45)
    one, two = parental_calls(het_panel, vcf[2])
    gt = np.stack([f2_sample(rng, vcf[0], one, two) for _ in range(6)], axis=1)
    ref = write("ghmm_d_het_parents", het_panel, vcf, ["H%d" % i for i in range(6)], gt, depths(rng, gt.shape), GENOME_RATES)
    assert (~np.isnan(ref["emission"][:, :, 0, 0])).any(axis=1).all(), "not all six parental pairs occur"

    # e. extremes: equal to parent 1, equal to parent 2, heterozygous everywhere, never called (but covered: AA and BB tie
    #    exactly at every step, argmax takes the first), an F2, and an individual without coverage at 90 % of the markers (dropped by the filter)
    vcf = records(rng, panel, extra=45)
    one, two = parental_calls(panel, vcf[2])
    filler = rng.choice([0, 1, 2], size=len(one))
    cols = [as_text(np.where(one >= 0, one, filler)), as_text(np.where(two >= 0, two, filler)), np.repeat("0/1", len(one)),
            np.repeat("./.", len(one)), f2_sample(rng, vcf[0], one, two), f2_sample(rng, vcf[0], one, two)]
    gt = np.stack(cols, axis=1)
    dp = depths(rng, gt.shape)
    dp[:, 3] = np.maximum(dp[:, 3], 1)
    dp[:, 5] = np.where(rng.random(len(one)) < 0.9, 0, dp[:, 5])
    ref = write("ghmm_e_extremes", panel, vcf, ["is_p1", "is_p2", "all_het", "no_calls", "f2", "low_cov"], gt, dp, GENOME_RATES)
    assert ref["kept"].tolist() == [0, 1, 2, 3, 4]
    assert np.array_equal(ref["omega"][:, 3, 0], ref["omega"][:, 3, 2]), "the never-called sample should tie AA and BB at every step"

    # f. a genome JSON without recomb_rates: 3.5 cM/Mb in the model, 3 in the printed genetic position
    vcf = records(rng, panel, extra=45)
    one, two = parental_calls(panel, vcf[2])
    gt = np.stack([f2_sample(rng, vcf[0], one, two) for _ in range(5)], axis=1)
    write("ghmm_f_no_rates", panel, vcf, ["R%d" % i for i in range(5)], gt, depths(rng, gt.shape), GENOME_PLAIN)

    # g. chains of 1, 2 and 3 markers: the VCF keeps that many matched segregating positions per chromosome (and its strangers)
    chrom, pos, rows = records(rng, panel, extra=45)
    one, two = parental_calls(panel, rows)
    drop = np.zeros(len(pos), dtype=bool)
    for name, wanted in (("Chr1", 1), ("Chr2", 2), ("Chr3", 3)):
        marker = np.flatnonzero((chrom == name) & (one >= 0))
        drop[rng.permutation(marker)[wanted:]] = True
    vcf = (chrom[~drop], pos[~drop], rows[~drop])
    one, two = one[~drop], two[~drop]
    gt = np.stack([f2_sample(rng, vcf[0], one, two, nocall=0.3) for _ in range(7)], axis=1)
    write("ghmm_g_short_chains", panel, vcf, ["T%d" % i for i in range(7)], gt, depths(rng, gt.shape, top=4), GENOME_RATES)


if __name__ == "__main__":
    main()
