"""shared by the genotype_cross_hmm tests: the golden cases (tests/golden/ghmm_*.npz, written by make_golden_ghmm.py from the
unmodified reference), a writer for the multi-sample VCF a case describes (GT:DP per sample), and random inputs for
``snpm_cross_hmm`` with their numpy-twin results (made once per shape, kept unchanged)"""
import gzip

import numpy as np

import ghmm_twin
from gcross_util import DuckGenotype, load, write_genome  # noqa: F401  (the same duck-typed DB and genome writer)
from snpmatch_amd.core import infer

CASES = ["ghmm_a_f2", "ghmm_b_phasing", "ghmm_c_multiallelic", "ghmm_d_het_parents", "ghmm_e_extremes", "ghmm_f_no_rates",
         "ghmm_g_short_chains"]


def write_vcf(path, chrom, pos, gt, dp, samples, fmt="GT:DP"):
    """a multi-sample VCF holding exactly these records, every sample entry ``GT:DP`` (``path`` ending in .gz: gzip)"""
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "wt") as fh:
        fh.write("##fileformat=VCFv4.2\n")
        fh.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(str(s) for s in samples) + "\n")
        for c, p, row, depth in zip(chrom, pos, gt, dp):
            fh.write("%s\t%d\t.\tA\tT\t50\tPASS\tDP=21\t%s\t%s\n" % (c, p, fmt, "\t".join("%s:%d" % (g, d) for g, d in zip(row, depth))))
    return path


def golden_lines(case, monkeypatch, tmp_path, step, vcf_name="f2.vcf"):
    """the package's lines for a golden case: VCF file -> reader -> host layer, ``step`` where the device call would be"""
    from snpmatch_amd.core import genomes, genotype_cross
    monkeypatch.setattr(genotype_cross, "genome", genomes.Genome(write_genome(case, str(tmp_path / "genome.json"))))
    if step is not None:
        monkeypatch.setattr(genotype_cross, "viterbi_paths", step)
    vcf = write_vcf(str(tmp_path / vcf_name), case["vcf_chr"], case["vcf_pos"], case["vcf_gt"], case["vcf_dp"], case["samples"])
    cross = genotype_cross.GenotypeCross(DuckGenotype(case), str(case["parents"]), 0, None, False)
    return cross.genotype_cross_hmm(vcf)


_random = {}


def random_case(n_samples, sizes, n_depth=7, minus_inf=False, seed=0):
    """(padded codes, padded depth ranks, pair, chain_off, logT, logI, logE, twin state, twin omega) for chains of the given
    sizes.  The tables are real ones (``infer.emission_tables`` at depths 0 .. n_depth - 1, transition matrices of different
    recombination fractions); ``minus_inf``: no transition of every second chain leads into AB (log 0 = -inf, which then reaches omega).
    Odd samples are phased and 10 % of all calls use the other separator, also in a chain's first row."""
    key = (n_samples, tuple(sizes), n_depth, minus_inf, seed)
    if key not in _random:
        rng = np.random.default_rng(hash(key) % (2**32))
        chain_off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
        n, n_chain = int(chain_off[-1]), len(sizes)
        cls = rng.choice(np.array([0, 1, 2, 3, 4]), size=(n, n_samples), p=[0.3, 0.3, 0.2, 0.15, 0.05])
        bar = (np.arange(n_samples)[None, :] % 2 == 1) ^ (rng.random((n, n_samples)) < 0.10)
        codes = np.full((n, n_samples + 5), 0xEE, dtype=np.uint8)
        codes[:, :n_samples] = cls | (bar.astype(np.int64) << 3)
        rank = np.full((n, n_samples + 5), 0xEEEE, dtype=np.uint16)
        rank[:, :n_samples] = rng.integers(0, n_depth, size=(n, n_samples))
        pair = rng.integers(0, 6, size=n).astype(np.uint8)
        _, logI, logE = infer.emission_tables(np.arange(n_depth, dtype=np.float64), 0.036)
        logT = np.empty((n_chain, 3, 3))
        for c in range(n_chain):
            frame = infer._transition_frame(1.0 + c, max(int(sizes[c]), 1) + 3, 3.5).values
            if minus_inf and c % 2 == 0:
                frame = frame.copy()
                frame[:, 1] = 0.0
            logT[c] = infer.log_transition(frame)
        state, omega = ghmm_twin.cross_hmm(codes[:, :n_samples], rank[:, :n_samples], pair, chain_off, logT, logI, logE)
        out = (codes, rank, pair, chain_off, logT, logI, logE, state, omega)
        for a in out:
            a.flags.writeable = False
        _random[key] = out
    return _random[key]
