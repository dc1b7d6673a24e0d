"""
The HMM behind ``genotype_cross_hmm``: ancestry (AA / AB / BB) of an F2 individual along one chromosome from its calls at
the markers where the parents differ, by a 3-state Viterbi.

Public surface follows the part of the reference module ``snpmatch.core.infer`` this path uses (core/infer.py:17-58, :173-358):
``viterbi``, ``IdentifyAncestryF2individual`` (``params``, ``init_prob``, ``transition_prob``, ``emission_prob``, ``viterbi``,
``snp_to_observations``), ``get_af``, ``polarize_snps`` and ``uniq_neighbor``.  The 2-state model of the reference
(``IdentifyStrechesofHeterozygosity``) is called by no command and is not provided.

Division of labour.  Every probability and every logarithm is computed HERE, on the host, by numpy, with the reference's
expressions on the reference's operand types -- ``pow`` through scalars, the 3x3 by 3x4 product through ``np.dot``, ``np.log`` on
a scalar (emissions), on a column of the transition matrix and on the 3-vector ``init x emission`` -- so that the values are the
reference's bit for bit.  The recurrence itself (fp64 additions in the reference's association, first-maximum comparisons, the
backtrack) runs on the device: ``engine.cross_hmm`` -> ``k_ghmm``, one lane per chain.

An emission matrix depends on the ordered parental pair (``PAIRS``), on ``rint(depth)`` and on nothing else, so a job needs one
table ``[pair][depth rank][observation][state]`` however many markers and samples it has (``emission_tables``).
"""
import logging

import numpy as np
import numpy.ma
import pandas as pd

log = logging.getLogger(__name__)

ANCESTRY = ['AA', 'AB', 'BB']
OBSERVED = ['00', '01', '11', 'NA']
INIT_PROB = [0.25, 0.5, 0.25]                    # an F2 individual under Mendelian segregation
# the ordered pairs of distinct parental calls (0 hom-ref, 1 hom-alt, 2 het), in the order the device tables are indexed
PAIRS = [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]
_OBS_TO_CLASS = np.array([0, 2, 1, 3], dtype=np.uint8)       # observation -> class bits of a call code (k_ghmm maps back)


def pair_index(snps_p1, snps_p2):
    """uint8 index into ``PAIRS`` of every marker; the parents must differ and be 0 / 1 / 2"""
    p1, p2 = np.asarray(snps_p1).astype(np.int64), np.asarray(snps_p2).astype(np.int64)
    assert np.all((p1 >= 0) & (p1 <= 2) & (p2 >= 0) & (p2 <= 2) & (p1 != p2)), "parental calls must be 0, 1 or 2 and differ"
    return (2 * p1 + p2 - (p2 > p1)).astype(np.uint8)


def get_af(snps):
    """alternative-allele frequency of a call: 0 -> 0, 1 (hom-alt) -> 1, 2 (het) -> 0.5"""
    calls = np.copy(snps)
    return np.where(calls == 1, 2, np.where(calls == 2, 1, calls)) / 2


def _emission_given_af(error_p1, error_p2, af_p1, af_p2, base_error, avg_depth):
    """P(observation | ancestry) as a [3, 4] array: P(genotype | ancestry) [3, 3] times P(observation | genotype) [3, 4]
    (the model of Andolfatto et al. as the reference writes it, core/infer.py:231-281: same operations, same order)"""
    depth = np.rint(avg_depth)
    ok1, ok2 = 1 - error_p1, 1 - error_p2
    # both alleles from parent 1 (AA), both from parent 2 (BB), one from each (AB): chance of genotype 00 and of 11
    aa00 = (ok1**2 * (1 - af_p1)) + (error_p1**2 * af_p1)
    aa11 = (ok1**2 * af_p1) + (error_p1**2 * (1 - af_p1))
    bb00 = (ok2**2 * (1 - af_p2)) + (error_p2**2 * af_p2)
    bb11 = (ok2**2 * af_p2) + (error_p2**2 * (1 - af_p2))
    ab00 = (((1 - af_p1) * ok1) + (af_p1 * error_p1)) * (((1 - af_p2) * ok2) + (af_p2 * error_p2))
    ab11 = ((af_p1 * ok1) + ((1 - af_p1) * error_p1)) * ((af_p2 * ok2) + ((1 - af_p2) * error_p2))
    genotype = [[aa00, 1 - aa00 - aa11, aa11], [ab00, 1 - ab11 - ab00, ab11], [bb00, 1 - bb00 - bb11, bb11]]
    # what `depth` reads show of a homozygous and of a heterozygous genotype
    same = (1 - base_error)**depth
    other = base_error**depth
    mixed = 1 - same - other
    het_seen = 1 - 2 * (0.5**depth)
    het_hidden = (1 - het_seen) / 2
    seen = [[same, mixed, other, 1], [het_hidden, het_seen, het_hidden, 1], [other, mixed, same, 1]]
    if depth <= 0:
        seen = np.ones((3, 4), dtype=float)
    return np.dot(np.array(genotype), np.abs(np.array(seen)))


def _transition_frame(chromosome_size, num_markers, recomb_rate):
    ri = (float(chromosome_size) / num_markers) * recomb_rate / 100
    rows = [[(1 - ri)**2, 2 * ri * (1 - ri), ri**2],
            [ri * (1 - ri), (1 - ri)**2 + ri**2, ri * (1 - ri)],
            [ri**2, 2 * ri * (1 - ri), (1 - ri)**2]]
    return pd.DataFrame(rows, index=ANCESTRY, columns=ANCESTRY)


def log_transition(trans_mat):
    """[3, 3] log of a transition matrix, column by column as the recurrence takes it (``np.log(trans_mat[:, j])``)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.stack([np.log(trans_mat[:, j]) for j in range(trans_mat.shape[1])], axis=1)


def log_emission(init_prob, emission):
    """(logI, logE), each [4, 3] = [observation][state], of one [3, 4] emission matrix: ``np.log(init_prob * E[:, o])`` and the
    scalar ``np.log(E[j, o])`` of the recurrence"""
    n_state, n_obs = emission.shape
    log_i, log_e = np.empty((n_obs, n_state)), np.empty((n_obs, n_state))
    with np.errstate(divide="ignore", invalid="ignore"):
        for o in range(n_obs):
            log_i[o] = np.log(init_prob * emission[:, o])
            for j in range(n_state):
                log_e[o, j] = np.log(emission[j, o])
    return log_i, log_e


def emission_tables(depth_levels, base_error, error_p1=0.00001, error_p2=0.00001, init_prob=INIT_PROB):
    """The tables of one job: ``E`` [6, n_depth, 3, 4] (probabilities, [state][observation]), ``logI`` and ``logE`` [6, n_depth,
    4, 3] ([observation][state]) for the six ``PAIRS`` and the given depths (already rounded: ``np.rint``)."""
    depth_levels = np.asarray(depth_levels, dtype=np.float64)
    emission = np.empty((len(PAIRS), len(depth_levels), 3, 4))
    log_i = np.empty((len(PAIRS), len(depth_levels), 4, 3))
    log_e = np.empty_like(log_i)
    for k, (one, two) in enumerate(PAIRS):
        af1, af2 = get_af(np.float64(one)), get_af(np.float64(two))
        for d, depth in enumerate(depth_levels):
            emission[k, d] = _emission_given_af(error_p1, error_p2, af1, af2, base_error, depth)
            log_i[k, d], log_e[k, d] = log_emission(init_prob, emission[k, d])
    return emission, log_i, log_e


def viterbi(init_prob, trans_mat, emission_mat, obs):
    """(path, omega) of one chain: ``path`` float [T] the most probable states, ``omega`` [T, 3] the log probabilities of the best
    path into every state (core/infer.py:17-58).  3 states and 4 observation symbols (the model of this module); ``emission_mat``
    [3, 4] or [3, 4, T].  The tables are built here, the recurrence runs on the device (one chain, one lane)."""
    from .. import engine
    obs = np.asarray(obs)
    trans_mat, emission_mat = np.asarray(trans_mat, dtype=np.float64), np.asarray(emission_mat, dtype=np.float64)
    n = obs.shape[0]
    if trans_mat.shape != (3, 3) or emission_mat.shape[:2] != (3, 4):
        raise ValueError("viterbi serves the 3-state, 4-symbol model of IdentifyAncestryF2individual only")
    assert n >= 1 and np.all((obs >= 0) & (obs <= 3)), "observations are 0 ('00'), 1 ('01'), 2 ('11') or 3 ('NA')"
    if emission_mat.ndim == 2:
        emission_mat = np.tile(emission_mat.T, (n, 1, 1)).T
    # one table entry per distinct emission matrix of the chain, addressed through the depth rank of pair 0
    flat = np.ascontiguousarray(np.moveaxis(emission_mat, 2, 0)).reshape(n, 12)
    levels, rank = np.unique(flat.view(np.uint64), axis=0, return_inverse=True)
    assert len(levels) <= 65536, "more than 65536 distinct emission matrices in one chain"
    log_i = np.zeros((len(PAIRS), len(levels), 4, 3))
    log_e = np.zeros_like(log_i)
    for d, bits in enumerate(levels):
        log_i[0, d], log_e[0, d] = log_emission(init_prob, bits.view(np.float64).reshape(3, 4))
    log_t = log_transition(trans_mat) if n > 1 else np.zeros((3, 3))
    if np.isnan(log_t).any() or np.isnan(log_i).any() or np.isnan(log_e).any():
        raise ValueError("a probability of the model is negative or NaN: its logarithm is not a number")
    codes = _OBS_TO_CLASS[obs.astype(np.int64)].reshape(n, 1)
    state, omega = engine.cross_hmm(engine.default_context(), codes, np.asarray(rank, dtype=np.uint16).reshape(n, 1), np.zeros(n, dtype=np.uint8),
                                    [0, n], log_t[None], log_i, log_e, return_omega=True)
    return (state[:, 0].astype(float), omega[:, 0, :])


class IdentifyAncestryF2individual(object):

    def __init__(self, chromosome_size, snps_p1, snps_p2, recomb_rate=3.5, error_p1=0.00001, error_p2=0.00001, base_error=0.01,
                 sample_depth=1.5):
        """``chromosome_size`` in Mb, ``recomb_rate`` in cM / Mb, ``snps_p1`` / ``snps_p2`` the parents' calls at the markers,
        ``sample_depth`` one number or one per marker"""
        self.ancestry = list(ANCESTRY)
        self.geno_parents = ['00', '01', '11']
        self.observed_states = list(OBSERVED)
        snps_p1, snps_p2 = np.asarray(snps_p1), np.asarray(snps_p2)
        assert snps_p1.shape[0] == snps_p2.shape[0], "both the SNP arrays for two parents should be of same size"
        num_markers = snps_p1.shape[0]
        if isinstance(sample_depth, (int, float)):
            sample_depth = np.repeat(sample_depth, num_markers)
        self.params = {'num_markers': num_markers, 'chromosome_size': chromosome_size, 'recomb_rate': recomb_rate, 'error_p1': error_p1,
                       'error_p2': error_p2, 'snps_p1': snps_p1, 'snps_p2': snps_p2, 'base_error': base_error,
                       'sample_depth': sample_depth}
        self.init_prob = list(INIT_PROB)
        self.transition_prob = self._transition_prob(chromosome_size, num_markers, recomb_rate)
        self.emission_prob = self._get_emissions(error_p1, error_p2, snps_p1, snps_p2, base_error, sample_depth)

    def _get_emissions(self, error_p1, error_p2, snps_p1, snps_p2, base_error, sample_depth):
        """[3, 4, num_markers]: one emission matrix per distinct (parent 1, parent 2, rounded depth), placed at its markers"""
        depth = np.rint(np.asarray(sample_depth, dtype=np.float64))
        out = np.zeros((len(self.ancestry), len(self.observed_states), len(snps_p1)))
        keys = np.stack([np.asarray(snps_p1, dtype=np.float64), np.asarray(snps_p2, dtype=np.float64), depth], axis=1)
        for one, two, d in np.unique(keys, axis=0) if len(keys) else ():
            here = np.flatnonzero((keys[:, 0] == one) & (keys[:, 1] == two) & (keys[:, 2] == d))
            out[:, :, here] = self._calc_emission_given_af(error_p1, error_p2, get_af(one), get_af(two), base_error, d).values[:, :, None]
        return out

    def _calc_emission_given_af(self, error_p1, error_p2, af_p1, af_p2, base_error, avg_depth):
        return pd.DataFrame(_emission_given_af(error_p1, error_p2, af_p1, af_p2, base_error, avg_depth), index=self.ancestry,
                            columns=self.observed_states)

    def _transition_prob(self, chromosome_size, num_markers, recomb_rate):
        return _transition_frame(chromosome_size, num_markers, recomb_rate)

    def viterbi(self, input_snps):
        return viterbi(self.init_prob, self.transition_prob.values, self.emission_prob, self.snp_to_observations(input_snps))

    @staticmethod
    def snp_to_observations(input_snps):
        """calls (0 hom-ref, 1 hom-alt, 2 het, -1 none) -> observation symbols 0 '00', 1 '01', 2 '11', 3 'NA'"""
        calls = np.copy(input_snps)
        return np.where(calls == -1, 3, np.where(calls == 2, 1, np.where(calls == 1, 2, calls)))


def polarize_snps(input_snps, snps_p1, snps_p2, polarize_to=None):
    """calls as parental classes: 0 like parent 1, 2 like parent 2, 1 heterozygous where the parents' homozygous calls differ,
    3 otherwise.  Only homozygous parental calls (0 / 1) and called sample genotypes take part.  ``polarize_to`` 'p1' / 'p2':
    every homozygous call that is not that parent's counts as the other parent."""
    num_snps = len(input_snps)
    out = np.repeat(3, num_snps)
    calls = numpy.ma.masked_less(input_snps, 0)
    one = numpy.ma.masked_less(numpy.ma.masked_greater(snps_p1, 1), 0)
    two = numpy.ma.masked_less(numpy.ma.masked_greater(snps_p2, 1), 0)
    if polarize_to == "p1":
        out[np.where(np.equal(calls, one))[0]] = 0
        out[np.where((~np.equal(calls, one)) & (calls < 2))[0]] = 2
    elif polarize_to == "p2":
        out[np.where(np.equal(calls, two))[0]] = 2
        out[np.where((~np.equal(calls, two)) & (calls < 2))[0]] = 0
    else:
        out[np.where(np.equal(calls, one))[0]] = 0
        out[np.where(np.equal(calls, two))[0]] = 2
    out[np.where(np.equal(calls, np.repeat(2, num_snps)) & (one != two))[0]] = 1
    return out


def uniq_neighbor(a):
    """run-length form of a 1-d array: (value of every run, its length) -- recombination break points of a path"""
    a = np.asarray(a)
    if len(a) == 0:
        return (np.array([], dtype=a.dtype), np.array([], dtype=int))
    starts = np.concatenate(([0], np.flatnonzero(a[1:] != a[:-1]) + 1))
    return (a[starts], np.diff(np.concatenate((starts, [len(a)]))).astype(int))
