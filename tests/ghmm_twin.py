"""numpy twin of ``snpm_cross_hmm`` / ``k_ghmm`` (test infrastructure): the 3-state Viterbi path and every step's omega of every
(chain, sample), vectorised over the sample axis, a loop over the markers of a chain.

Written from the rule:
  observation of an element = {0, 2, 1, 3, 0}[class] when its separator bit equals the one of the chain's first row of that sample,
  else 0;  table entry t = (pair, depth rank, observation);  omega[first] = logI[t];
  omega[r][j] = max_i ((omega[r - 1][i] + logT[i][j]) + logE[t][j]), backpointer = the FIRST i that reaches the maximum
  (``np.argmax``);  last state = first maximum of the last omega;  the path follows the backpointers downwards.
No logarithm is taken here either: the tables carry them (``snpmatch_amd.core.infer``).
"""
import numpy as np

CLASS_OBS = np.array([0, 2, 1, 3, 0, 0, 0, 0], dtype=np.int64)


def observations(codes, chain_off):
    """int64 [n, n_samples]: the observation symbol of every call under its chain's governing separator"""
    codes = np.asarray(codes, dtype=np.uint8)
    chain_off = np.asarray(chain_off, dtype=np.int64)
    first_row = np.repeat(chain_off[:-1], np.diff(chain_off))
    bar = (codes >> 3) & 1
    if len(codes) == 0:
        return np.zeros(codes.shape, dtype=np.int64)
    return np.where(bar == bar[first_row], CLASS_OBS[codes & 7], 0)


def cross_hmm(codes, depth_rank, pair, chain_off, logT, logI, logE):
    """(state int8 [n, n_samples], omega float64 [n, n_samples, 3])"""
    codes = np.asarray(codes, dtype=np.uint8)
    n, ns = codes.shape
    depth_rank = np.asarray(depth_rank).astype(np.int64)
    pair = np.asarray(pair).astype(np.int64)
    chain_off = np.asarray(chain_off, dtype=np.int64)
    logT, logI, logE = (np.asarray(a, dtype=np.float64) for a in (logT, logI, logE))
    obs = observations(codes, chain_off)
    state = np.zeros((n, ns), dtype=np.int8)
    omega = np.zeros((n, ns, 3), dtype=np.float64)
    back = np.zeros((n, ns, 3), dtype=np.int8)
    lanes = np.arange(ns)
    for c in range(len(chain_off) - 1):
        a, b = int(chain_off[c]), int(chain_off[c + 1])
        if a == b:
            continue
        omega[a] = logI[pair[a], depth_rank[a], obs[a]]
        for r in range(a + 1, b):
            e = logE[pair[r], depth_rank[r], obs[r]]                                     # [ns, 3 (target state)]
            cand = (omega[r - 1][:, :, None] + logT[c][None, :, :]) + e[:, None, :]      # [ns, source, target]
            back[r] = cand.argmax(axis=1)
            omega[r] = cand.max(axis=1)
        k = omega[b - 1].argmax(axis=1)
        state[b - 1] = k
        for r in range(b - 1, a, -1):
            k = back[r][lanes, k]
            state[r - 1] = k
    return state, omega
