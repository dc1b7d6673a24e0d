"""numpy twin of ``snpm_panel_sim_counts`` / ``k_sim_noise`` + ``k_sim_count`` (test infrastructure): the sample simulated from every
accession column scored against every accession column, per group of selected rows.  The hash is restated here with numpy uint64
arithmetic, independently of the ``__host__ __device__`` definition in csrc/snpm_k_sim.hpp; the indicator products run in fp64 through
BLAS (sums of 0/1 products far below 2^53: exact) and are converted to int32."""
import numpy as np

NO_CALL = 0xFF
_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def _mix(z):
    """the splitmix64 finaliser on a uint64 array (arithmetic modulo 2^64)"""
    z = (z ^ (z >> np.uint64(30))) * _M1
    z = (z ^ (z >> np.uint64(27))) * _M2
    return z ^ (z >> np.uint64(31))


def sim_hash(seed, a, k):
    """h(seed, a, k) for arrays a (column positions) and k (selected-row positions), broadcast against each other: one round of the
    finaliser over seed + 0x9E3779B97F4A7C15 (a + 1), the row position xor-ed in, a second round"""
    with np.errstate(over="ignore"):
        a = np.asarray(a, dtype=np.uint64)
        k = np.asarray(k, dtype=np.uint64)
        key = _mix(np.asarray(int(seed) % (1 << 64), dtype=np.uint64) + _GOLDEN * (a + np.uint64(1)))
        return _mix(key ^ k)


def err_threshold(err_rate):
    """floor(err_rate * 2^32), as ``engine.sim_counts`` maps it"""
    assert 0.0 <= err_rate <= 1.0
    return int(np.floor(err_rate * 4294967296.0))


def _selected(snps, cols, rows):
    v = np.asarray(snps)
    if rows is not None:
        v = v[rows, :]
    if cols is not None:
        v = v[:, np.asarray(cols, dtype=np.int64)]
    return v


def sample_classes(v, err_thr, seed):
    """uint8 [n_rows, n_cols]: the class of the sample simulated from column position a at selected-row position k (0 / 1 / 2), 0xFF
    where it has no call (the column's code there is not 0, 1 or 2).  ``v``: the SELECTED calls, int8 [n_rows, n_cols]."""
    n, nc = v.shape
    cls = np.where((v >= 0) & (v <= 2), v, NO_CALL).astype(np.uint8)
    if err_thr:
        h = sim_hash(seed, np.arange(nc)[None, :], np.arange(n)[:, None])
        hit = ((h >> np.uint64(32)) < np.uint64(err_thr)) & (cls != NO_CALL)
        drawn = (((h & np.uint64(0xFFFFFFFF)) * np.uint64(3)) >> np.uint64(32)).astype(np.uint8)
        cls = np.where(hit, drawn, cls)
    return cls


def sim_counts(snps, grp_off, err_thr, seed, cols=None, rows=None):
    """snps int8 [n_snp, n_acc] (negative = missing, 0 / 1 / 2, anything else one further class); grp_off [n_grp + 1] offsets into the
    selected rows; err_thr 0 .. 2^32; cols / rows as numpy fancy indices (repeats count as listed) or None for all.  Returns
    (score, ninfo) int32 [n_grp, n_cols, n_cols]: score[g][a][b] = rows of g where b's code is the class of sample a,
    ninfo[g][a][b] = rows of g where sample a has a call and b's code is not missing."""
    v = _selected(snps, cols, rows)
    grp_off = np.asarray(grp_off, dtype=np.int64)
    assert grp_off[0] == 0 and grp_off[-1] == len(v) and (np.diff(grp_off) >= 0).all()
    cls = sample_classes(v, err_thr, seed)
    nc = v.shape[1]
    score = np.zeros((len(grp_off) - 1, nc, nc), dtype=np.int32)
    ninfo = np.zeros_like(score)
    for g in range(len(grp_off) - 1):
        vg, cg = v[grp_off[g]:grp_off[g + 1]], cls[grp_off[g]:grp_off[g + 1]]
        if not len(vg):
            continue
        s = sum((cg == c).astype(np.float64).T @ (vg == c).astype(np.float64) for c in (0, 1, 2))
        n = (cg != NO_CALL).astype(np.float64).T @ (vg >= 0).astype(np.float64)
        score[g], ninfo[g] = np.rint(s).astype(np.int32), np.rint(n).astype(np.int32)
    return score, ninfo


def _scalar_hash(seed, a, k):
    """the hash once more with Python integers (the brute force's own statement of it)"""
    m = (1 << 64) - 1

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        return z ^ (z >> 31)
    return mix(mix((seed + 0x9E3779B97F4A7C15 * (a + 1)) & m) ^ k)


def sim_counts_direct(snps, grp_off, err_thr, seed, cols=None, rows=None):
    """the same counts row by row and pair by pair, straight from the rules (small inputs)"""
    v = _selected(snps, cols, rows).astype(np.int64)
    n, nc = v.shape
    score = np.zeros((len(grp_off) - 1, nc, nc), dtype=np.int32)
    ninfo = np.zeros_like(score)
    for g in range(len(grp_off) - 1):
        for k in range(int(grp_off[g]), int(grp_off[g + 1])):
            for a in range(nc):
                c = int(v[k, a])
                if c < 0 or c > 2:
                    continue
                h = _scalar_hash(int(seed), a, k)
                if (h >> 32) < err_thr:
                    c = ((h & 0xFFFFFFFF) * 3) >> 32
                for b in range(nc):
                    ninfo[g, a, b] += v[k, b] >= 0
                    score[g, a, b] += v[k, b] == c
    return score, ninfo


# ------------------------------------------------------------------------------------------------ the planted case
PLANTED_TWINS = (4, 9)
PLANTED_LEVELS = (40, 3000)
PLANTED_ERR = 0.005


def planted_case():
    """A DB of 12 accessions x 3000 rows in which accessions 4 and 9 differ at 30 rows only, all of them outside the 40 rows of the
    first level of the ladder that ``power.draw_ladder`` draws under seed 7: at the first level neither can be told from the other
    (both score 38 of 38 against either), at the last level (every row) each is unique even with calls redrawn at a rate of 0.005
    (under hash seed 7 the samples of 4 / 9 keep 2881 / 2883 of their 2889 calls; the likelihood ratio of the other twin is 5.39 /
    6.96, above 3.841).  Returns a dict: snps, names, positions, chrs, chr_regions, seed, levels."""
    from snpmatch_amd.core import power
    rng = np.random.default_rng(2214)
    n, na = 3000, 12
    a, b = PLANTED_TWINS
    db = rng.choice(np.array([0, 1], dtype=np.int8), size=(n, na))
    db[rng.random((n, na)) < 0.03] = -1
    db[:, b] = db[:, a]
    rows, _ = power.draw_ladder(n, PLANTED_LEVELS, np.random.default_rng(7))
    later = rows[PLANTED_LEVELS[0]:]
    both = later[(db[later, a] >= 0)][:30]
    db[both, b] = 1 - db[both, a]
    positions = np.arange(100, 100 + 50 * n, 50).astype(np.int64)
    return dict(snps=db, names=np.array(["acc%02d" % i for i in range(na)]), positions=positions, chrs=np.array(["Chr1"]),
                chr_regions=np.array([[0, n]], dtype=np.int64), seed=7, levels=PLANTED_LEVELS)
