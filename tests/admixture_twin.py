"""numpy twin of ``snpm_panel_admix`` / ``engine.admix`` (test infrastructure): one joint EM iteration of the admixture model as array
operations in any floating-point type -- fp64 stands in for the device in the CPU tests, ``numpy.longdouble`` (64-bit mantissa on
x86) is the reference of the tolerance tests -- the same iteration as plain Python loops, the bounds of the issue, and the planted
panel of the command tests (three Balding-Nichols populations, pure and two-way admixed accessions)."""
import math

import numpy as np

EPS = 1e-6
ONE_MINUS_EPS = 1.0 - 1e-6          # (the fp64 value the device clamps at)
U52 = 2.0 ** -52


def dosage(snps, cols=None, rows=None):
    """(g int64 [n_rows, n_cols], called bool): dosage 0 / 2 / 1 of the codes 0 / 1 / 2 of the selected rows and columns of snps int8
    [n_snp, n_acc]; a negative code and anything above 2 is no call.  cols / rows: fancy indices (repeats count as listed), a range,
    or None"""
    v = np.asarray(snps)
    if rows is not None:
        v = v[np.arange(rows.start, rows.stop) if isinstance(rows, range) else np.asarray(rows, dtype=np.int64), :]
    if cols is not None:
        v = v[:, np.asarray(cols, dtype=np.int64).reshape(-1)]
    called = (v >= 0) & (v <= 2)
    return np.where(v == 1, 2, np.where(v == 2, 1, 0)).astype(np.int64), called


def step(snps, Q, F, cols=None, rows=None, update_q=True, update_f=True, dtype=np.float64):
    """one iteration: (Q', F', ll of the OLD pair) in ``dtype``; a component that is not updated is returned as it came"""
    g, called = dosage(snps, cols, rows)
    Q, F = np.asarray(Q, dtype=dtype), np.asarray(F, dtype=dtype)
    one, two = dtype(1.0), dtype(2.0)
    g = g.astype(dtype)
    Fb = one - F
    p, pbar = F @ Q.T, Fb @ Q.T                                      # [rows, cols]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(called, g / p, dtype(0.0))
        v = np.where(called, (two - g) / pbar, dtype(0.0))
        ll = np.where(called & (g > 0), g * np.log(p), dtype(0.0)).sum(dtype=dtype) + np.where(called & (g < 2), (two - g) * np.log(pbar), dtype(0.0)).sum(dtype=dtype)
    Qn, Fn = Q, F
    if update_f:
        a, b = u @ Q, v @ Q
        x, den = F * a, F * a + Fb * b
        with np.errstate(divide="ignore", invalid="ignore"):
            Fn = np.where(den != 0, np.clip(x / den, dtype(EPS), dtype(ONE_MINUS_EPS)), F)
    if update_q:
        w = Q * (u.T @ F + v.T @ Fb)
        sw = w.sum(axis=1, dtype=dtype)[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            Qn = np.where(sw != 0, w / sw, Q)
    return Qn, Fn, ll


def admix(snps, Q, F, n_iter=1, cols=None, rows=None, update_q=True, update_f=True, dtype=np.float64):
    """the signature of ``engine.admix`` on a matrix in memory: (Q, F, loglik [n_iter])"""
    Q, F = np.array(Q, dtype=dtype), np.array(F, dtype=dtype)
    trace = np.zeros(n_iter, dtype=dtype)
    for t in range(n_iter):
        Q, F, trace[t] = step(snps, Q, F, cols, rows, update_q, update_f, dtype)
    return Q, F, trace


def step_loops(snps, Q, F):
    """the same iteration (all rows, all columns, both updates) as plain Python loops over lists of floats"""
    snps, Q, F = np.asarray(snps).tolist(), np.asarray(Q, dtype=np.float64).tolist(), np.asarray(F, dtype=np.float64).tolist()
    R, n, K = len(F), len(Q), len(Q[0])
    a = [[0.0] * K for _ in range(R)]
    b = [[0.0] * K for _ in range(R)]
    c = [[0.0] * K for _ in range(n)]
    ll = 0.0
    for s in range(R):
        for i in range(n):
            code = snps[s][i]
            if code < 0 or code > 2:
                continue
            g = (0.0, 2.0, 1.0)[code]
            p = math.fsum(Q[i][k] * F[s][k] for k in range(K))
            pbar = math.fsum(Q[i][k] * (1.0 - F[s][k]) for k in range(K))
            u, v = g / p, (2.0 - g) / pbar
            if g > 0:
                ll += g * math.log(p)
            if g < 2:
                ll += (2.0 - g) * math.log(pbar)
            for k in range(K):
                a[s][k] += u * Q[i][k]
                b[s][k] += v * Q[i][k]
                c[i][k] += u * F[s][k] + v * (1.0 - F[s][k])
    Fn = [row[:] for row in F]
    for s in range(R):
        for k in range(K):
            x, y = F[s][k] * a[s][k], (1.0 - F[s][k]) * b[s][k]
            if x + y != 0:
                Fn[s][k] = min(max(x / (x + y), EPS), ONE_MINUS_EPS)
    Qn = [row[:] for row in Q]
    for i in range(n):
        w = [Q[i][k] * c[i][k] for k in range(K)]
        if sum(w) != 0:
            Qn[i] = [wk / sum(w) for wk in w]
    return np.array(Qn), np.array(Fn), ll


def random_start(rng, n, R, K):
    """a valid pair: Dirichlet(1) rows of Q, F uniform in 0.1 .. 0.9"""
    return rng.dirichlet(np.ones(K), size=n), rng.uniform(0.1, 0.9, size=(R, K))


def ll_bound(ll_ref, cells, ncols, K):
    """the issue's bound of |ll - ll_ref|: 2^-52 ((K + 2) cells + (ceil(ncols / 64) + 64) |ll_ref|)"""
    return U52 * ((K + 2) * cells + ((ncols + 63) // 64 + 64) * abs(float(ll_ref)))


def worst_ratios(got, ref, snps, cols=None, rows=None):
    """(F, Q, ll): the largest error of ``got`` = (Q', F', ll) against the long-double ``ref`` as a fraction of its bound -- each
    entry of F' within (ncols + 64) 2^-52 relative, of Q' within (n_rows + 64) 2^-52 relative, ll within ``ll_bound``"""
    (Qg, Fg, llg), (Qr, Fr, llr) = got, ref
    n, K = Qr.shape
    R = Fr.shape[0]
    cells = int(dosage(snps, cols, rows)[1].sum())

    def rel(g, r):                          # (an entry whose reference is 0 must be 0)
        err = np.abs(np.asarray(g, dtype=np.longdouble) - r)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(r != 0, err / np.abs(r), np.where(err == 0, 0.0, np.inf)).max() if r.size else 0.0
    return (float(rel(Fg, Fr) / ((n + 64) * U52)), float(rel(Qg, Qr) / ((R + 64) * U52)),
            float(abs(np.longdouble(llg) - llr) / max(ll_bound(llr, cells, n, K), 1e-300)))


# ------------------------------------------------------------------------------------------------ the planted panel
PLANTED_POPS, PLANTED_PER_POP, PLANTED_ROWS, PLANTED_FST = 3, 13, 600, 0.15
PLANTED_MIX = ((0, 1, 0.3), (1, 2, 0.4), (2, 0, 0.5), (0, 1, 0.6), (1, 2, 0.7), (2, 0, 0.45))      # (source A, source B, fraction of A)


def planted_case(seed):
    """the recipe of pca_twin.planted_case -- 3 Balding-Nichols populations (Fst 0.15) x 13 inbred accessions x 600 rows on two
    chromosomes, the LAST accession of every population held out -- plus 6 inbred two-way admixed accessions (every row's allele drawn
    from source A with the fraction given, else from B); then 2 % of the calls het, then 3 % missing.  ``panel`` lists the 36 pure
    accessions, population by population, then the 6 admixed ones; ``truth`` [45, 3] is the planted ancestry."""
    rng = np.random.default_rng(2000 + seed)
    n_pure = PLANTED_POPS * PLANTED_PER_POP
    n_acc = n_pure + len(PLANTED_MIX)
    anc = rng.uniform(0.1, 0.9, size=PLANTED_ROWS)
    f = (1.0 - PLANTED_FST) / PLANTED_FST
    freq = np.stack([rng.beta(anc * f, (1.0 - anc) * f) for _ in range(PLANTED_POPS)], axis=1)
    snps = np.empty((PLANTED_ROWS, n_acc), dtype=np.int8)
    truth = np.zeros((n_acc, PLANTED_POPS))
    for q in range(PLANTED_POPS):
        snps[:, q * PLANTED_PER_POP:(q + 1) * PLANTED_PER_POP] = rng.random((PLANTED_ROWS, PLANTED_PER_POP)) < freq[:, [q]]
        truth[q * PLANTED_PER_POP:(q + 1) * PLANTED_PER_POP, q] = 1.0
    for m, (qa, qb, frac) in enumerate(PLANTED_MIX):
        src = np.where(rng.random(PLANTED_ROWS) < frac, qa, qb)
        snps[:, n_pure + m] = rng.random(PLANTED_ROWS) < freq[np.arange(PLANTED_ROWS), src]
        truth[n_pure + m, qa], truth[n_pure + m, qb] = frac, 1.0 - frac
    snps[rng.random(snps.shape) < 0.02] = 2
    snps[rng.random(snps.shape) < 0.03] = -1
    names = np.array(["p%da%02d" % (a // PLANTED_PER_POP, a % PLANTED_PER_POP) for a in range(n_pure)] + ["mix%d" % m for m in range(len(PLANTED_MIX))])
    pop = np.array(["pop%d" % (a // PLANTED_PER_POP) for a in range(n_pure)] + ["mixed"] * len(PLANTED_MIX))
    held = np.array([(q + 1) * PLANTED_PER_POP - 1 for q in range(PLANTED_POPS)])
    pure = np.array([a for a in range(n_pure) if a not in held.tolist()])
    panel = np.concatenate([pure, np.arange(n_pure, n_acc)])
    chrs = np.array(["Chr1", "Chr2"])
    chr_regions = np.array([[0, 350], [350, 600]])
    positions = np.concatenate([101 + 1000 * np.arange(350), 101 + 1000 * np.arange(250)]).astype(np.int64)
    return {"snps": snps, "names": names, "pop": pop, "held": held, "pure": pure, "panel": panel, "truth": truth, "positions": positions, "chrs": chrs,
            "chr_regions": chr_regions}
