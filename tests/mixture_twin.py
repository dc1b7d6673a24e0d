"""numpy twin of ``snpm_panel_mix_counts`` / ``k_mix_count`` (test infrastructure): the read-count-weighted 2 x 2 table of every
ordered pair of accession columns against one sample's alt / ref read counts, the scalar form of the host fit, and the planted
panel of the ``mixture`` tests."""
import math

import numpy as np


def _select(snps, cols, rows):
    v = np.asarray(snps)
    if rows is not None:
        v = v[rows, :]
    if cols is not None:
        v = v[:, np.asarray(cols, dtype=np.int64)]
    return v


def mix_counts(snps, alt, ref, cols=None, rows=None):
    """snps int8 [n_snp, n_acc] (0 / 1 homozygous calls; anything else -- missing, het, other -- drops the row for a pair); alt,
    ref: one read count per selected row; cols / rows as numpy fancy indices (repeats count as listed), a slice for rows, or None
    for all.  Returns int32 [2, 2, 2, n_cols, n_cols]: ``T[w, ca, cb, a, b]`` = the sum over rows where column a has call ca and
    column b has call cb of the alt (w = 0) or ref (w = 1) reads.  The contraction runs in int64."""
    v = _select(snps, cols, rows)
    weights = np.stack([np.asarray(alt).reshape(-1), np.asarray(ref).reshape(-1)]).astype(np.int64)
    assert weights.shape[1] == len(v), "one alt and one ref count per selected row"
    ind = np.stack([v == 0, v == 1]).astype(np.int64)                 # [call, row, column]
    table = np.einsum("wr,cra,drb->wcdab", weights, ind, ind, optimize=True)
    assert table.max(initial=0) < 2 ** 31
    return table.astype(np.int32)


def mix_counts_direct(snps, alt, ref):
    """the same table by three nested loops, straight from the definition (small inputs)"""
    v = np.asarray(snps)
    n, k = v.shape
    table = np.zeros((2, 2, 2, k, k), dtype=np.int32)
    for a in range(k):
        for b in range(k):
            for r in range(n):
                ca, cb = int(v[r, a]), int(v[r, b])
                if ca in (0, 1) and cb in (0, 1):
                    table[0, ca, cb, a, b] += int(alt[r])
                    table[1, ca, cb, a, b] += int(ref[r])
    return table


def fit_scalar(cell, err, grid):
    """one ordered pair in plain Python: ``cell`` [2][2][2] (weight, call of a, call of b) -> (alpha_hat, LL(alpha_hat), LL(0),
    every LL); the first of equal maxima wins"""
    lls = []
    for alpha in grid:
        ll = 0.0
        for ca in (0, 1):
            for cb in (0, 1):
                f = (1.0 - alpha) * ca + alpha * cb
                fe = f * (1.0 - 2.0 * err) + err
                ll += int(cell[0][ca][cb]) * math.log(fe) + int(cell[1][ca][cb]) * math.log(1.0 - fe)
        lls.append(ll)
    best = max(range(len(lls)), key=lambda k: (lls[k], -k))
    return float(grid[best]), lls[best], lls[0], lls


# ------------------------------------------------------------------------------------------------ the planted case
PLANTED_MAJOR, PLANTED_MINOR = 7, 23


def planted_case(alpha, seed=2026, n=6000, na=40, err=0.01, depth=3.0):
    """A DB of 40 accessions x 6000 rows on two chromosomes (calls 0 / 1, 4 % missing) and the reads of a pool of accession 7 with a
    fraction ``alpha`` of accession 23: depth Poisson(3) per row, every read alt with probability f (1 - 2e) + e, f = (1 - alpha)
    c7 + alpha c23; rows where either is missing draw f from another column.  Returns a dict: snps, names, positions, chrs,
    chr_regions (the DB) and chrom, pos, alt, ref (the sample, every DB row plus 40 positions the DB does not have)."""
    rng = np.random.default_rng(seed)
    db = rng.choice(np.array([0, 1], dtype=np.int8), size=(n, na))
    db[rng.random((n, na)) < 0.04] = -1
    ca, cb = db[:, PLANTED_MAJOR].astype(np.float64), db[:, PLANTED_MINOR].astype(np.float64)
    other = np.abs(db[:, 0]).astype(np.float64)
    ca = np.where(ca < 0, other, ca)
    cb = np.where(cb < 0, ca, cb)
    f = (1.0 - alpha) * ca + alpha * cb
    dp = rng.poisson(depth, size=n)
    alt = rng.binomial(dp, f * (1.0 - 2.0 * err) + err)
    ref = dp - alt
    half = n // 2
    positions = np.concatenate([np.arange(10, 10 + 10 * half, 10), np.arange(7, 7 + 10 * (n - half), 10)]).astype(np.int64)
    regions = np.array([[0, half], [half, n]], dtype=np.int64)
    chrom = np.where(np.arange(n) < half, 1, 2)
    extra_chr = np.repeat([1, 2], 20)
    extra_pos = np.concatenate([np.arange(15, 15 + 700 * 20, 700) + 1, np.arange(12, 12 + 500 * 20, 500) + 1]).astype(np.int64)
    s_chr, s_pos = np.concatenate([chrom, extra_chr]), np.concatenate([positions, extra_pos])
    s_alt, s_ref = np.concatenate([alt, np.full(40, 2)]), np.concatenate([ref, np.full(40, 1)])
    order = np.lexsort((s_pos, s_chr))
    return dict(snps=db, names=np.array(["acc%02d" % i for i in range(na)]), positions=positions, chrs=np.array(["Chr1", "Chr2"]),
                chr_regions=regions, chrom=np.array(["Chr%d" % c for c in s_chr[order]]), pos=s_pos[order], alt=s_alt[order],
                ref=s_ref[order])


def write_planted(case, directory):
    """the DB of ``planted_case`` as an .npz and the sample as a one-sample VCF with GT:AD:DP (GT left uncalled: the reader does
    not look at it); returns (db path, vcf path)"""
    import os
    db = os.path.join(str(directory), "db.npz")
    np.savez(db, snps=case["snps"], accessions=case["names"], positions=case["positions"], chrs=case["chrs"], chr_regions=case["chr_regions"])
    vcf = os.path.join(str(directory), "sample.vcf")
    with open(vcf, "w") as fh:
        fh.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tpool\n")
        for c, p, a, r in zip(case["chrom"], case["pos"], case["alt"], case["ref"]):
            fh.write("%s\t%d\t.\tA\tT\t50\tPASS\tDP=%d\tGT:AD:DP\t./.:%d,%d:%d\n" % (c, p, a + r, r, a, a + r))
    return db, vcf


def install_twin(monkeypatch):
    """``engine.mix_counts`` answered by the twin on the DB the next ``Genotype`` is loaded from, and no panel made; returns the list
    that records (cols, rows, largest count) of every call"""
    from snpmatch_amd import engine
    from snpmatch_amd.core import snp_genotype
    calls, loaded = [], {}
    stub = engine.Panel.__new__(engine.Panel)
    stub.h = None
    real_init = snp_genotype.Genotype.__init__

    def init(self, *a, **k):
        real_init(self, *a, **k)
        loaded["snps"] = np.asarray(self.g.snps)

    def twin(panel, alt, ref, cols=None, rows=None):
        calls.append((cols, rows, int(max(np.max(alt, initial=0), np.max(ref, initial=0)))))
        rows = np.arange(rows.start, rows.stop) if isinstance(rows, range) else rows
        return mix_counts(loaded["snps"], alt, ref, cols, rows)
    monkeypatch.setattr(snp_genotype.Genotype, "__init__", init)
    monkeypatch.setattr(snp_genotype.Genotype, "panel", lambda self, ctx=None, packed=None: stub)
    monkeypatch.setattr(engine, "mix_counts", twin)
    return calls
