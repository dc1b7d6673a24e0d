"""numpy twin of ``snpm_panel_mosaic`` (include/snpmatch_hip.h): the copying-model Viterbi with a uniform switch cost and integer
costs over the listed accession columns, vectorised over the columns, one Python step per row -- and ``brute``, the full
ncols x ncols transition DP, for the costs only.  Both work on canonical calls: -1 missing, 0 / 1 / 2, 3 an int8 panel's "other"."""
import numpy as np

NO_CLASS = 0xFF


def canon(snps, packed=False):
    """calls of a panel as the device sees them: negative -> -1; a packed panel has no code 3 (it stores 3 for missing)"""
    s = np.asarray(snps).astype(np.int64)
    s = np.where(s < 0, -1, s)
    if packed:
        s = np.where(s > 2, -1, s)
    return s


def emissions(sel, cls, cost):
    """e [n_rows, ncols] int64 of one sample: sel [n_rows, ncols] canonical calls of the selected rows and listed columns"""
    cost = np.asarray(cost, dtype=np.int64).reshape(3, 4)
    cls = np.asarray(cls).astype(np.int64)
    e = np.zeros(sel.shape, dtype=np.int64)
    have = (cls <= 2)[:, None] & (sel >= 0)
    ci = np.where(cls <= 2, cls, 0)[:, None]
    e[have] = cost[np.broadcast_to(ci, sel.shape)[have], np.clip(sel, 0, 3)[have]]
    return e


def select(snps, cols=None, rows=None, packed=False):
    s = canon(snps, packed)
    if rows is not None:
        s = s[np.asarray(rows, dtype=np.int64)]
    if cols is not None:
        s = s[:, np.asarray(cols, dtype=np.int64)]
    return s


def mosaic_e(e, chain_off, S):
    """the model on the emissions of one sample: (state [n_rows] int32, chain_cost [n_chain] int32, col_cost [n_chain, ncols] int32)"""
    n_rows, ncols = e.shape
    chain_off = np.asarray(chain_off, dtype=np.int64)
    n_chain = len(chain_off) - 1
    state = np.zeros(n_rows, dtype=np.int32)
    chain_cost = np.zeros(n_chain, dtype=np.int32)
    col_cost = np.zeros((n_chain, ncols), dtype=np.int32)
    S = int(S)
    for c in range(n_chain):
        c0, c1 = int(chain_off[c]), int(chain_off[c + 1])
        if c1 <= c0:
            continue
        col_cost[c] = e[c0:c1].sum(axis=0)
        sw = np.zeros((c1 - c0, ncols), dtype=bool)
        j = np.zeros(c1 - c0, dtype=np.int64)
        V = e[c0].copy()
        for k in range(c0 + 1, c1):
            jj = int(np.argmin(V))              # the first minimum: the lowest a
            B = V[jj]
            j[k - 1 - c0] = jj
            sw[k - c0] = V > B + S
            V = np.minimum(V, B + S) + e[k]
        st = int(np.argmin(V))
        chain_cost[c] = V[st]
        state[c1 - 1] = st
        for k in range(c1 - 1, c0, -1):
            if sw[k - c0, st]:
                st = int(j[k - 1 - c0])
            state[k - 1] = st
    return state, chain_cost, col_cost


def mosaic(snps, classes, chain_off, cost, S, cols=None, rows=None, packed=False):
    """the twin of ``engine.mosaic``: classes [n_samples, n_rows] -> (state [n_samples, n_rows], chain_cost [n_samples, n_chain],
    col_cost [n_samples, n_chain, ncols])"""
    sel = select(snps, cols, rows, packed)
    classes = np.asarray(classes, dtype=np.uint8).reshape(-1, sel.shape[0])
    out = [mosaic_e(emissions(sel, cls, cost), chain_off, S) for cls in classes]
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


def path_cost(e, chain_off, S, state):
    """the cost of a path under the model: its emissions plus S per change of state inside a chain, per chain"""
    chain_off = np.asarray(chain_off, dtype=np.int64)
    out = np.zeros(len(chain_off) - 1, dtype=np.int64)
    for c in range(len(out)):
        c0, c1 = int(chain_off[c]), int(chain_off[c + 1])
        if c1 <= c0:
            continue
        st = np.asarray(state[c0:c1], dtype=np.int64)
        out[c] = e[np.arange(c0, c1), st].sum() + S * int(np.count_nonzero(st[1:] != st[:-1]))
    return out


def brute(e, chain_off, S):
    """the full-transition DP (cost 0 to stay, S to move to any other column), for the chain costs only"""
    chain_off = np.asarray(chain_off, dtype=np.int64)
    ncols = e.shape[1]
    trans = np.full((ncols, ncols), int(S), dtype=np.int64)
    np.fill_diagonal(trans, 0)
    out = np.zeros(len(chain_off) - 1, dtype=np.int64)
    for c in range(len(out)):
        c0, c1 = int(chain_off[c]), int(chain_off[c + 1])
        if c1 <= c0:
            continue
        V = e[c0].copy()
        for k in range(c0 + 1, c1):
            V = (V[:, None] + trans).min(axis=0) + e[k]
        out[c] = V.min()
    return out


# ------------------------------------------------------------------------------------------------ the planted case
PLANTED_SOURCES = (5, 17, 23, 31)       # the accessions the sample copies
PLANTED_NEAR = 38                       # a near-duplicate of accession 17: 5 % of its calls differ
PLANTED_TOL = 10                        # sites: every planted breakpoint has a segment boundary this close, and no segment is extra
PLANTED_S, PLANTED_MISMATCH, PLANTED_HET = 40, 2, 1
# (chain, first matched row, one past the last, accession) -- stretches of the MATCHED rows, chain by chain
PLANTED_PLAN = ((0, 0, 420, 5), (0, 420, 900, 17), (0, 900, 1350, 31), (1, 1350, 1800, 23), (1, 1800, 2300, 17), (1, 2300, 2700, 5))


def planted(seed=11):
    """A 40-accession panel of 3000 rows on two chromosomes (homozygous calls, 3 % missing, 1 % het), accession 38 a near-duplicate
    of 17, and a sample that has calls at 2700 of the rows (every tenth row dropped) copied from four accessions in the stretches
    of PLANTED_PLAN with 1 % of its calls flipped.  dict: snps, accessions, positions, chrs, chr_regions; s_chr, s_pos, s_gt (the
    sample's records as text); rows (the matched DB rows), classes, chain_off."""
    rng = np.random.default_rng(seed)
    n, n_acc = 3000, 40
    snps = rng.choice(np.array([0, 1], dtype=np.int8), size=(n, n_acc))
    near = snps[:, 17].copy()
    flip = rng.random(n) < 0.05
    near[flip] = 1 - near[flip]
    snps[:, PLANTED_NEAR] = near
    snps[rng.random((n, n_acc)) < 0.03] = -1
    snps[rng.random((n, n_acc)) < 0.01] = 2
    positions = np.concatenate([np.arange(1, 1501) * 100, np.arange(1, 1501) * 100]).astype(np.int32)
    regions = np.array([[0, 1500], [1500, 3000]])
    rows = np.flatnonzero(np.arange(n) % 10 != 9)
    assert len(rows) == 2700
    chain_off = np.array([0, 1350, 2700])
    true = np.zeros(len(rows), dtype=np.int64)
    for _, k0, k1, a in PLANTED_PLAN:
        true[k0:k1] = a
    calls = snps[rows, true].astype(np.int64)
    calls[calls < 0] = rng.integers(0, 2, size=int((calls < 0).sum()))          # the sample has a call where its source has none
    flipped = rng.random(len(rows)) < 0.01
    calls[flipped] = (calls[flipped] + 1 + rng.integers(0, 2, size=int(flipped.sum()))) % 3
    classes = calls.astype(np.uint8)
    text = np.array(["0/0", "1/1", "0/1"])[classes]
    chrs = np.array(["1", "2"])
    return {"snps": snps, "accessions": np.array(["acc%02d" % a for a in range(n_acc)]), "positions": positions, "chrs": chrs, "chr_regions": regions,
            "s_chr": np.repeat(chrs, 1500)[rows], "s_pos": positions[rows], "s_gt": text, "rows": rows, "classes": classes, "chain_off": chain_off}


def plan_recovered(segs, tol=PLANTED_TOL):
    """segs: rows of (chain, first, last, accession index).  The planted plan is recovered when the segments are the plan's, in
    order, with the plan's accessions, and every boundary lies within ``tol`` sites of the planted one"""
    segs = [tuple(int(v) for v in s) for s in segs]
    if len(segs) != len(PLANTED_PLAN):
        return False
    for (c, k0, k1, a), (pc, p0, p1, pa) in zip(segs, PLANTED_PLAN):
        if (c, a) != (pc, pa) or abs(k0 - p0) > tol or abs(k1 + 1 - p1) > tol:
            return False
    return True
