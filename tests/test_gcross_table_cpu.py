"""the decision rule of genotype_cross over its whole argument space, without a GPU: every count tuple of windows of 1..40 rows
(tests/gcross_table.py) against the 50-digit decisions of tests/golden/gcross_table.npz -- the numpy twin, the package's scalar
port, the table generator's closed-form counts, and the condition that lets every cell be compared: no tuple on a threshold.
The top ``tot`` is 40 (the fixture is under half a MiB; it was not lowered)."""
import functools

import numpy as np
import pytest

import gcross_table
import gcross_twin
from snpmatch_amd.core import genotype_cross

PAIRS = gcross_table.PARENT_PAIRS
pair_ids = ["%dx%d" % p for p in PAIRS]


@functools.lru_cache(maxsize=2)
def _table(parents, bar):
    return gcross_table.build(parents, bar)


def _tuples_of(parents):
    """(counts [k, 3], tot [k]) of every cell a table of these parents holds, each tuple once per window size"""
    cnt = [gcross_table.true_counts(gcross_table.triples(tot), parents) for tot in range(1, gcross_table.TOP_TOT + 1)]
    tot = np.repeat(np.arange(1, gcross_table.TOP_TOT + 1), [len(c) for c in cnt])
    return np.concatenate(cnt), tot


def test_fixture_holds_every_tuple_once():
    fix = gcross_table.fixture()
    key = fix["key"].astype(np.int64)
    assert len(np.unique(key, axis=0)) == len(key) and key[:, 0].min() == 1 and key[:, 0].max() == gcross_table.TOP_TOT
    assert np.all(key[:, 1:].max(axis=1) <= key[:, 0])
    assert tuple(fix["thresholds"]) == gcross_table.THRESHOLDS and int(fix["n_marker_thres"]) == gcross_table.N_MARKER_THRES
    assert len(gcross_table.triples(40)) == 12341 and gcross_table.triples(2).tolist()[:4] == [[0, 0, 0], [0, 0, 1], [0, 0, 2], [0, 1, 0]]
    plain, tot = _tuples_of((0, 1))
    assert len(plain) == 135750 and len(np.unique(gcross_table.lookup(plain, tot))) == 135750
    for parents in PAIRS:
        cnt, tot = _tuples_of(parents)
        gcross_table.lookup(cnt, tot)                         # (asserts that every tuple is there)
    # three tuples by name: a window too small for lr_thres 1.5 to matter, a lone full count (``lr_thres`` stands in for the
    # ratio, so ``>=`` decides) and an exact tie m1 == m2 that only the tie rule turns into 1
    named = np.array([[3, 0, 0], [9, 0, 0], [4, 1, 4]])
    at = gcross_table.lookup(named, np.array([4, 9, 9]))
    assert fix["call"][at].tolist() == [[-1, -1, -1], [0, 0, 0], [1, 1, 1]]
    assert fix["tie"][at].tolist() == [False, False, True] and fix["high"][at].tolist() == [0, 0, 0]
    assert np.isnan(fix["ratio"][at[1]]) and not np.isnan(fix["ratio"][at[2]])
    # the recorded calls are the rule applied to the recorded parts
    at = np.arange(len(key))
    for j, thres in enumerate(gcross_table.THRESHOLDS):
        assert np.array_equal(gcross_table.stored_decide(at, key[:, 0], thres), fix["call"][:, j])


def test_twin_against_fixture():
    fix = gcross_table.fixture()
    key = fix["key"].astype(np.int64)
    for j, thres in enumerate(gcross_table.THRESHOLDS):
        geno, lr_next = gcross_twin.decide(key[:, None, 1:], key[:, 0], thres)
        assert np.array_equal(geno[:, 0], fix["call"][:, j]), thres
        # what the twin reports as consulted is the fixture's runner-up ratio, to rounding
        seen = ~np.isnan(lr_next[:, 0])
        assert np.all(~np.isnan(fix["ratio"][seen]))
        assert np.max(np.abs(lr_next[seen, 0] - fix["ratio"][seen]) / fix["ratio"][seen]) <= gcross_twin.KNIFE_EDGE_WIDTH / 4
    # with every window allowed (n_marker_thres 1) the twin follows the stored parts too
    geno, _ = gcross_twin.decide(key[:, None, 1:], key[:, 0], 1.5, n_marker_thres=1)
    assert np.array_equal(geno[:, 0], gcross_table.stored_decide(np.arange(len(key)), key[:, 0], 1.5, n_marker_thres=1))


def test_no_tuple_lies_on_a_threshold():
    """the condition under which NO cell is left out of any comparison: zero tuples within the knife-edge width of a threshold"""
    fix = gcross_table.fixture()
    key = fix["key"].astype(np.int64)
    width = gcross_twin.KNIFE_EDGE_WIDTH
    assert int(fix["consulted"]) == np.count_nonzero(~np.isnan(fix["ratio"]) & ~fix["tie"] & (fix["high"] != 1)) > 80000
    for j, thres in enumerate(gcross_table.THRESHOLDS):
        with np.errstate(invalid="ignore"):
            near = np.abs(fix["ratio"] - thres) <= width * thres              # every stored ratio, consulted or not
        assert np.count_nonzero(near) == 0, (thres, key[near])
        assert fix["min_distance"][j] > width
        _, lr_next = gcross_twin.decide(key[:, None, 1:], key[:, 0], thres, n_marker_thres=1)
        assert gcross_twin.knife_edge_cells(lr_next, thres) == 0
    positive = fix["lik"][~np.isnan(fix["lik"])]
    assert len(positive) == 40 * 39 // 2 and positive.min() > 1.0         # no likelihood <= 0: get_fraction never gives NaN here


def test_numpy_likelihood_against_50_digits():
    lik = gcross_table.fixture()["lik"]
    m, tot = np.nonzero(~np.isnan(lik))
    e_np = np.max(np.abs(gcross_twin.likeli(tot, m) - lik[m, tot]) / lik[m, tot])
    print("e_np = %.3e over %d (m, tot)" % (e_np, len(m)))
    assert 4 * e_np <= gcross_twin.KNIFE_EDGE_WIDTH


@pytest.mark.parametrize("bar", [0, 1])
@pytest.mark.parametrize("parents", PAIRS, ids=pair_ids)
def test_scan_against_closed_form(parents, bar):
    t = _table(parents, bar)
    assert t.codes.shape == (820, 12341) and np.array_equal(np.diff(t.win_off), np.arange(1, 41))
    assert np.all((t.codes >> 3) == bar) and np.all((t.codes & 7) <= 3)
    assert np.all(t.p1 == parents[0]) and np.all(t.p2 == parents[1])
    assert np.array_equal(gcross_twin.counts(t.codes, t.p1, t.p2, t.win_off), t.counts)
    for tot in (1, 7, 40):
        k = len(gcross_table.triples(tot))
        assert np.array_equal(t.triple[tot - 1], gcross_table.triples(tot)[np.arange(12341) % k])
    if 2 not in parents:
        assert np.array_equal(t.counts, t.triple)
    elif parents[0] == 2:
        assert np.all(t.counts[:, :, 0] == t.counts[:, :, 1])
    else:
        assert np.all(t.counts[:, :, 2] == t.counts[:, :, 1])
    # the rows of a sample are permuted on their own: in the longest window the four waves' shares of a count differ
    last = (t.codes[t.win_off[-2]:] & 7) == parents[0]
    shares = np.stack([last[w::4].sum(axis=0) for w in range(4)])
    assert np.count_nonzero(shares.max(axis=0) - shares.min(axis=0) > 1) > 1000


@pytest.mark.parametrize("parents", PAIRS, ids=pair_ids)
def test_scalar_port_against_fixture(parents):
    t = _table(parents, 0)
    rng = np.random.default_rng(7 + 10 * parents[0] + parents[1])
    text = np.array(["0/0", "1/1", "0/1", "./."])
    win = rng.integers(0, len(t.tots), size=500)
    smp = np.array([rng.integers(0, len(gcross_table.triples(int(t.tots[w])))) for w in win])
    for thres in gcross_table.THRESHOLDS:
        want = gcross_table.golden_calls(t.counts[win, smp], t.tots[win], thres)
        for w, s, expected in zip(win.tolist(), smp.tolist(), want.tolist()):
            rows = slice(int(t.win_off[w]), int(t.win_off[w + 1]))
            call = genotype_cross.GenotypeCross.get_window_genotype_gts(text[t.codes[rows, s] & 7], t.p1[rows], t.p2[rows], thres)[0]
            assert (-1 if call == 'NA' else call) == expected, (parents, t.counts[w, s], t.tots[w], thres)


@pytest.mark.parametrize("parents", PAIRS, ids=pair_ids)
def test_every_outcome_and_both_special_rules_occur(parents):
    """NA, 0, 1 and 2 all occur for every threshold -- except the call of a parent that is itself heterozygous: its count IS the
    heterozygous count (m1 == mh or m2 == mh in every cell), so whenever it is the most likely class two ratios equal 1 and the tie
    rule gives 1.  For those pairs the test asserts that this call never occurs, and that the other three do."""
    cnt, tot = _tuples_of(parents)
    never = [k for k in (0, 2) if parents[k // 2] == 2]
    big = tot >= gcross_table.N_MARKER_THRES
    tied = big & (cnt[:, 0] == cnt[:, 2]) & (cnt[:, 0] > 0)
    full = big & (cnt.max(axis=1) == tot)
    assert np.count_nonzero(tied) > 0 and np.count_nonzero(full) > 0
    # ``tied`` also holds the cells where heterozygous simply wins: the tie rule itself ("more than one ratio equal to 1") is hit
    # where the 50-digit rule recorded it, and there it is what decides (``high`` is not 1 in some of them)
    by_tie = np.zeros(len(cnt), dtype=bool)
    by_tie[big] = gcross_table.fixture()["tie"][gcross_table.lookup(cnt[big], tot[big])]
    assert np.count_nonzero(by_tie) > 0 and np.count_nonzero(by_tie & tied) > 0
    assert np.count_nonzero(by_tie & (gcross_table.fixture()["high"][gcross_table.lookup(cnt, tot)] != 1)) > 0
    for thres in gcross_table.THRESHOLDS:
        call = gcross_table.golden_calls(cnt, tot, thres)
        assert sorted(np.unique(call).tolist()) == [c for c in (-1, 0, 1, 2) if c not in never], (parents, thres)
        assert np.all(call[tied] == 1) and np.all(call[by_tie] == 1)   # m1 == m2 > 0: a tie, or heterozygous the most likely
        assert np.all(call[full] >= 0)                           # a count equal to tot: likelihood 1, always decided
        only = full & (np.count_nonzero(cnt, axis=1) == 1)       # ... and alone: that class, lr_thres standing in for the ratio
        assert np.count_nonzero(only) > 0 and np.array_equal(call[only], np.argmax(cnt[only], axis=1))
        assert np.all(call[~big] == -1) and np.all(call[cnt.max(axis=1) == 0] == -1)
