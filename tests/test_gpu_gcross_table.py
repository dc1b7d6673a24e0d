"""the decision of ``k_gcross`` over its whole argument space on the device: every count triple of windows of 1..40 rows
(tests/gcross_table.py: 820 rows x 12 341 samples, 49 sample tiles, every split of a window over the four waves) for the six
ordered parent pairs, against the 50-digit decisions of tests/golden/gcross_table.npz and the numpy twin -- no cell is left out
(tests/test_gcross_table_cpu.py holds the condition for that: no tuple lies on a threshold).  Also both sides of
``n_marker_thres``, the other separator, and the measured distance of the device's and numpy's ``likeliTest`` from the true value,
which is what the knife-edge width of ``gcross_twin`` has to cover.  The top ``tot`` is 40: the fixture did not have to shrink.

What stays sampled (tests/test_gpu_gcross.py): separators mixed inside a window and windows longer than 40 rows."""
import functools

import numpy as np
import pytest

import gcross_table
import gcross_twin
from snpmatch_amd import engine

pytestmark = pytest.mark.gpu
PAIRS = gcross_table.PARENT_PAIRS
pair_ids = ["%dx%d" % p for p in PAIRS]
N_SAMPLES = 12341
TOTS = np.arange(1, gcross_table.TOP_TOT + 1)


@pytest.fixture(scope="module")
def ctx():
    return engine.default_context()


@functools.lru_cache(maxsize=2)
def _case(parents, bar=0):
    """(table, view): the view is row-strided, 0xEE in the seven columns behind every row"""
    t = gcross_table.build(parents, bar)
    padded = np.full((len(t.codes), N_SAMPLES + 7), 0xEE, dtype=np.uint8)
    padded[:, :N_SAMPLES] = t.codes
    padded.flags.writeable = False
    return t, padded[:, :N_SAMPLES]


def _differing(got, want, t):
    """the first cells that differ, as (tot, m1, mh, m2, got, want): what a failure should name"""
    w, s = np.nonzero(got != want)
    return [(int(t.tots[a]),) + tuple(t.counts[a, b].tolist()) + (int(got[a, b]), int(want[a, b])) for a, b in zip(w[:8], s[:8])]


@pytest.mark.parametrize("parents", PAIRS, ids=pair_ids)
def test_every_count_triple(parents, ctx):
    t, view = _case(parents)
    assert view.shape == (820, N_SAMPLES) and view.strides[0] == N_SAMPLES + 7 and -(-N_SAMPLES // 256) == 49
    geno, counts = engine.cross_calls(ctx, view, t.p1, t.p2, t.win_off, 1.5, return_counts=True)
    assert np.array_equal(counts, t.counts), "counts differ in %d cells" % np.count_nonzero((counts != t.counts).any(axis=2))
    twin_counts = gcross_twin.counts(t.codes, t.p1, t.p2, t.win_off)
    assert np.array_equal(twin_counts, t.counts)
    at = gcross_table.lookup(t.counts, TOTS[:, None])
    fix = gcross_table.fixture()
    for j, thres in enumerate(gcross_table.THRESHOLDS):
        want = fix["call"][at, j]
        twin, lr_next = gcross_twin.decide(twin_counts, TOTS, thres)
        assert gcross_twin.knife_edge_cells(lr_next, thres) == 0
        assert np.array_equal(twin, want), ("twin != fixture", thres, _differing(twin, want, t))
        got = engine.cross_calls(ctx, view, t.p1, t.p2, t.win_off, thres)               # counts == NULL
        assert np.array_equal(got, want), ("device != fixture", thres, _differing(got, want, t))
        assert np.array_equal(got, twin)
        if thres == 1.5:
            assert np.array_equal(geno, want), ("device (with counts) != fixture", _differing(geno, want, t))


@pytest.mark.parametrize("n_marker_thres", [1, 6, 41])
def test_both_sides_of_the_marker_threshold(n_marker_thres, ctx):
    t, view = _case((0, 1))
    at = gcross_table.lookup(t.counts, TOTS[:, None])
    want = gcross_table.stored_decide(at, TOTS[:, None], 1.5, n_marker_thres)          # the rule on the stored 50-digit parts
    small = TOTS < n_marker_thres
    recorded = gcross_table.fixture()["call"][at, 1]                                   # (n_marker_thres 5)
    assert np.all(want[small] == -1)
    if n_marker_thres >= gcross_table.N_MARKER_THRES:
        assert np.array_equal(want[~small], recorded[~small])
    else:
        assert np.array_equal(want[4:], recorded[4:]) and np.all(recorded[:4] == -1) and np.any(want[:4] >= 0)
    got = engine.cross_calls(ctx, view, t.p1, t.p2, t.win_off, 1.5, n_marker_thres=n_marker_thres)
    assert np.all(got[small] == -1)
    assert np.array_equal(got, want), _differing(got, want, t)
    twin, _ = gcross_twin.decide(t.counts, TOTS, 1.5, n_marker_thres)
    assert np.array_equal(got, twin)


def test_the_other_separator_changes_nothing(ctx):
    parents = (1, 2)
    t0, view0 = _case(parents)
    t1, view1 = _case(parents, 1)
    assert np.array_equal(t1.codes, t0.codes | 8) and np.array_equal(t1.counts, t0.counts)
    geno0, counts0 = engine.cross_calls(ctx, view0, t0.p1, t0.p2, t0.win_off, 1.5, return_counts=True)
    geno1, counts1 = engine.cross_calls(ctx, view1, t1.p1, t1.p2, t1.win_off, 1.5, return_counts=True)
    assert np.array_equal(counts1, counts0) and np.array_equal(counts1, t1.counts)
    assert np.array_equal(geno1, geno0) and np.array_equal(geno1, gcross_table.golden_calls(t1.counts, TOTS[:, None], 1.5))


def test_likelihood_error_fits_the_knife_edge_width(ctx):
    """how far the device's ``likeli_one`` and numpy's ``likeliTest`` are from the 50-digit value, over every (y, n) with
    1 <= y < n <= 40.  A ratio of two such values carries both errors and one rounding of the division; twice that keeps a call
    from flipping when the two implementations err in opposite directions: 4 * max(e_dev, e_np) must fit the knife-edge width.
    The figures are printed; DESIGN.md section 13 records the measured ones."""
    lik = gcross_table.fixture()["lik"]
    y, n = np.nonzero(~np.isnan(lik))
    assert len(y) == 780 and y.min() == 1 and np.all(y < n) and n.max() == 40
    dev, _ = ctx.likelihood(y[:, None].astype(np.float64), n[:, None])                 # one point per row: the ratio column is 1
    e_dev = float(np.max(np.abs(dev[:, 0] - lik[y, n]) / lik[y, n]))               # (not |x / ref - 1|: that is quantised to 2^-53)
    e_np = float(np.max(np.abs(gcross_twin.likeli(n, y) - lik[y, n]) / lik[y, n]))
    print("likeliTest against 50 digits, 780 (y, n): e_dev = %.3e  e_np = %.3e  width = %.1e" % (e_dev, e_np, gcross_twin.KNIFE_EDGE_WIDTH))
    assert 4 * max(e_dev, e_np) <= gcross_twin.KNIFE_EDGE_WIDTH
