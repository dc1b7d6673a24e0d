"""The resident-panel scans of ``snpmatch_amd.engine`` as ONE table for the tests that walk all of them (test infrastructure):
scan -> how it is called on a panel, what its numpy twin gives on the same rows held in memory, and how the two are compared.

Every entry takes its further arguments (sample classes, window / chain / group offsets, class table, read counts ...) from one
namespace ``a``, see ``make_args``, so the same table serves a 70-row panel and the last rows of a 16-million-row one.  The twin
is always handed the SELECTED rows as a small int8 array [n_sel, n_acc] and ``rows=None``; ``cols`` is the column list of the call or
None.  Integer results are compared with ``array_equal`` (and dtype and shape), the r2 of ``ld_band`` as tests/test_gpu_ld.py compares
it (fp64 bits, nan where the twin has nan), ``admix`` with the bound of tests/test_gpu_admixture.py (``worst_ratios`` <= 1 against the
long-double iteration).  No tolerance is made here."""
import collections
import types

import numpy as np

import admixture_twin
import f1search_twin
import ibd_twin
import kinship_twin
import ld_twin
import markers_twin
import mixture_twin
import mosaic_twin
import parentsearch_twin
import pca_twin
import power_twin
import sitestats_twin
import windows_twin
from snpmatch_amd import engine

# call(panel, a, cols, rows) -> the device's result; twin(sel, a, cols) -> the expected one from sel int8 [n_sel, n_acc];
# check(got, want, sel, a, cols) asserts; counts_integers: the result does not depend on the order of summation
Scan = collections.namedtuple("Scan", "call twin check counts_integers")


def assert_equal(got, want, what=""):
    """the same structure, and every array equal with its dtype and shape"""
    if isinstance(want, dict):
        assert isinstance(got, dict) and sorted(got) == sorted(want), what
        for k in want:
            assert_equal(got[k], want[k], "%s[%r]" % (what, k))
    elif isinstance(want, (tuple, list)):
        assert isinstance(got, (tuple, list)) and len(got) == len(want), what
        for i, (g, w) in enumerate(zip(got, want)):
            assert_equal(g, w, "%s[%d]" % (what, i))
    elif isinstance(want, np.ndarray):
        assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape, (what, getattr(got, "dtype", None), getattr(got, "shape", None))
        assert np.array_equal(got, want), "%s: %d of %d entries differ" % (what, int((got != want).sum()), want.size)
    else:
        assert got == want, (what, got, want)            # None, and the integers of ``marker_select``


def _check_equal(got, want, sel, a, cols):
    assert_equal(got, want)


def _check_ld(got, want, sel, a, cols):
    assert_equal(got[0], want[0], "counts")
    r2, ref = got[1], want[1]
    nan = np.isnan(ref)
    assert r2.dtype == np.float64 and r2.shape == ref.shape and np.array_equal(np.isnan(r2), nan)
    assert np.array_equal(r2[~nan].view(np.uint64), ref[~nan].view(np.uint64)) and (r2[~nan] <= 1.0).all()


def _check_admix(got, want, sel, a, cols):
    Qn, Fn, ll = got
    assert Qn.dtype == Fn.dtype == ll.dtype == np.float64 and Qn.shape == a.Q.shape and Fn.shape == a.F.shape and ll.shape == (1,)
    ratios = admixture_twin.worst_ratios((Qn, Fn, ll[0]), want, sel, cols, None)
    print("admix: worst error / bound F %.4f Q %.4f ll %.4f" % ratios)
    assert max(ratios) <= 1.0, ratios


def _admix_reference(sel, a, cols):
    assert a.n_iter == 1, "the long-double reference is one iteration"
    return admixture_twin.step(sel, a.Q, a.F, cols, None, dtype=np.longdouble)


SCANS = {
    "kinship_counts": Scan(lambda p, a, c, r: engine.kinship_counts(p, c, r),
                           lambda s, a, c: kinship_twin.kinship_counts(s, c), _check_equal, True),
    "f1_counts": Scan(lambda p, a, c, r: engine.f1_counts(p, a.cls[0], c, r),
                      lambda s, a, c: f1search_twin.f1_counts(s, a.cls[0], c), _check_equal, True),
    "parent_counts": Scan(lambda p, a, c, r: engine.parent_counts(p, a.cls[0], a.win_off, a.par_min_sites, c, r),
                          lambda s, a, c: parentsearch_twin.parent_counts(s, a.cls[0], a.win_off, a.par_min_sites, c), _check_equal, True),
    "ibd_counts": Scan(lambda p, a, c, r: engine.ibd_counts(p, a.win_off, a.ibd[0], a.ibd[1], a.ibd[2], c, r),
                       lambda s, a, c: ibd_twin.ibd_counts(s, a.win_off, a.ibd[0], a.ibd[1], a.ibd[2], c), _check_equal, True),
    "mix_counts": Scan(lambda p, a, c, r: engine.mix_counts(p, a.alt, a.ref, c, r),
                       lambda s, a, c: mixture_twin.mix_counts(s, a.alt, a.ref, c), _check_equal, True),
    "marker_select": Scan(lambda p, a, c, r: engine.marker_select(p, a.mk_depth, a.mk_max, None, 0, None, c, r),
                          lambda s, a, c: markers_twin.marker_select(s, a.mk_depth, a.mk_max, cols=c), _check_equal, True),
    "sim_counts": Scan(lambda p, a, c, r: engine.sim_counts(p, a.grp_off, a.err_rate, a.seed, c, r),
                       lambda s, a, c: power_twin.sim_counts(s, a.grp_off, power_twin.err_threshold(a.err_rate), a.seed, c), _check_equal, True),
    "mosaic": Scan(lambda p, a, c, r: engine.mosaic(p, a.cls, a.chain_off, a.cost, a.switch, c, r, want_col_cost=True),
                   lambda s, a, c: mosaic_twin.mosaic(s, a.cls, a.chain_off, a.cost, a.switch, c), _check_equal, True),
    "site_counts": Scan(lambda p, a, c, r: engine.site_counts(p, c, r),
                        lambda s, a, c: sitestats_twin.site_counts(s, c), _check_equal, True),
    "ld_band": Scan(lambda p, a, c, r: engine.ld_band(p, a.band, c, r),
                    lambda s, a, c: ld_twin.ld_band(s, a.band, c), _check_ld, True),
    "window_counts": Scan(lambda p, a, c, r: engine.window_counts(p, a.win_off, c, a.pairs, r),
                          lambda s, a, c: windows_twin.window_counts(s, a.win_off, c, a.pairs), _check_equal, True),
    "gram": Scan(lambda p, a, c, r: engine.gram(p, a.tab, c, r),
                 lambda s, a, c: pca_twin.gram(s, a.tab, c), _check_equal, False),
    "loadings": Scan(lambda p, a, c, r: engine.loadings(p, a.tab, a.vec, c, r),
                     lambda s, a, c: pca_twin.loadings(s, a.tab, a.vec, c), _check_equal, False),
    "admix": Scan(lambda p, a, c, r: engine.admix(p, a.Q, a.F, a.n_iter, c, r), _admix_reference, _check_admix, False),
}


def window_offsets(n_rows, size):
    """offsets into ``n_rows`` selected rows: windows of ``size`` rows, an EMPTY one after the first, the last one ragged"""
    cuts = list(range(0, n_rows, size)) + [n_rows]
    return np.array(cuts[:2] + cuts[1:], dtype=np.int64)


def make_args(rng, n_rows, ncols, windows=50):
    """the further arguments of every scan of the table for a selection of ``n_rows`` rows and a call of ``ncols`` columns, drawn
    from ``rng``: integer class table and integer ``vec`` (``gram`` and ``loadings`` are then exact integers, so equal bit for bit),
    read counts up to 255, windows of ``windows`` rows with an empty one among them (so are the chains and the groups, longer), an
    ``ibd`` threshold in the middle of what unrelated columns give, ``marker_select`` stopped after four picks, one ``admix``
    iteration with K = 3.  The pairs of ``window_counts`` and the rows of ``vec`` and ``Q`` are positions in a list of ``ncols``."""
    a = types.SimpleNamespace()
    a.cls = rng.choice(np.array([0, 1, 2, 0xFF], dtype=np.uint8), size=(2, n_rows), p=[0.4, 0.35, 0.15, 0.1])
    a.win_off = window_offsets(n_rows, windows)
    a.par_min_sites = 3
    a.ibd = (5, 470000, 2)                      # min_win_sites, max_diff_ppm, min_run
    a.alt, a.ref = (np.where(rng.random(n_rows) < 0.25, 0, rng.integers(0, 256, n_rows)).astype(np.uint8) for _ in range(2))
    a.alt[n_rows // 2] = 255                    # the largest count
    a.mk_depth, a.mk_max = 1, 4
    a.grp_off = window_offsets(n_rows, max(1, n_rows // 3 + 1))
    a.err_rate, a.seed = 0.01, 5
    a.chain_off = window_offsets(n_rows, max(1, n_rows // 2 + 7))
    a.cost = np.array([[0, 2, 1, 2], [2, 0, 1, 2], [1, 1, 0, 2]], dtype=np.uint8)
    a.switch = 5
    a.band = 5
    a.pairs = np.concatenate([rng.integers(0, ncols, size=(30, 2)), [[0, ncols - 1], [ncols - 1, 0], [ncols // 2, ncols // 2]]]).astype(np.int32)
    a.tab = pca_twin.integer_table(rng, n_rows)
    a.vec = rng.integers(-3, 4, size=(ncols, 3)).astype(np.float64)
    a.Q, a.F = admixture_twin.random_start(rng, ncols, n_rows, 3)
    a.n_iter = 1
    return a
