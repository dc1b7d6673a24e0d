"""The resident-panel scans at the most columns one call takes -- the width their ``*_cpu.py`` tests only see refused one column
later: 361 tiles of 32 columns (65 341 tile pairs on ``grid.x``, the whole triangle walk), one Gram split, 46 column blocks of
``admix``, 64 words per plane row of ``marker_select``, eight words in every lane of ``site_counts``, result cells near 2^31.

The pair scans limit the LIST, not the panel: a 300-accession x 1100-row panel (int8, and packed as the library lays it out by
itself) is listed out to the family's limit, ``cols = permutation(arange(LIMIT) % 300)``, as tests/test_gpu_mosaic.py does for
``mosaic``; all 1100 rows, two 1024-row steps.  The full-width result is compared with the twin on the sub-block of a dozen list
positions ``few`` -- both edges of the first two and the last two tiles and four in between, ascending, so that a rule that
prefers the smaller position reads the same -- the twin being called with ``cols[few]``.  Where a result depends on every column
or on the position itself, the twin runs at full width instead: ``loadings`` (every row compared), ``admix`` (Q', F' and ll, all
entries), ``marker_select`` (stopped after three picks; everything compared) and ``sim_counts`` (the twin's own simulated classes
at the true positions, contracted for the sub-block).  On the whole result: symmetry, cell by cell, where the scan promises it, and
two list positions that name the same panel column give the same row and the same column of cells.

``site_counts`` and ``ld_band`` limit the PANEL: a real panel of 16384 accessions x 200 rows, int8 and packed, against their twins."""
import time
import types

import numpy as np
import pytest

import ld_twin
import markers_twin
import power_twin
import scan_cases
import sitestats_twin
from snpmatch_amd import engine

pytestmark = pytest.mark.gpu

N_ROWS, N_ACC = 1100, 300
LAYOUTS = ["int8", "packed"]
LIMIT = {"kinship_counts": engine.KIN_MAX_ACCESSIONS, "f1_counts": engine.F1X_MAX_ACCESSIONS, "parent_counts": engine.F1X_MAX_ACCESSIONS,
         "ibd_counts": engine.F1X_MAX_ACCESSIONS, "mix_counts": engine.MIX_MAX_ACCESSIONS, "gram": engine.PCA_MAX_ACCESSIONS,
         "loadings": engine.PCA_MAX_ACCESSIONS, "admix": engine.PCA_MAX_ACCESSIONS, "sim_counts": engine.SIM_MAX_ACCESSIONS,
         "marker_select": engine.MK_MAX_ACCESSIONS}
TILE = 32
_cases = {}


def _calls(rng, n_rows, n_acc, other=False):
    v = rng.choice(np.array([-1, 0, 1, 2], dtype=np.int8), size=(n_rows, n_acc), p=[0.12, 0.45, 0.35, 0.08])
    if other:
        v[rng.random((n_rows, n_acc)) < 0.05] = 3
    return v


def _snps(layout):
    if layout not in _cases:
        v = _calls(np.random.default_rng(8100 + len(layout)), N_ROWS, N_ACC, other=layout == "int8")
        v.setflags(write=False)
        _cases[layout] = v
    return _cases[layout]


@pytest.fixture(scope="module", params=LAYOUTS)
def narrow(request):
    snps = _snps(request.param)
    panel = engine.Panel.from_host(engine.default_context(), snps, packed=request.param == "packed")
    yield panel, snps
    panel.free()


def _listing(scan):
    """(cols [LIMIT], few, arguments): the panel's columns listed out to the scan's limit, shuffled; the sampled positions"""
    limit = LIMIT[scan]
    assert limit % TILE == 0 and limit > 8 * TILE
    rng = np.random.default_rng(limit + len(scan))
    cols = rng.permutation(np.arange(limit) % N_ACC).astype(np.int32)
    edges = [0, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, limit - TILE - 1, limit - TILE, limit - 1]
    few = np.unique(np.concatenate([edges, rng.integers(2 * TILE + 1, limit - TILE - 1, size=4)]))
    a = scan_cases.make_args(rng, N_ROWS, limit, windows=400)
    a.grp_off, a.err_rate, a.mk_max = np.array([0, N_ROWS], dtype=np.int64), 0.2, 3
    return cols, few, a


def _namesake(cols, f):
    """another list position that names the panel column of position f"""
    same = np.flatnonzero(cols == cols[f])
    return int(same[same != f][0])


def _layers(scan, got):
    """the result as (name, array [..., n, n]) layers"""
    if isinstance(got, dict):
        return [(k, np.moveaxis(v, 2, 0) if v.ndim == 3 else v) for k, v in got.items() if isinstance(v, np.ndarray) and v.ndim >= 2]
    if isinstance(got, tuple):
        return [(str(i), v) for i, v in enumerate(got)]
    return [("", got)]


def _assert_symmetric(name, v, partner=None):
    """v == partner^T (partner: v itself), every cell"""
    assert np.array_equal(v, np.swapaxes(v if partner is None else partner, -1, -2)), "%s is not symmetric" % name


def _assert_namesakes_agree(name, v, cols, few, rows=True):
    for f in few.tolist():
        g = _namesake(cols, f)
        assert np.array_equal(v[..., :, f], v[..., :, g]), "%s: columns %d and %d of the cells name panel column %d" % (name, f, g, cols[f])
        assert not rows or np.array_equal(v[..., f, :], v[..., g, :]), "%s: rows %d and %d of the cells name panel column %d" % (name, f, g, cols[f])


def _sub(v, few):
    return v[..., few, :][..., :, few]


# scan -> the layers that are NOT symmetric / whose cells depend on the list positions (a tie goes to the smaller one)
POSITIONAL = {"parent_counts": {"2"}}            # w_first


@pytest.mark.parametrize("scan", ["kinship_counts", "f1_counts", "parent_counts", "ibd_counts", "gram"])
def test_pair_scan_at_its_limit(narrow, scan):
    panel, snps = narrow
    cols, few, a = _listing(scan)
    entry = scan_cases.SCANS[scan]
    t0 = time.time()
    got = entry.call(panel, a, cols, None)
    print("%s: %d columns, %.2f s on the device and back" % (scan, len(cols), time.time() - t0))
    want = entry.twin(snps, a, cols[few])

    def pick(v):
        return v[np.ix_(few, few)]                  # (the window bits of ``ibd_counts`` keep their third axis)
    picked = {k: pick(v) for k, v in got.items()} if isinstance(got, dict) else tuple(pick(v) for v in got) if isinstance(got, tuple) else pick(got)
    entry.check(picked, want, snps, a, cols[few])
    for k, (name, v) in enumerate(_layers(scan, got)):
        assert v.shape[-2:] == (len(cols), len(cols)) and (k or v.any())
        if name in POSITIONAL.get(scan, ()):
            continue
        _assert_symmetric(scan + " " + name, v)
        _assert_namesakes_agree(scan + " " + name, v, cols, few)


def test_mix_counts_at_its_limit(narrow):
    panel, snps = narrow
    cols, few, a = _listing("mix_counts")
    entry = scan_cases.SCANS["mix_counts"]
    t0 = time.time()
    got = entry.call(panel, a, cols, None)
    print("mix_counts: %d columns, %.2f s on the device and back" % (len(cols), time.time() - t0))
    entry.check(_sub(got, few), entry.twin(snps, a, cols[few]), snps, a, cols[few])
    for w in range(2):                              # table[w, ca, cb, a, b] == table[w, cb, ca, b, a]
        for ca in range(2):
            for cb in range(ca, 2):
                _assert_symmetric("table[%d, %d, %d]" % (w, ca, cb), got[w, ca, cb], got[w, cb, ca])
    _assert_namesakes_agree("table", got, cols, few)


def test_loadings_at_their_limit(narrow):
    panel, snps = narrow
    cols, _, a = _listing("loadings")
    entry = scan_cases.SCANS["loadings"]
    got = entry.call(panel, a, cols, None)
    assert got.any()
    entry.check(got, entry.twin(snps, a, cols), snps, a, cols)           # integer table and integer vec: every row, bit for bit


def test_admix_at_its_limit(narrow):
    panel, snps = narrow
    cols, _, a = _listing("admix")
    entry = scan_cases.SCANS["admix"]
    t0 = time.time()
    got = entry.call(panel, a, cols, None)
    print("admix: %d columns, %.2f s on the device and back" % (len(cols), time.time() - t0))
    entry.check(got, entry.twin(snps, a, cols), snps, a, cols)           # Q', F' and ll, every entry, within the bound of the narrow tests


def test_marker_select_at_its_limit(narrow):
    """the twin at full width; the namesakes of a column can never be told apart, so the call stops at ``max_markers``"""
    panel, snps = narrow
    cols, few, a = _listing("marker_select")
    entry = scan_cases.SCANS["marker_select"]
    got = entry.call(panel, a, cols, None)
    want = entry.twin(snps, a, cols)
    assert want["stop_reason"] == markers_twin.STOP_MAX_MARKERS and want["n_chosen"] == a.mk_max
    entry.check(got, want, snps, a, cols)
    assert np.array_equal(got["need"], got["need"].T)
    assert np.array_equal(_sub(got["need"], few), markers_twin.replay(snps, got["chosen"], a.mk_depth, cols[few]))


def _sim_block(snps, a, cols, few):
    """(score, ninfo) [n_grp, len(few), len(few)] of samples ``few`` against columns ``few``: the twin's simulated classes of the whole
    list -- the noise of a sample is keyed by its position -- and the two contractions of ``power_twin.sim_counts`` on the sub-block"""
    cls = power_twin.sample_classes(snps[:, cols], power_twin.err_threshold(a.err_rate), a.seed)[:, few]
    v = snps[:, cols[few]]
    score, ninfo = (np.zeros((len(a.grp_off) - 1, len(few), len(few)), dtype=np.int32) for _ in range(2))
    for g, (lo, hi) in enumerate(zip(a.grp_off[:-1], a.grp_off[1:])):
        cg, vg = cls[lo:hi], v[lo:hi]
        score[g] = sum((cg == c).astype(np.int64).T @ (vg == c).astype(np.int64) for c in (0, 1, 2))
        ninfo[g] = (cg != power_twin.NO_CALL).astype(np.int64).T @ (vg >= 0).astype(np.int64)
    return score, ninfo


def _check_sim(panel, snps, cols, few, a):
    t0 = time.time()
    got = scan_cases.SCANS["sim_counts"].call(panel, a, cols, None)
    seconds = time.time() - t0
    n_grp = len(a.grp_off) - 1
    scan_cases.assert_equal(tuple(_sub(v, few) for v in got), _sim_block(snps, a, cols, few))
    for name, v in zip(("score", "ninfo"), got):
        assert v.shape == (n_grp, len(cols), len(cols)) and all(v[g].any() for g in (0, n_grp - 1))
        _assert_namesakes_agree(name, v, cols, few, rows=False)           # (the sample of a row of cells carries the noise of its position)
    return seconds


def test_sim_counts_at_its_limit(narrow):
    panel, snps = narrow
    cols, few, a = _listing("sim_counts")
    print("sim_counts: 1 group x %d columns, %.2f s on the device and back" % (len(cols), _check_sim(panel, snps, cols, few, a)))


def test_sim_counts_at_the_most_cells_its_guard_admits():
    """16 groups x 11552 columns: 16 x 11552^2 < 2^31 <= 17 x 11552^2; the cell index of the last group runs up to 2^31 - 12 million"""
    snps = _snps("packed")
    n = engine.SIM_MAX_ACCESSIONS
    assert 16 * n * n < 1 << 31 <= 17 * n * n
    cols, few, a = _listing("sim_counts")
    a.grp_off = np.linspace(0, N_ROWS, 17).astype(np.int64)
    panel = engine.Panel.from_host(engine.default_context(), snps, packed=True)
    try:
        print("sim_counts: 16 groups x %d columns, %.2f s on the device and back" % (n, _check_sim(panel, snps, cols, few, a)))
    finally:
        panel.free()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_site_counts_and_ld_band_on_the_widest_panel(layout):
    n_acc = 64 * 8 * 32                              # WAVE * SITE_WORDS * 32 = LD_MAX_ACCESSIONS
    snps = _calls(np.random.default_rng(8300), 200, n_acc, other=layout == "int8")
    snps[3], snps[4] = 0, -1                         # a monomorphic row and one without a call
    panel = engine.Panel.from_host(engine.default_context(), snps, packed=layout == "packed")
    try:
        got = engine.site_counts(panel)
        scan_cases.assert_equal(got, sitestats_twin.site_counts(snps))
        assert got[0, :, 3].max() > 14000
        rows = np.random.default_rng(8301).permutation(200)[:150].astype(np.int64)
        scan_cases.assert_equal(engine.site_counts(panel, rows=rows), sitestats_twin.site_counts(snps, None, rows))
        a = types.SimpleNamespace(band=8)
        entry = scan_cases.SCANS["ld_band"]
        entry.check(entry.call(panel, a, None, None), ld_twin.ld_band(snps, 8), snps, a, None)
        entry.check(entry.call(panel, a, None, rows), ld_twin.ld_band(snps, 8, None, rows), snps[rows], a, None)
    finally:
        panel.free()
