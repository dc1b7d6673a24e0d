"""pca on the device: ``snpm_panel_gram`` (``k_win_planes`` + ``k_pca_gram`` + ``k_pca_fold``) and ``snpm_panel_loadings``
(``k_pca_load``) against the numpy twin (tests/pca_twin.py) on panels filled through the normal upload path in each of the three
layouts (int8, packed whole rows, packed split rows).  Tables of small integers make every partial sum an exact integer: those cases
are compared bit for bit, at the shapes where the decomposition could break -- 64 accessions per tile side (T - 1, T, T + 1, 2 T + 1),
64 rows per word, 32 rows per pass, 1024 rows per plane step, slabs of the row axis.  Tables of ``standardise`` are compared with the
exactly rounded sums (``math.fsum`` of exact products) within the bound of ANY order of summation: R products, each partial sum rounded
once, |error| <= R 2^-53 sum |t||t| to first order; the tests allow twice that, as the issue sets it."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import kinship_twin
import pca_twin as twin
import sitestats_twin
import test_pca_cpu as cpu
from snpmatch_amd import _lib, cli, engine
from snpmatch_amd.core import pca

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = ["int8", "packed", "split"]
TILE = 64               # accessions per tile side of k_pca_gram (PCA_TILE of csrc/snpm_k_pca.hpp)
U = 2.0 ** -53
KERNELS = ("pca_gram", "pca_fold", "pca_load")


@pytest.fixture(scope="module")
def ctx():
    return engine.default_context()


def _calls(rng, n_rows, n_acc, other=False):
    v = rng.choice(np.array([-1, 0, 1, 2], dtype=np.int8), size=(n_rows, n_acc), p=[0.12, 0.45, 0.35, 0.08])
    if other:
        v[rng.random((n_rows, n_acc)) < 0.05] = 3
    return v


def _panel(ctx, snps, layout, monkeypatch):
    """the normal upload path; packed panels are split (main part + ragged tail) wherever that saves memory, SNPM_PACKED_SPLIT=0
    keeps whole rows"""
    if layout == "packed":
        monkeypatch.setenv("SNPM_PACKED_SPLIT", "0")
    panel = engine.Panel.from_host(ctx, snps, packed=layout != "int8")
    monkeypatch.delenv("SNPM_PACKED_SPLIT", raising=False)
    return panel


def _twin_rows(rows):
    return None if rows is None else (np.arange(rows.start, rows.stop) if isinstance(rows, range) else rows)


def _check_exact(panel, snps, rng, cols=None, rows=None, k=2, tab=None):
    """integer table, integer vec: both results equal to the twin bit for bit; the matrix symmetric"""
    n_rows = panel.n_snp if rows is None else len(rows)
    ncols = panel.n_acc if cols is None else len(cols)
    tab = twin.integer_table(rng, n_rows) if tab is None else tab
    got = engine.gram(panel, tab, cols, rows)
    want = twin.gram(snps, tab, cols, _twin_rows(rows))
    assert got.dtype == np.float64 and got.shape == (ncols, ncols) and np.array_equal(got, got.T)
    assert np.array_equal(got, want), "gram differs in %d cells" % int((got != want).sum())
    vec = rng.integers(-4, 5, size=(ncols, k)).astype(np.float64)
    load = engine.loadings(panel, tab, vec, cols, rows)
    want = twin.loadings(snps, tab, vec, cols, _twin_rows(rows))
    assert load.dtype == np.float64 and load.shape == (n_rows, k)
    assert np.array_equal(load, want), "loadings differ in %d cells" % int((load != want).sum())
    return got, load


# ------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n_acc", [1, 2, 31, 32, 33, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 130])
def test_tile_edges_of_accessions_words_passes_and_steps_of_rows(n_acc, layout, ctx, monkeypatch):
    rng = np.random.default_rng(1000 + n_acc)
    snps = _calls(rng, 2503, n_acc)
    panel = _panel(ctx, snps, layout, monkeypatch)
    for at, n_rows in enumerate((1, 63, 64, 65, 1023, 1024, 1025, 2500)):
        _check_exact(panel, snps, rng, rows=range(3, 3 + n_rows), k=(1, 2, 10, 32)[at % 4])
    panel.free()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k", [1, 2, 10, 32])
def test_every_group_of_components(k, layout, ctx, monkeypatch):
    rng = np.random.default_rng(1500 + k)
    snps = _calls(rng, 300, 70)
    panel = _panel(ctx, snps, layout, monkeypatch)
    _check_exact(panel, snps, rng, k=k)
    _check_exact(panel, snps, rng, rows=range(0, 1), k=k)
    panel.free()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_lists_ranges_missing_rows_and_the_other_code(layout, ctx, monkeypatch):
    rng = np.random.default_rng(2000)
    snps = _calls(rng, 400, 90, other=layout == "int8")
    snps[100:180] = -1                                              # rows that are all missing
    panel = _panel(ctx, snps, layout, monkeypatch)
    cols = np.arange(89, 20, -1)                                    # descending, with repeats
    cols[5], cols[-1] = cols[4], cols[0]
    _check_exact(panel, snps, rng, cols=cols, k=10)
    rows = rng.integers(0, 400, size=333)                           # unsorted, with repeats
    rows[7] = rows[6]
    _check_exact(panel, snps, rng, rows=rows, k=2)
    _check_exact(panel, snps, rng, cols=cols, rows=rows, k=32)
    _check_exact(panel, snps, rng, rows=range(57, 400), k=1)        # a dense range with row0 > 0
    got, load = _check_exact(panel, snps, rng, rows=range(100, 180), k=2, tab=np.full((80, 4), 3.0))
    assert not got.any() and not load.any()
    if layout == "int8":                                            # the "other" code takes the fourth entry of its row
        tab = np.zeros((400, 4))
        tab[:, 3] = 2.0
        got, _ = _check_exact(panel, snps, rng, tab=tab)
        assert np.array_equal(np.diag(got), 4.0 * (snps == 3).sum(axis=0)) and got.any()
    # calls that do no work
    assert engine.gram(panel, np.zeros((0, 4)), rows=range(5, 5)).tolist() == np.zeros((90, 90)).tolist()
    assert engine.gram(panel, np.zeros((400, 4)), cols=[]).shape == (0, 0)
    assert engine.loadings(panel, np.zeros((0, 4)), np.ones((90, 3)), rows=range(0, 0)).shape == (0, 3)
    panel.free()


@functools.lru_cache(maxsize=None)
def _big(n_acc, n_rows, other):
    return _calls(np.random.default_rng(3000 + n_acc), n_rows, n_acc, other)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", [(130, 2500), (1135, 3000)])
def test_wide_panel_exact_and_against_the_kinship_counts(shape, layout, ctx, monkeypatch):
    """1135 columns x 3000 rows exactly; and two tables whose Gram matrices are counts the package already serves: (1, 1, 1, 1)
    gives ninfo of ``kinship_counts`` over the same selection, (1, -1, 0, 0) gives same - diff"""
    n_acc, n_rows = shape
    snps = _big(n_acc, n_rows, layout == "int8")
    panel = _panel(ctx, snps, layout, monkeypatch)
    rng = np.random.default_rng(3100)
    _check_exact(panel, snps, rng, k=10)
    ninfo, same, diff = engine.kinship_counts(panel)
    assert np.array_equal(ninfo, kinship_twin.kinship_counts(snps)[0])
    ones = engine.gram(panel, np.ones((n_rows, 4)))
    assert np.array_equal(ones, ninfo.astype(np.float64))
    hom = engine.gram(panel, np.tile(np.array([1.0, -1.0, 0.0, 0.0]), (n_rows, 1)))
    assert np.array_equal(hom, (same.astype(np.int64) - diff.astype(np.int64)).astype(np.float64))
    rows = np.random.default_rng(3200).integers(0, n_rows, size=1500)
    ninfo, same, diff = engine.kinship_counts(panel, None, rows)
    assert np.array_equal(engine.gram(panel, np.ones((1500, 4)), None, rows), ninfo.astype(np.float64))
    panel.free()


# ------------------------------------------------------------------------------------------------ real tables
EXACT_CELL_ROWS = {130: None, 1135: [0, 1, TILE - 1, TILE, TILE + 1, 500, 1087, 1088, 1134]}     # (None: every cell)
REAL_K = {130: 10, 1135: 4}


@functools.lru_cache(maxsize=None)
def _real_case(n_acc, n_rows):
    """a panel with allele frequencies down to 0.01 (|t| reaches about 10), its table from ``standardise`` over ALL its rows (rows
    that fail keep a zero table), the exactly rounded references and the sums of absolute products -- computed once, read-only"""
    rng = np.random.default_rng(4000 + n_acc)
    freq = np.concatenate([rng.uniform(0.01, 0.06, n_rows // 3), rng.uniform(0.06, 0.94, n_rows - n_rows // 3)])
    snps = (rng.random((n_rows, n_acc)) < freq[:, None]).astype(np.int8)
    u = rng.random((n_rows, n_acc))
    snps[u < 0.04] = 2
    snps[u > 0.95] = -1
    keep, tab, p, _ = pca.standardise(sitestats_twin.site_counts(snps)[0], n_acc, 0.01, 0.1)
    assert keep.sum() > 0.8 * n_rows and np.abs(tab).max() > 8.0
    cell_rows = EXACT_CELL_ROWS[n_acc]
    g_ref = twin.gram_exact(snps, tab, cell_rows=cell_rows)
    vec = pca.decompose(twin.gram(snps, tab), int(keep.sum()), REAL_K[n_acc])[1]
    case = {"snps": snps, "tab": tab, "vec": vec, "gram_ref": g_ref, "gram_abs": twin.gram_abs(snps, tab), "gram_twin": twin.gram(snps, tab),
            "load_ref": twin.loadings_exact(snps, tab, vec), "load_abs": twin.loadings_abs(snps, tab, vec)}
    for a in case.values():
        a.setflags(write=False)
    return case


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", [(130, 2500), (1135, 3000)])
def test_standardised_tables_within_the_bound_of_any_summation_order(shape, layout, ctx, monkeypatch):
    """|gram - ref| <= 2 R 2^-53 S with S = sum |t||t|, |load - ref| <= 2 ncols 2^-53 sum |t||vec|, ref exactly rounded.  At 1135
    columns the exactly rounded matrix costs minutes in Python: it is made for nine rows of cells (the edges of the first tiles and of
    the last, partial one; by the bit-for-bit symmetry asserted here, for those columns too), and every cell is held against numpy's
    own order of summation within the same figure (both lie within R 2^-53 S of the exact sum).  The same call twice: same bits."""
    n_acc, n_rows = shape
    c = _real_case(n_acc, n_rows)
    panel = _panel(ctx, c["snps"], layout, monkeypatch)
    got = engine.gram(panel, c["tab"])
    bound = 2.0 * n_rows * U * c["gram_abs"]
    cell_rows = EXACT_CELL_ROWS[n_acc]
    sub = got if cell_rows is None else got[cell_rows]
    err = np.abs(sub - c["gram_ref"])
    print("gram %s %s: worst error / bound %.4f" % (shape, layout, float((err / (bound if cell_rows is None else bound[cell_rows])).max())))
    assert (err <= (bound if cell_rows is None else bound[cell_rows])).all()
    assert (np.abs(got - c["gram_twin"]) <= bound).all() and np.array_equal(got, got.T)
    load = engine.loadings(panel, c["tab"], c["vec"])
    bound = 2.0 * n_acc * U * c["load_abs"]
    err = np.abs(load - c["load_ref"])
    print("loadings %s %s: worst error / bound %.4f" % (shape, layout, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all()
    assert np.array_equal(engine.gram(panel, c["tab"]), got) and np.array_equal(engine.loadings(panel, c["tab"], c["vec"]), load)
    panel.free()


# ------------------------------------------------------------------------------------------------ slabs
def test_three_slabs_with_a_partial_last_one(tmp_path):
    """a fresh process (snpm_init reads the knob) under SNPM_PCA_WS_MB=1: 33 accessions pad to 64 plane rows, a plane step and its
    table rows take 4 * 64 * 128 + 32768 = 65536 bytes, so a slab holds 16 steps = 16384 rows and 33768 rows are two whole slabs and
    one of 1000 rows; the loadings (k = 10: 120 bytes per row) go in slabs of 8738 rows.  Integer table: equal to the twin; the
    standardised table: within the bound (exactly rounded reference for the first and the last row of cells)."""
    rng = np.random.default_rng(5000)
    n_rows, n_acc, k = 2 * 16384 + 1000, 33, 10
    freq = rng.uniform(0.02, 0.98, n_rows)
    snps = (rng.random((n_rows, n_acc)) < freq[:, None]).astype(np.int8)
    snps[rng.random((n_rows, n_acc)) < 0.05] = -1
    tab_int = twin.integer_table(rng, n_rows)
    tab_real = pca.standardise(sitestats_twin.site_counts(snps)[0], n_acc, 0.01, 0.2)[1]
    vec_int = rng.integers(-4, 5, size=(n_acc, k)).astype(np.float64)
    vec_real = rng.normal(size=(n_acc, k))
    np.savez(tmp_path / "in.npz", snps=snps, tab_int=tab_int, tab_real=tab_real, vec_int=vec_int, vec_real=vec_real)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pca_ws_worker.py"), str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       capture_output=True, text=True, env=dict(os.environ, SNPM_PCA_WS_MB="1"), timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    z = np.load(tmp_path / "out.npz")
    assert z["launches"].tolist() == [3, 3, 3, 4]                  # win_planes, pca_gram, pca_fold per slab; pca_load per slab of loadings
    assert np.array_equal(z["gram_int"], twin.gram(snps, tab_int)) and np.array_equal(z["load_int"], twin.loadings(snps, tab_int, vec_int))
    bound = 2.0 * n_rows * U * twin.gram_abs(snps, tab_real)
    assert (np.abs(z["gram_real"][[0, n_acc - 1]] - twin.gram_exact(snps, tab_real, cell_rows=[0, n_acc - 1])) <= bound[[0, n_acc - 1]]).all()
    assert (np.abs(z["gram_real"] - twin.gram(snps, tab_real)) <= bound).all() and np.array_equal(z["gram_real"], z["gram_real"].T)
    some = np.concatenate([np.arange(0, 3), np.arange(8736, 8740), np.arange(16383, 16386), np.arange(n_rows - 2, n_rows)])
    ref = twin.loadings_exact(snps[some], tab_real[some], vec_real)
    assert (np.abs(z["load_real"][some] - ref) <= 2.0 * n_acc * U * twin.loadings_abs(snps[some], tab_real[some], vec_real)).all()
    assert (np.abs(z["load_real"] - twin.loadings(snps, tab_real, vec_real)) <= 2.0 * n_acc * U * twin.loadings_abs(snps, tab_real, vec_real)).all()


# ------------------------------------------------------------------------------------------------ the command
def test_command_end_to_end_on_the_planted_panel(ctx, tmp_path):
    case = twin.planted_case(cpu.PLANTED_COMMAND_SEED)
    db, pops, accs, vcf = cpu.write_planted_inputs(case, tmp_path)
    out = str(tmp_path / "out")
    assert cli.main(["pca", "-d", db, "--pops", pops, "-i", vcf, "-o", out]) == 0
    stats, z = cpu.check_planted_outputs(case, out)
    res = pca.analyse(cpu.TwinGenotype(case["snps"]), case["panel"], 36, np.arange(600), 0.05, 0.1, 10)
    assert np.array_equal(z["table"], res["tab"]) and np.allclose(z["eigenvalues"], res["eigenvalues"], rtol=1e-12)
    assert np.allclose(z["eigenvectors"][:, :2], res["vec"][:, :2], rtol=0, atol=1e-9)
    assert cli.main(["pca", "-d", db, "-a", accs, "--components", "3", "--keep_grm", "-o", out]) == 0
    cpu.check_planted_outputs(case, out, k=3, with_pops=False, with_projection=False)


# ------------------------------------------------------------------------------------------------ refusals that need a panel
def test_refusals_that_need_a_panel_launch_nothing(ctx):
    snps = _calls(np.random.default_rng(6000), 50, 20)
    panel = engine.Panel.from_host(ctx, snps, packed=False)
    tab, vec = np.ones((50, 4)), np.ones((20, 3))
    ctx.profile(True)
    ctx.profile_reset()
    try:
        def refused(call, text):
            with pytest.raises(AssertionError) as err:         # (SNPM_ERR_BADARG: ``_lib.check`` raises it as the reference's assert)
                call()
            assert text in str(err.value), str(err.value)
        refused(lambda: engine.gram(panel, np.ones((2, 4)), cols=[0, 20], rows=range(0, 2)), "accession index outside the panel")
        refused(lambda: engine.gram(panel, np.ones((2, 4)), cols=[-1], rows=range(0, 2)), "accession index outside the panel")
        refused(lambda: engine.loadings(panel, np.ones((2, 4)), np.ones((1, 1)), cols=[20], rows=range(0, 2)), "accession index outside the panel")
        refused(lambda: engine.gram(panel, np.ones((2, 4)), rows=np.array([0, 50])), "row index outside the panel")
        refused(lambda: engine.loadings(panel, np.ones((2, 4)), vec, rows=np.array([-1, 5])), "row index outside the panel")
        out = np.zeros((19, 19))
        rc = ctx.lib.snpm_panel_gram(panel.h, None, 19, None, 0, 50, _lib.ptr(tab), _lib.ptr(out))
        assert rc == _lib.SNPM_ERR_BADARG and "cols is NULL (all accessions)" in ctx.lib.snpm_last_error(ctx.h).decode()
        rc = ctx.lib.snpm_panel_loadings(panel.h, None, 19, None, 0, 50, _lib.ptr(tab), _lib.ptr(vec), 3, _lib.ptr(np.zeros((50, 3))))
        assert rc == _lib.SNPM_ERR_BADARG and "cols is NULL (all accessions)" in ctx.lib.snpm_last_error(ctx.h).decode()
        for poison in (np.nan, np.inf):
            t = tab.copy()
            t[49, 2] = poison
            refused(lambda: engine.gram(panel, t), "tab holds a value that is not finite")
            refused(lambda: engine.loadings(panel, t, vec), "tab holds a value that is not finite")
            v = vec.copy()
            v[19, 2] = poison
            refused(lambda: engine.loadings(panel, tab, v), "vec holds a value that is not finite")
        refused(lambda: engine.loadings(panel, tab, np.ones((20, 33))), "k outside 1 .. SNPM_PCA_MAX_COMPONENTS")
        assert [ctx.profile_read(name)[0] for name in KERNELS + ("win_planes",)] == [0, 0, 0, 0]
        # ... and sound calls do launch: one slab each
        engine.gram(panel, tab)
        engine.loadings(panel, tab, vec)
        assert [ctx.profile_read(name)[0] for name in KERNELS + ("win_planes",)] == [1, 1, 1, 1]
    finally:
        ctx.profile(False)
        panel.free()
