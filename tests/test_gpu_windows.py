"""Panel windows on the device: ``snpm_panel_window_counts`` / ``k_win_planes`` + ``k_win_count`` against the numpy twin
(tests/windows_twin.py), cell by cell as integers and the derived values as fp64 bits, on panels filled through the normal upload
path in each of the three layouts, at the smallest shapes where each mechanism could break: 64 accessions per plane tile, 64 rows per
word with window edges at bits 0, 1, 63, 64 and 65, 1024 rows per plane step (2200 rows: more than two), groups of 1 to 64 lanes per
cell, slabs of the row axis with a window across all of them; the selections, each output alone, the cross-checks against the
kernels of site statistics and kinship, and the two ``Genotype`` methods against a golden of the reference."""
import os
import subprocess
import sys

import numpy as np
import pytest

import windows_twin
from snpmatch_amd import engine
from snpmatch_amd.core import genomes, snp_genotype

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = ["int8", "packed", "split"]
N_ROWS = 2200               # more than two plane steps of 1024 rows
# every edge case in one table: an empty window first, edges at bits 0, 1, 63, 64 and 65 of a word, an empty window in the middle,
# a one-row window (65), windows inside one word, a window longer than a plane step (192 .. 1400), an empty window last
EDGES = np.array([0, 0, 1, 63, 64, 65, 65, 66, 127, 129, 192, 1400, 2100, N_ROWS, N_ROWS], dtype=np.int64)
ONE = np.array([0, N_ROWS], dtype=np.int64)
_panels, _twins = {}, {}


@pytest.fixture(scope="module")
def ctx():
    return engine.default_context()


def calls_of(n_acc, other):
    """the calls of the shape grid, made once per width: -1 / 0 / 1 / 2, int8 panels also 3"""
    if (n_acc, other) not in _panels:
        rng = np.random.default_rng(6000 + n_acc)
        v = rng.choice(np.array([-1, 0, 1, 2], dtype=np.int8), size=(N_ROWS, n_acc), p=[0.12, 0.45, 0.35, 0.08])
        if other:
            v[rng.random(v.shape) < 0.05] = 3
        v[200:260] = -1                      # rows without a call, inside the long window
        _panels[(n_acc, other)] = v
    return _panels[(n_acc, other)]


def pairs_of(n_acc):
    """(a, a), (a, b), (b, a) and two more"""
    a, b = 0, n_acc - 1
    return np.array([(a, a), (a, b), (b, a), (n_acc // 2, b), (n_acc // 3, n_acc // 2)], dtype=np.int64)


def twin_of(n_acc, other, table):
    """the twin's (acc, pair) of all rows, computed once and shared by the layouts; never written to"""
    key = (n_acc, other, len(table))
    if key not in _twins:
        _twins[key] = windows_twin.window_counts(calls_of(n_acc, other), table, None, pairs_of(n_acc))
        for a in _twins[key]:
            a.setflags(write=False)
    return _twins[key]


def _panel(ctx, snps, layout, monkeypatch):
    """the normal upload path; packed panels are split (main part + ragged tail) wherever that saves memory, SNPM_PACKED_SPLIT=0
    keeps whole rows"""
    if layout == "packed":
        monkeypatch.setenv("SNPM_PACKED_SPLIT", "0")
    panel = engine.Panel.from_host(ctx, snps, packed=layout != "int8")
    monkeypatch.delenv("SNPM_PACKED_SPLIT", raising=False)
    return panel


def same_bits(a, b):
    nan = np.isnan(b)
    return a.dtype == np.float64 and a.shape == b.shape and np.array_equal(np.isnan(a), nan) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def _check(got, want):
    for g, w, name in zip(got, want, ("acc_counts", "pair_counts")):
        assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), "%d cells of %s differ" % (int((g != w).sum()), name)
    assert same_bits(snp_genotype.het_from_counts(got[0]), windows_twin.het(want[0]))
    assert same_bits(snp_genotype.mismatch_from_counts(got[1]), windows_twin.mismatch(want[1]))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n_acc", [1, 33, 65, 1135])
def test_shape_grid(n_acc, layout, ctx, monkeypatch):
    other = layout == "int8"
    panel = _panel(ctx, calls_of(n_acc, other), layout, monkeypatch)
    if layout == "split" and n_acc == 1135:
        assert panel.pitch == 256 + 32      # main part + tail: the split layout exists at this width
    if layout == "packed":
        assert panel.pitch % 256 == 0       # whole rows
    for table in (EDGES, ONE):
        _check(engine.window_counts(panel, table, None, pairs_of(n_acc)), twin_of(n_acc, other, table))
    panel.free()


def test_selections_each_output_alone_and_refusals_that_need_a_panel(ctx, monkeypatch):
    snps = calls_of(1135, True)
    panel = _panel(ctx, snps, "int8", monkeypatch)
    rng = np.random.default_rng(6100)
    rows = np.concatenate([np.arange(1500, 300, -1), [7, 7, 2199, 0]]).astype(np.int64)       # descending, with a repeat
    cols = rng.permutation(1135)[:700]
    cols[-1] = cols[0]                      # a column subset with a repeat
    pairs = np.array([(5, 5), (5, 600), (600, 5), (699, 0), (1, 2)])
    table = np.array([0, 0, 1, 64, 65, 65, 700, 1203, len(rows), len(rows)])
    want = windows_twin.window_counts(snps, table, cols, pairs, rows)
    _check(engine.window_counts(panel, table, cols, pairs, rows), want)
    assert np.array_equal(want[0][:, -1], want[0][:, 0]) and np.array_equal(want[1][3, :, 0], want[1][3, :, 1])      # the repeated column; paired with itself
    only_a, none_p = engine.window_counts(panel, table, cols, None, rows)
    none_a, only_p = engine.window_counts(panel, table, cols, pairs, rows, acc_counts=False)
    assert none_p is None and none_a is None and np.array_equal(only_a, want[0]) and np.array_equal(only_p, want[1])
    _check(engine.window_counts(panel, [0, 3, 10], np.array([5]), [(0, 0)], range(2190, 2200)), windows_twin.window_counts(snps, [0, 3, 10], [5], [(0, 0)], range(2190, 2200)))
    acc, pair = engine.window_counts(panel, [0], None, pairs, range(10, 10))                       # n_win == 0
    assert acc.shape == (0, 1135, 4) and pair.shape == (5, 0, 4)
    acc, pair = engine.window_counts(panel, [0, 0, 0], None, pairs, range(10, 10))                 # windows, no row: zeros
    assert acc.shape == (2, 1135, 4) and not acc.any() and not pair.any()
    with pytest.raises(AssertionError, match="accession index outside the panel"):
        engine.window_counts(panel, ONE, [0, 1135])
    with pytest.raises(AssertionError, match="pair index outside the column list"):
        engine.window_counts(panel, ONE, [0, 1, 2], [(0, 3)])
    with pytest.raises(AssertionError, match="row index outside the panel"):
        engine.window_counts(panel, [0, 2], None, None, np.array([0, 2200], dtype=np.int64))
    with pytest.raises(AssertionError, match="row range outside the panel"):
        engine.window_counts(panel, [0, 2], None, None, range(2199, 2201))
    with pytest.raises(AssertionError, match="win_off must end at n"):
        engine.window_counts(panel, [0, 5], None, None, range(0, 6))
    panel.free()


def test_slabs_of_a_small_workspace_in_a_fresh_process(tmp_path):
    """SNPM_WIN_WS_MB=1 is read when a context is created: a child process.  1135 accessions are 1152 padded columns, 576 KiB of
    planes per step of 1024 rows: the budget holds one step, 2200 rows are three slabs; one window spans all of them, the others
    cross each slab edge; as a range and as a row list.  The results must be those of the one-slab run: the twin's."""
    n_acc = 1135
    table = np.array([0, 900, 1100, 2000, 2100, N_ROWS], dtype=np.int64)
    plan = engine.window_slabs(1 << 20, n_acc, n_acc + 5, table, N_ROWS)
    assert [p[:2] for p in plan] == [(0, 1), (1024, 1), (2048, 1)] and len(engine.window_slabs(256 << 20, n_acc, n_acc + 5, table, N_ROWS)) == 1
    snps = calls_of(n_acc, False)
    rows = np.random.default_rng(6200).integers(0, N_ROWS, size=N_ROWS).astype(np.int64)
    pairs = pairs_of(n_acc)
    for name, off in (("crossing", table), ("spanning", ONE)):
        np.savez(tmp_path / "in.npz", snps=snps, rows=rows, win_off=off, pairs=pairs)
        env = dict(os.environ, SNPM_WIN_WS_MB="1")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "win_slab_worker.py"), str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                           capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        z = np.load(tmp_path / "out.npz")
        assert z["launches"].tolist() == [3, 3, 3, 3], name         # planes and count kernels of the two calls: one launch each per slab
        _check((z["acc_range"], z["pair_range"]), windows_twin.window_counts(snps, off, None, pairs))
        _check((z["acc_list"], z["pair_list"]), windows_twin.window_counts(snps, off, None, pairs, rows))


def test_cross_checks_against_site_counts_and_kinship_counts(ctx, monkeypatch):
    """the same selection through three kernel families: the column counts summed over the windows are the site counts of one-column
    groups summed over the rows; hom_same / hom_diff summed over the windows are kinship's same / diff"""
    snps = calls_of(65, True)
    panel = _panel(ctx, snps, "int8", monkeypatch)
    cols = np.array([64, 3, 17, 40, 3, 0, 22, 63])
    rows = np.concatenate([np.arange(2100, 90, -3), [5, 5]]).astype(np.int64)
    table = np.array([0, 10, 10, 77, 400, len(rows)])
    pairs = np.array([(a, b) for a in range(len(cols)) for b in range(len(cols))])
    acc, pair = engine.window_counts(panel, table, cols, pairs, rows)
    site = engine.site_counts(panel, [np.array([c]) for c in cols], rows)
    assert np.array_equal(acc.sum(axis=0), site.sum(axis=1))
    ninfo, same, diff = engine.kinship_counts(panel, cols, rows)
    assert np.array_equal(pair[:, :, 2].sum(axis=1).reshape(len(cols), len(cols)), same) and np.array_equal(pair[:, :, 3].sum(axis=1).reshape(len(cols), len(cols)), diff)
    assert (pair[:, :, 0].sum(axis=1).reshape(len(cols), len(cols)) <= ninfo).all() and same.any() and diff.any()
    panel.free()


def test_the_genotype_methods_on_the_device_against_a_golden_of_the_reference(ctx, golden_dir):
    case = np.load(os.path.join(golden_dir, "windows_a7_w100.npz"))
    snps = case["snps"]
    g = snp_genotype.Genotype.from_arrays(snps, ["A%d" % i for i in range(7)], case["positions"], ["Chr1", "Chr2"], case["chr_regions"])
    assert not g.panel(ctx, packed=False).packed                    # (code 3 is in the golden)
    toy = genomes.Genome(os.path.join(golden_dir, "windows_toy_genome.json"))
    frame = g.calculate_heterozygosity_windows(toy, 100)
    assert list(frame.index) == case["index"].tolist() and same_bits(frame.to_numpy(), case["het"])
    assert same_bits(g.calculate_heterozygosity_windows(toy, 100, case["listed"]).to_numpy(), case["het_listed"])
    for i, (x, y) in enumerate(case["pairs"].tolist()):
        frame = g.mismatch_between_accs(x, y, 100, toy)
        assert list(frame["start"]) == case["start"].tolist() and same_bits(frame["mismatch"].to_numpy(dtype=np.float64), case["mismatch"][i])
        assert same_bits(g.mismatch_between_accs(x, y), case["mismatch_rows"][i])
    g.panel().free()
