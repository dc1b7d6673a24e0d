"""Panel LD on the device: ``snpm_panel_ld_band`` / ``k_ld_planes`` + ``k_ld_band`` against the numpy twin (tests/ld_twin.py), cell by
cell -- counts equal as integers, r2 equal as fp64 bits, ``nan`` where the twin has ``nan`` -- on panels filled through the normal
upload path in each of the three layouts, at the smallest shapes where each mechanism could break: 32 columns per word, a column
chunk of 24 words (768 columns), 64 rows per tile, 64 offsets per block of the band, slabs of the row axis with the halo behind
them; the selections, the output modes, ``Genotype.calculate_ld`` and one golden of the reference."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ld_twin
from snpmatch_amd import engine
from snpmatch_amd.core import snp_genotype

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = ["int8", "packed", "split"]
N_ROWS = 200
_panels, _twins = {}, {}


@pytest.fixture(scope="module")
def ctx():
    return engine.default_context()


def calls_of(n_acc, other):
    """the calls of the shape grid, made once per width: -1 / 0 / 1 / 2, int8 panels also 3, with a monomorphic row and one without a call"""
    if (n_acc, other) not in _panels:
        rng = np.random.default_rng(5000 + n_acc)
        v = rng.choice(np.array([-1, 0, 1, 2], dtype=np.int8), size=(N_ROWS, n_acc), p=[0.12, 0.45, 0.35, 0.08])
        if other:
            v[rng.random(v.shape) < 0.05] = 3
        v[3], v[4] = 0, -1
        _panels[(n_acc, other)] = v
    return _panels[(n_acc, other)]


def twin_of(n_acc, other, n_rows, band):
    """the twin's (counts, r2) of rows 0 .. n_rows - 1, computed once and shared by the layouts; never written to"""
    key = (n_acc, other, n_rows, band)
    if key not in _twins:
        _twins[key] = ld_twin.ld_band(calls_of(n_acc, other), band, None, range(0, n_rows))
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
    assert got[0].dtype == np.int32 and got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), "%d counts differ" % int((got[0] != want[0]).sum())
    assert same_bits(got[1], want[1]) and (got[1][~np.isnan(got[1])] <= 1.0).all()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n_acc", [1, 33, 65, 1135, 800])
def test_shape_grid(n_acc, layout, ctx, monkeypatch):
    """rows 1 / 65 / 200 x band 1 / 64 / 65 (a tile and one row; one block of offsets and one offset more); 800 accessions: 25 words,
    one more than a column chunk"""
    other = layout == "int8"
    panel = _panel(ctx, calls_of(n_acc, other), layout, monkeypatch)
    if layout == "split" and n_acc == 1135:
        assert panel.pitch == 256 + 32      # main part + tail: the split layout exists at this width
    if layout == "packed":
        assert panel.pitch % 256 == 0       # whole rows
    for n_rows in (1, 65, N_ROWS):
        for band in (1, 64, 65):
            _check(engine.ld_band(panel, band, None, range(0, n_rows)), twin_of(n_acc, other, n_rows, band))
    panel.free()


def test_selections_output_modes_and_refusals_that_need_a_panel(ctx, monkeypatch):
    snps = calls_of(1135, True)
    panel = _panel(ctx, snps, "int8", monkeypatch)
    rng = np.random.default_rng(5100)
    rows = np.concatenate([np.arange(150, 60, -1), [7, 7, 199, 0]]).astype(np.int64)       # descending, with a repeat
    cols = rng.permutation(1135)[:700]
    want = ld_twin.ld_band(snps, 9, cols, rows, 1, 3, 5)
    _check(engine.ld_band(panel, 9, cols, rows, 1, 3, 5), want)
    only_c, none_r = engine.ld_band(panel, 9, cols, rows, 1, 3, 5, r2=False)
    none_c, only_r = engine.ld_band(panel, 9, cols, rows, 1, 3, 5, counts=False)
    assert none_r is None and none_c is None and np.array_equal(only_c, want[0]) and same_bits(only_r, want[1])
    _check(engine.ld_band(panel, 3, np.array([5]), range(190, 200)), ld_twin.ld_band(snps, 3, [5], range(190, 200)))
    assert engine.ld_band(panel, 4, None, range(10, 10))[1].shape == (0, 4)
    with pytest.raises(AssertionError, match="accession index outside the panel"):
        engine.ld_band(panel, 2, [0, 1135])
    with pytest.raises(AssertionError, match="an accession is listed twice"):
        engine.ld_band(panel, 2, [4, 9, 4])
    with pytest.raises(AssertionError, match="row index outside the panel"):
        engine.ld_band(panel, 2, None, np.array([0, 200], dtype=np.int64))
    with pytest.raises(AssertionError, match="row range outside the panel"):
        engine.ld_band(panel, 2, None, range(199, 201))
    panel.free()
    wide = engine.Panel.from_host(ctx, np.zeros((2, 16385), dtype=np.int8), packed=False)
    with pytest.raises(AssertionError, match="wider than 16384 accessions"):
        engine.ld_band(wide, 1)
    wide.free()


def test_slabs_of_a_small_workspace_in_a_fresh_process(tmp_path):
    """SNPM_LD_WS_MB=1 is read when a context is created: a child process.  1135 accessions at band 300 leave 64 rows per slab:
    200 rows are four slabs, the halo crosses every edge and the last slab (8 rows) is shorter than the band; as a range and as
    a row list"""
    n_acc, band = 1135, 300
    slab_rows = engine.ld_slab_rows(1 << 20, n_acc, band, N_ROWS)
    slabs = -(-N_ROWS // slab_rows)
    assert slab_rows == 64 and slabs == 4 >= 3
    snps = calls_of(n_acc, False)
    rows = np.random.default_rng(5200).integers(0, N_ROWS, size=N_ROWS).astype(np.int64)
    np.savez(tmp_path / "in.npz", snps=snps, rows=rows, band=band)
    env = dict(os.environ, SNPM_LD_WS_MB="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ld_slab_worker.py"), str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    z = np.load(tmp_path / "out.npz")
    assert z["launches"].tolist() == [slabs, slabs, slabs, slabs]    # planes and band kernels of the two calls: one launch each per slab
    _check((z["counts_range"], z["r2_range"]), ld_twin.ld_band(snps, band))
    _check((z["counts_list"], z["r2_list"]), ld_twin.ld_band(snps, band, None, rows))


def test_calculate_ld_of_a_genotype_is_the_dense_twin_matrix(ctx):
    rng = np.random.default_rng(5300)
    snps = calls_of(65, False)
    g = snp_genotype.Genotype.from_arrays(snps, ["A%d" % i for i in range(65)], np.arange(1, N_ROWS + 1), ["Chr1"], [[0, N_ROWS]])
    assert g.panel(ctx, packed=True).packed
    rows, accs = rng.permutation(N_ROWS)[:40], rng.permutation(65)[:50]
    rows[:3] = [3, 4, rows[5]]              # monomorphic, no call, a repeat
    got = g.calculate_ld(rows, accs)
    assert same_bits(got, ld_twin.dense(snps, rows, accs)) and got[2, 5] == got[5, 5] == 1.0 and np.isnan(got[0]).all() and np.isnan(got[1]).all()
    g.panel().free()


def test_a_golden_of_the_reference_on_the_device(ctx, golden_dir, monkeypatch):
    """the reference takes the codes as numbers (alt 1, het 2); its dense fp64 form lies within 1e-12 of the exact integers (measured
    by the generator: 6.9e-15 at this width), ``nan`` in the same places"""
    case = np.load(os.path.join(golden_dir, "ld_a130_r200.npz"))
    snps, n = case["snps"], 200
    ref = np.full((n, n), np.nan)
    ref[np.triu_indices(n)] = case["r2_upper"]
    panel = _panel(ctx, snps, "split", monkeypatch)
    r2 = engine.ld_band(panel, n - 1, v_alt=1, v_het=2, min_n=1, counts=False)[1]
    panel.free()
    for d in range(1, n):
        got, want = r2[:n - d, d - 1], ref[np.arange(n - d), np.arange(d, n)]
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan) and (not (~nan).any() or np.abs(got[~nan] - want[~nan]).max() <= 1e-12)
        assert np.isnan(r2[n - d:, d - 1]).all()
    assert same_bits(r2, ld_twin.ld_band(snps, n - 1, None, None, 1, 2, 1)[1])
