"""mosaic on the device: ``snpm_panel_mosaic`` / ``k_win_planes`` + ``k_mos_fwd`` + ``k_mos_back`` against the numpy twin
(tests/mosaic_twin.py), cell by cell -- state, chain_cost and col_cost, without a tolerance -- on panels filled through the normal
upload path in each of the three layouts (int8, packed whole rows, packed split rows), at the shapes where the decomposition could
break: the widths of the four forms of the forward kernel (64 columns: one wave; 256: four waves of one column; 1280: four waves of
five columns; above: sixteen waves of twelve), 64 rows per word with chain boundaries anywhere inside it, 1024 rows per plane step,
slabs of whole chains and groups of samples under a small workspace budget; and ``core.mosaic`` end to end on the planted sample."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mosaic_twin as twin
from snpmatch_amd import engine
from snpmatch_amd.core import mosaic, snp_genotype

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = ["int8", "packed", "split"]
NONE = 0xFF
S_MAX = 1 << 20


@pytest.fixture(scope="module")
def ctx():
    return engine.default_context()


def _calls(rng, n_rows, n_acc, other=False):
    v = rng.choice(np.array([-1, 0, 1, 2], dtype=np.int8), size=(n_rows, n_acc), p=[0.12, 0.45, 0.35, 0.08])
    if other:
        v[rng.random((n_rows, n_acc)) < 0.05] = 3
    return v


def _classes(rng, snps, n_samples, rows=None, cols=None):
    """samples that copy a column in stretches with a tenth of their calls redrawn and a twentieth without a class: paths switch"""
    sel = twin.select(snps, cols, rows)
    n, ncols = sel.shape
    out = np.zeros((n_samples, n), dtype=np.uint8)
    for s in range(n_samples):
        src = np.repeat(rng.integers(0, ncols, size=n // 25 + 1), 25)[:n]
        v = sel[np.arange(n), src]
        redraw = (v < 0) | (v > 2) | (rng.random(n) < 0.1)
        out[s] = np.where(redraw, rng.integers(0, 3, size=n), v)
        out[s][rng.random(n) < 0.05] = NONE
    return out


def _panel(ctx, snps, layout, monkeypatch):
    """the normal upload path; packed panels are split (main part + ragged tail) wherever that saves memory, SNPM_PACKED_SPLIT=0
    keeps whole rows"""
    if layout == "packed":
        monkeypatch.setenv("SNPM_PACKED_SPLIT", "0")
    panel = engine.Panel.from_host(ctx, snps, packed=layout != "int8")
    monkeypatch.delenv("SNPM_PACKED_SPLIT", raising=False)
    return panel


def _table(rng, kind):
    if kind == 0:
        return mosaic.cost_table()                      # two cost planes
    t = rng.integers(0, 16, size=(3, 4)).astype(np.uint8)
    t[0, 1] = 0                                         # a zero off the diagonal
    t[2, 3] = 9
    return t


def _cut(n, at):
    return np.array(sorted([0] + [max(0, min(c, n)) for c in at] + [n]), dtype=np.int64)


def _check(panel, snps, classes, chain_off, cost, S, cols=None, rows=None, packed=False):
    got = engine.mosaic(panel, classes, chain_off, cost, S, cols, rows, want_col_cost=True)
    want = twin.mosaic(snps, classes, chain_off, cost, S, cols, None if rows is None else (np.arange(rows.start, rows.stop) if isinstance(rows, range) else rows), packed)
    for g, w, name in zip(got, want, ("state", "chain_cost", "col_cost")):
        assert g.dtype == np.int32 and g.shape == w.shape, name
        assert np.array_equal(g, w), "%s differs in %d cells" % (name, int((g != w).sum()))
    # without col_cost: the same path
    state, chain_cost, none = engine.mosaic(panel, classes, chain_off, cost, S, cols, rows)
    assert none is None and np.array_equal(state, want[0]) and np.array_equal(chain_cost, want[1])
    return got


WIDTHS = [1, 2, 63, 64, 65, 130, 255, 256, 257, 1279, 1280, 1281]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n_acc", WIDTHS)
def test_width_edges_of_every_form(n_acc, layout, ctx, monkeypatch):
    """one below, at and above the width of each form; 1281 columns force the widest form"""
    k = WIDTHS.index(n_acc)
    rng = np.random.default_rng(1000 + n_acc)
    snps = _calls(rng, 135, n_acc, other=layout == "int8")
    assert layout != "int8" or n_acc < 2 or (snps == 3).any()
    panel = _panel(ctx, snps, layout, monkeypatch)
    rows = range(3, 133)
    classes = _classes(rng, snps, 2, np.arange(3, 133))
    _check(panel, snps, classes, _cut(130, [64, 65]), _table(rng, k % 2), (1, 7, S_MAX)[k % 3], None, rows, layout != "int8")
    _check(panel, snps, classes[:1], _cut(130, []), _table(rng, (k + 1) % 2), (7, S_MAX, 1)[k % 3], None, rows, layout != "int8")
    panel.free()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n_rows", [1, 2, 63, 64, 65, 1023, 1024, 1025])
def test_row_edges_of_words_and_plane_steps(n_rows, layout, ctx, monkeypatch):
    rng = np.random.default_rng(2000 + n_rows)
    snps = _calls(rng, n_rows, 66, other=layout == "int8")
    panel = _panel(ctx, snps, layout, monkeypatch)
    classes = _classes(rng, snps, 2)
    _check(panel, snps, classes, _cut(n_rows, []), _table(rng, 0), 7, packed=layout != "int8")
    _check(panel, snps, classes, _cut(n_rows, [1, 63, 64, 65, n_rows - 1]), _table(rng, 1), 1, packed=layout != "int8")
    panel.free()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_chain_boundaries_inside_a_word_empty_chains_and_chains_of_one_row(layout, ctx, monkeypatch):
    rng = np.random.default_rng(3000)
    snps = _calls(rng, 200, 9, other=layout == "int8")
    panel = _panel(ctx, snps, layout, monkeypatch)
    classes = _classes(rng, snps, 2)
    packed = layout != "int8"
    _check(panel, snps, classes, _cut(200, [70, 71, 75, 100]), _table(rng, 0), 2, packed=packed)                      # several boundaries in word 1, a chain of one row
    _check(panel, snps, classes, _cut(200, [0, 0, 90, 90, 90, 200, 200]), _table(rng, 1), 7, packed=packed)          # empty chains first, in the middle, last
    _check(panel, snps, classes[:, :130], np.arange(131), _table(rng, 0), 1, rows=range(0, 130), packed=packed)      # every row its own chain
    # no rows: zero costs, nothing launched; no chains either
    state, chain_cost, col_cost = engine.mosaic(panel, np.zeros((2, 0), dtype=np.uint8), [0, 0, 0], _table(rng, 0), 5, rows=range(0, 0), want_col_cost=True)
    assert state.shape == (2, 0) and not chain_cost.any() and chain_cost.shape == (2, 2) and not col_cost.any() and col_cost.shape == (2, 2, 9)
    panel.free()


@pytest.mark.parametrize("n_samples", [1, 2, 65])
def test_samples(n_samples, ctx, monkeypatch):
    rng = np.random.default_rng(4000 + n_samples)
    snps = _calls(rng, 150, 70, other=True)
    panel = _panel(ctx, snps, "int8", monkeypatch)
    _check(panel, snps, _classes(rng, snps, n_samples), _cut(150, [10, 64, 100]), _table(rng, n_samples % 2), 7)
    panel.free()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_column_and_row_lists(layout, ctx, monkeypatch):
    """cols shuffled with repeats (two states of one column: the tie rules decide), row_idx unsorted with repeats, a dense range
    with row0 > 0"""
    rng = np.random.default_rng(5000)
    snps = _calls(rng, 400, 130, other=layout == "int8")
    panel = _panel(ctx, snps, layout, monkeypatch)
    packed = layout != "int8"
    cols = rng.permutation(np.concatenate([np.arange(130), [5, 5, 77, 129]])).astype(np.int32)
    rows = rng.integers(0, 400, size=300).astype(np.int64)
    rows[-1] = rows[0]
    for S in (1, 7, S_MAX):
        _check(panel, snps, _classes(rng, snps, 2, rows, cols), _cut(300, [63, 150]), _table(rng, S % 2), S, cols, rows, packed)
    _check(panel, snps, _classes(rng, snps, 1, np.arange(37, 337), cols), _cut(300, [200]), _table(rng, 1), 7, cols, range(37, 337), packed)
    # a sample that IS a column listed twice: no cost, and the lower position is the state
    twice = np.array([9, 4, 9], dtype=np.int32)
    sel = twin.select(snps, twice, np.arange(400), packed)
    cls = np.where((sel[:, 0] >= 0) & (sel[:, 0] <= 2), sel[:, 0], NONE).astype(np.uint8)
    state, chain_cost, _ = _check(panel, snps, cls[None, :], _cut(400, [100]), mosaic.cost_table(), 3, twice, None, packed)
    assert not state.any() and not chain_cost.any()
    panel.free()


def test_never_switching_at_the_largest_switch_cost(ctx, monkeypatch):
    """S = 2^20 and chains of at most 500 rows (15 * 500 < S): chain_cost == min over the columns of col_cost"""
    rng = np.random.default_rng(6000)
    snps = _calls(rng, 1200, 260, other=True)
    panel = _panel(ctx, snps, "int8", monkeypatch)
    off = _cut(1200, [500, 700, 1199])
    state, chain_cost, col_cost = _check(panel, snps, _classes(rng, snps, 3), off, _table(rng, 1), S_MAX)
    assert np.array_equal(chain_cost, col_cost.min(axis=2)) and chain_cost[:, :3].all()       # (the chain of one row may cost nothing)
    for c in range(len(off) - 1):
        assert np.array_equal(state[:, off[c]:off[c + 1]], np.repeat(col_cost[:, c].argmin(axis=1)[:, None], off[c + 1] - off[c], axis=1))
    panel.free()


def test_the_most_columns_of_one_call(ctx, monkeypatch):
    """SNPM_MOS_MAX_ACCESSIONS states: a 300-accession panel listed 12288 times over, shuffled"""
    rng = np.random.default_rng(7000)
    snps = _calls(rng, 70, 300)
    panel = _panel(ctx, snps, "split", monkeypatch)
    cols = rng.permutation(np.arange(engine.MOS_MAX_ACCESSIONS) % 300).astype(np.int32)
    _check(panel, snps, _classes(rng, snps, 1, None, cols), _cut(70, [64]), _table(rng, 1), 7, cols, None, True)
    with pytest.raises(AssertionError, match="SNPM_MOS_MAX_ACCESSIONS"):
        engine.mosaic(panel, np.zeros((1, 70), dtype=np.uint8), [0, 70], mosaic.cost_table(), 7, np.zeros(engine.MOS_MAX_ACCESSIONS + 1, dtype=np.int32))
    with pytest.raises(AssertionError, match="accession index outside the panel"):
        engine.mosaic(panel, np.zeros((1, 70), dtype=np.uint8), [0, 70], mosaic.cost_table(), 7, np.array([0, 300], dtype=np.int32))
    with pytest.raises(AssertionError, match="row index outside the panel"):
        engine.mosaic(panel, np.zeros((1, 2), dtype=np.uint8), [0, 2], mosaic.cost_table(), 7, None, np.array([0, 70]))
    panel.free()


def test_small_workspace_budget_gives_the_same_results(tmp_path):
    """A fresh process under SNPM_MOS_WS_MB=1: 130 columns (192 padded) x 9000 rows in 5 chains, 3 samples.  The planes of 1024 rows
    take 96 KiB: the chain of 8300 rows (864 KiB of planes and 263 KiB of sw words, j, states and class words per sample) is larger
    than the budget and a slab of its own, with the samples one at a time; the two chains before it and the two after it are a slab
    each, with the three samples in one group."""
    rng = np.random.default_rng(8000)
    snps = _calls(rng, 9100, 130)
    rows = rng.permutation(9100)[:9000].astype(np.int64)
    chain_off = np.array([0, 200, 400, 8700, 8850, 9000], dtype=np.int64)
    classes = _classes(rng, snps, 3, rows)
    cost = mosaic.cost_table()
    np.savez(tmp_path / "in.npz", snps=snps, rows=rows, classes=classes, chain_off=chain_off, cost=cost, S=7)
    env = dict(os.environ, SNPM_MOS_WS_MB="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mos_slab_worker.py"), str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    z = np.load(tmp_path / "out.npz")
    assert z["launches"].tolist() == [3, 5, 5]                  # three slabs; the samples in one group, one at a time, in one group
    want = twin.mosaic(snps, classes, chain_off, cost, 7, None, rows, True)
    assert np.array_equal(z["state"], want[0]) and np.array_equal(z["chain_cost"], want[1]) and np.array_equal(z["col_cost"], want[2])
    # the default budget in this process: one slab, one group
    ctx = engine.default_context()
    panel = engine.Panel.from_host(ctx, snps, packed=True)
    ctx.profile(True)
    ctx.profile_reset()
    got = engine.mosaic(panel, classes, chain_off, cost, 7, None, rows, want_col_cost=True)
    assert [ctx.profile_read(k)[0] for k in ("win_planes", "mos_fwd", "mos_back")] == [1, 1, 1]
    ctx.profile(False)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    panel.free()


def test_mosaic_end_to_end_on_the_planted_sample(ctx, tmp_path):
    p = twin.planted()
    g = snp_genotype.Genotype.from_arrays(p["snps"], p["accessions"], p["positions"], p["chrs"], p["chr_regions"])
    g.panel(ctx)
    # two samples on the shared records: the planted one, and the same with every third record uncalled
    gt = np.stack([p["s_gt"], np.where(np.arange(2700) % 3 == 0, "./.", p["s_gt"])], axis=1)
    painted = mosaic.Mosaic(["planted", "thinned"], p["s_chr"], p["s_pos"], gt, g, str(tmp_path / "out"), twin.PLANTED_S, twin.PLANTED_MISMATCH, twin.PLANTED_HET)
    assert np.array_equal(painted.db_rows, p["rows"]) and np.array_equal(painted.chain_off, p["chain_off"])
    assert np.array_equal(painted.classes[0], p["classes"]) and (painted.classes[1][::3] == NONE).all() and np.array_equal(painted.classes[1][1::3], p["classes"][1::3])
    want = twin.mosaic(p["snps"], painted.classes, p["chain_off"], painted.cost, twin.PLANTED_S, None, p["rows"], True)
    assert np.array_equal(painted.state, want[0]) and np.array_equal(painted.chain_cost, want[1]) and np.array_equal(painted.col_cost, want[2])
    assert twin.plan_recovered(painted.segs[0]) and twin.plan_recovered(painted.segs[1], 2 * twin.PLANTED_TOL)
    e = twin.emissions(twin.select(p["snps"], rows=p["rows"]), p["classes"], painted.cost)
    assert painted.seg_costs[0].tolist() == [int(e[k0:k1 + 1, a].sum()) for _, k0, k1, a in painted.segs[0].tolist()]
    s = painted.stats["samples"]["planted"]
    assert s["switches"] == 4 and s["total_cost"] == int(want[1][0].sum()) == int(painted.seg_costs[0].sum()) + 4 * twin.PLANTED_S
    assert all(os.path.exists(str(tmp_path / "out") + ext) for ext in (".mosaic.json", ".mosaic.npz", ".mosaic.segments.tsv"))
    g.panel().free()
