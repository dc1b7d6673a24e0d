"""parentsearch on the device: ``snpm_panel_parent_counts`` / ``k_win_planes`` + ``k_par_count`` against the numpy twin
(tests/parentsearch_twin.py), cell by cell, all four matrices and without a tolerance, on panels filled through the normal upload path
in each of the three layouts (int8, packed whole rows, packed split rows), at the shapes where the decomposition could break: 32
accessions per tile side of the count kernel, 64 rows per word with window boundaries anywhere inside it, 1024 rows per LDS step,
groups of whole windows of about 8192 rows, slabs of whole windows; and ``ParentSearch`` end to end on the planted F2."""
import os
import re

import numpy as np
import pytest

import parentsearch_twin as twin
from snpmatch_amd import engine
from snpmatch_amd.core import parentsearch, parsers, snp_genotype

pytestmark = pytest.mark.gpu

LAYOUTS = ["int8", "packed", "split"]
NONE = 0xFF


def _kernel_constant(name):
    """a ``constexpr int`` of csrc/snpm_k_f1x.hpp (the tiling k_par_count keeps)"""
    text = open(os.path.join(os.path.dirname(os.path.abspath(engine.__file__)), "csrc", "snpm_k_f1x.hpp")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


CHUNK = _kernel_constant("F1X_CHUNK_WORDS") * 64          # rows a group of windows aims at
STEP = _kernel_constant("F1X_STEP_WORDS") * 64            # rows per LDS step


@pytest.fixture(scope="module")
def ctx():
    return engine.default_context()


def _calls(rng, n_rows, n_acc, other=False):
    v = rng.choice(np.array([-1, 0, 1, 2], dtype=np.int8), size=(n_rows, n_acc), p=[0.12, 0.45, 0.35, 0.08])
    if other:
        v[rng.random((n_rows, n_acc)) < 0.05] = 3
    return v


def _classes(rng, n):
    return rng.choice(np.array([0, 1, 2, NONE], dtype=np.uint8), size=n, p=[0.4, 0.3, 0.22, 0.08])


def _panel(ctx, snps, layout, monkeypatch):
    """the normal upload path; packed panels are split (main part + ragged tail) wherever that saves memory, SNPM_PACKED_SPLIT=0
    keeps whole rows"""
    if layout == "packed":
        monkeypatch.setenv("SNPM_PACKED_SPLIT", "0")
    panel = engine.Panel.from_host(ctx, snps, packed=layout != "int8")
    monkeypatch.delenv("SNPM_PACKED_SPLIT", raising=False)
    return panel


def _every(n, length):
    return np.append(np.arange(0, n, length), n).astype(np.int64)


def _window_sets(n):
    """one window; every row its own; boundaries at 63 | 64 | 65; empty windows first, in the middle and last"""
    cut = lambda at: np.array([0] + [min(c, n) for c in at] + [n], dtype=np.int64)      # noqa: E731
    return [np.array([0, n]), np.arange(n + 1), cut([63, 64, 65]), cut([0, 0, n // 2, n // 2, n, n])]


def _check(panel, snps, classes, win_off, min_sites=1, cols=None, rows=None):
    got = engine.parent_counts(panel, classes, win_off, min_sites, cols, rows)
    want = twin.parent_counts(snps, classes, win_off, min_sites, cols, None if rows is None else (np.arange(rows.start, rows.stop) if isinstance(rows, range) else rows))
    for g, w, name in zip(got, want, ("score", "n_tot", "w_first", "w_het")):
        assert g.dtype == np.int32 and g.shape == w.shape, name
        assert np.array_equal(g, w), "%s differs in %d cells" % (name, int((g != w).sum()))
    score, n_tot, w_first, w_het = got
    assert np.array_equal(score, score.T) and np.array_equal(n_tot, n_tot.T) and np.array_equal(w_het, w_het.T)
    assert not np.diag(w_het).any() and (score <= n_tot).all()
    return got


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n_acc", [1, 2, 31, 32, 33, 65, 130])
def test_tile_edges_of_accessions_and_window_boundaries_inside_words(n_acc, layout, ctx, monkeypatch):
    rng = np.random.default_rng(1000 + n_acc)
    snps = _calls(rng, 70, n_acc, other=layout == "int8")
    assert layout != "int8" or (snps == 3).any()
    panel = _panel(ctx, snps, layout, monkeypatch)
    for k, win_off in enumerate(_window_sets(70)):
        _check(panel, snps, _classes(rng, 70), win_off, 1 + k % 2)
    for n_rows in (1, 63, 64, 65):
        _check(panel, snps, _classes(rng, n_rows), _window_sets(n_rows)[n_rows % 4], 1, rows=range(5, 5 + n_rows))
    panel.free()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_groups_at_chunk_minus_one_exact_plus_one(layout, ctx, monkeypatch):
    """33 accessions at chunk - 1 / chunk / chunk + 1 rows, as one window (chunk + 1: a window longer than a chunk, a group of its own
    with one more step) and as windows of 100 rows (groups of 81 windows; the boundaries fall anywhere inside the words)"""
    rng = np.random.default_rng(2000)
    snps = _calls(rng, CHUNK + 1, 33, other=layout == "int8")
    classes = _classes(rng, CHUNK + 1)
    panel = _panel(ctx, snps, layout, monkeypatch)
    for n_rows in (CHUNK - 1, CHUNK, CHUNK + 1):
        _check(panel, snps, classes[:n_rows], np.array([0, n_rows]), 1, rows=range(0, n_rows))
        _check(panel, snps, classes[:n_rows], _every(n_rows, 100), 5, rows=range(0, n_rows))
    _check(panel, snps, classes[:STEP + 1], np.array([0, STEP - 1, STEP + 1]), 1, rows=range(1, STEP + 2))      # a window across an LDS step
    panel.free()


@pytest.mark.parametrize("layout", ["int8", "split"])
def test_three_slabs_of_whole_windows_equal_one_slab(layout, monkeypatch):
    """SNPM_PAR_WS_MB=1: 130 accessions are 192 padded columns, 96 KiB of planes per 1024 rows -- the budget holds 10 such steps.
    Three windows of 9000 rows (9 steps each) are three slabs; a slab is never cut inside a window.  Once as a range and once as a
    row list with repeats; the budget changes the launches, not the counts."""
    step_bytes = 4 * 192 * (STEP // 64) * 8
    assert (1 << 20) // step_bytes == 10
    win_off = np.array([0, 9000, 9000, 18000, 27000], dtype=np.int64)
    monkeypatch.setenv("SNPM_PAR_WS_MB", "1")
    small = engine.Context(0)
    try:
        rng = np.random.default_rng(3000)
        snps = _calls(rng, 27000, 130, other=layout == "int8")
        classes = _classes(rng, len(snps))
        panel = _panel(small, snps, layout, monkeypatch)
        small.profile(True)
        small.profile_reset()
        ranged = _check(panel, snps, classes, win_off, 5)
        assert small.profile_read("win_planes")[0] == 3 and small.profile_read("par_count")[0] == 3
        small.profile_reset()
        order = rng.integers(0, len(snps), size=27000).astype(np.int64)               # a row list crosses slabs too; with repeats
        order[-1] = order[0]
        _check(panel, snps, classes, win_off, 5, rows=order)
        assert small.profile_read("win_planes")[0] == 3 and small.profile_read("par_count")[0] == 3
        # a window larger than the budget is a slab of its own: the planes workspace grows to it
        small.profile_reset()
        wide = np.array([0, 500, 26000, 27000], dtype=np.int64)
        _check(panel, snps, classes, wide, 1)
        assert small.profile_read("win_planes")[0] == 3 and small.profile_read("par_count")[0] == 3
        small.profile(False)
        panel.free()
        # the same scan under the default budget: one slab, the same counts
        monkeypatch.delenv("SNPM_PAR_WS_MB")
        ctx = engine.default_context()
        whole = _panel(ctx, snps, layout, monkeypatch)
        ctx.profile(True)
        ctx.profile_reset()
        once = engine.parent_counts(whole, classes, win_off, 5)
        assert ctx.profile_read("par_count")[0] == 1 and ctx.profile_read("win_planes")[0] == 1
        ctx.profile(False)
        assert all(np.array_equal(a, b) for a, b in zip(ranged, once))
        whole.free()
    finally:
        small.close()


def test_min_win_sites_one_window_relations_and_the_w_first_identity(ctx, monkeypatch):
    rng = np.random.default_rng(5000)
    snps = _calls(rng, 1500, 70, other=True)
    snps[:, 7] = -1
    panel = _panel(ctx, snps, "int8", monkeypatch)
    cols = rng.permutation(70)[:41].astype(np.int32)
    cols[3] = cols[-1] = 11                                                             # a repeated column (not the blank one)
    rows = rng.integers(0, 1500, size=1100).astype(np.int64)                          # unsorted, with repeats
    classes = _classes(rng, 1100)
    win_off = np.sort(np.concatenate([[0, 1100], rng.integers(0, 1101, size=150)])).astype(np.int64)      # ~7 rows a window, some empty
    one = _check(panel, snps, classes, win_off, 1, cols, rows)
    five = _check(panel, snps, classes, win_off, 5, cols, rows)
    assert (five[1] <= one[1]).all() and (five[1] < one[1]).any() and (five[0] <= one[0]).all()
    # the number of used windows per pair, from the twin's raw counts of two cells
    for a, b in ((0, 1), (5, 40), (3, 40)):
        n = twin.pair_windows(snps, classes, win_off, a, b, cols, rows)[:, 0]
        for got, m in ((one, 1), (five, 5)):
            assert got[2][a, b] + got[2][b, a] + got[3][a, b] == (n >= m).sum()
            assert got[2][a, a] == (twin.pair_windows(snps, classes, win_off, a, a, cols, rows)[:, 0] >= m).sum()
    off_diag = ~np.eye(41, dtype=bool)
    used = one[2] + one[2].T + one[3]
    assert np.array_equal(used, used.T) and (used[off_diag] <= 150 + 1).all()
    assert one[2][3, 40] > 0 and one[2][40, 3] == 0                                    # the same column twice: every tie to the smaller position
    # one window and every class set: n_tot is f1_counts' ninfo, score the maximum of the three whole-genome counts
    full = rng.choice(np.array([0, 1, 2], dtype=np.uint8), size=1500)
    score, n_tot, w_first, w_het = _check(panel, snps, full, np.array([0, 1500]), 1)
    hits, ninfo = engine.f1_counts(panel, full)
    assert np.array_equal(n_tot, ninfo) and (score >= hits).all() and np.array_equal(score[w_het == 1], hits[w_het == 1])
    assert not n_tot[7].any() and not score[:, 7].any()
    assert np.array_equal((w_first + w_first.T + w_het)[~np.eye(70, dtype=bool)], (ninfo > 0).astype(np.int32)[~np.eye(70, dtype=bool)])
    with pytest.raises(AssertionError, match="win_off must end at n"):
        engine.parent_counts(panel, full, np.array([0, 1499]))
    with pytest.raises(AssertionError, match="min_win_sites must be 1 or more"):
        engine.parent_counts(panel, full, np.array([0, 1500]), 0)
    panel.free()


def test_split_layout_at_the_width_of_the_1001_genomes_panel_and_empty_calls(ctx, monkeypatch):
    rng = np.random.default_rng(7000)
    snps = _calls(rng, 3000, 1135)
    panel = _panel(ctx, snps, "split", monkeypatch)
    assert panel.pitch == 256 + 32                      # main part + tail: the split layout exists at this width
    win_off = np.sort(np.concatenate([[0, 3000], rng.integers(0, 3001, size=19)])).astype(np.int64)       # 20 windows
    _check(panel, snps, _classes(rng, 3000), win_off, 5)
    none8 = np.zeros(0, dtype=np.uint8)
    empty = engine.parent_counts(panel, none8, np.array([0, 0, 0]), 1, cols=np.array([1, 2, 3], dtype=np.int32), rows=range(0, 0))       # n_rows == 0: zeros
    assert len(empty) == 4 and all(m.shape == (3, 3) and m.dtype == np.int32 and not m.any() for m in empty)
    nothing = engine.parent_counts(panel, _classes(rng, 3000), win_off, 1, cols=np.zeros(0, dtype=np.int32))                      # ncols == 0: nothing
    assert all(m.shape == (0, 0) for m in nothing)
    blind = engine.parent_counts(panel, np.full(3000, NONE, dtype=np.uint8), win_off, 1, cols=np.arange(40, dtype=np.int32))     # no class: zeros
    assert all(not m.any() for m in blind)
    with pytest.raises(AssertionError, match="accession index outside the panel"):
        engine.parent_counts(panel, _classes(rng, 3000), win_off, 1, cols=np.array([0, 1135], dtype=np.int32))
    with pytest.raises(AssertionError, match="row index outside the panel"):
        engine.parent_counts(panel, _classes(rng, 2), np.array([0, 2]), 1, rows=np.array([0, 3000], dtype=np.int64))
    panel.free()


def _planted_inputs(case):
    inputs = parsers.ParseInputs("")
    inputs.load_snp_info(case["s_chr"], case["s_pos"], case["s_gt"], parsers.ParseInputs.get_wei_from_GT(case["s_gt"]), "NA")
    return inputs


def test_parentsearch_end_to_end_on_the_planted_panel(ctx, tmp_path):
    import json
    case = twin.planted_case()
    pa, pb = twin.PLANTED_PARENTS
    genome = str(tmp_path / "two_chromosomes.json")
    with open(genome, "w") as fh:
        json.dump(case["genome"], fh)
    g = snp_genotype.Genotype.from_arrays(case["snps"], case["names"], case["positions"], case["chrs"], case["chr_regions"])
    g.panel(ctx)
    search = parentsearch.ParentSearch(_planted_inputs(case), g, genome, twin.PLANTED_BIN, str(tmp_path / "out"), top=10, min_sites=100, min_win_sites=5)
    assert np.array_equal(search.db_rows, np.arange(3000)) and np.array_equal(search.classes, case["classes"]) and np.array_equal(search.win_off, case["win_off"])
    want = twin.parent_counts(case["snps"], case["classes"], case["win_off"], 5)
    for got, w in zip((search.score, search.n_tot, search.w_first, search.w_het), want):
        assert np.array_equal(got, w)
    assert search.pairs[0] == (pa, pb, 3000, 3000) and len(search.pairs) == 10
    singles = np.argsort(-search.result.probabilies[:40])[:10]
    assert pa not in singles and pb not in singles and search.stats["in_top10_route"] is False
    best = search.stats["best_pair"]
    assert (best["windows_A"], best["windows_B"], best["windows_AB"], best["windows_unused"]) == (3, 3, 6, 0)
    # the shortlist's tracks: the twin's raw counts, and the device's w_first / w_het of the same cells
    for (a, b, _, _), (counts, state) in zip(search.pairs, search.tracks):
        assert np.array_equal(counts, twin.pair_windows(case["snps"], case["classes"], case["win_off"], a, b))
        assert [(state == k).sum() for k in range(3)] == [search.w_first[a, b], search.w_first[b, a], search.w_het[a, b]]
    assert [parentsearch.STATES[s] for s in search.tracks[0][1]] == [{"AA": "A", "BB": "B", "AB": "AB"}[m] for m in twin.PLANTED_MOSAIC]
    assert all(os.path.exists(str(tmp_path / "out") + ext) for ext in (".parentsearch.json", ".parentsearch.npz", ".parentsearch.windows.tsv"))
    g.panel().free()
