"""f1search on the device: ``snpm_panel_f1_counts`` / ``k_win_planes`` + ``k_f1x_count`` against the numpy twin (tests/f1search_twin.py),
cell by cell and without a tolerance, on panels filled through the normal upload path in each of the three layouts (int8, packed
whole rows, packed split rows), at the shapes where the decomposition could break: 32 accessions per tile side of the count kernel
(a 2 x 2 register tile of pairs per lane; the plane kernel works on 64 accessions x 64 rows), 64 rows per word, 1024 rows per LDS
step, 8192 rows per chunk, slabs of the row axis; ``Genotype.f1_counts`` against the reference's goldens; and ``F1Search`` end to end
on the planted panel whose parents the ten-best route cannot find."""
import itertools
import os
import re

import numpy as np
import pytest

import f1search_twin
from snpmatch_amd import engine
from snpmatch_amd.core import f1search, parsers, snp_genotype

pytestmark = pytest.mark.gpu

LAYOUTS = ["int8", "packed", "split"]


def _kernel_constant(name):
    """a ``constexpr int`` of csrc/snpm_k_f1x.hpp"""
    text = open(os.path.join(os.path.dirname(os.path.abspath(engine.__file__)), "csrc", "snpm_k_f1x.hpp")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


CHUNK = _kernel_constant("F1X_CHUNK_WORDS") * 64          # rows per block of k_f1x_count
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
    return rng.choice(np.array([0, 1, 2, 0xFF], dtype=np.uint8), size=n, p=[0.4, 0.3, 0.22, 0.08])


def _panel(ctx, snps, layout, monkeypatch):
    """the normal upload path; packed panels are split (main part + ragged tail) wherever that saves memory, SNPM_PACKED_SPLIT=0
    keeps whole rows"""
    if layout == "packed":
        monkeypatch.setenv("SNPM_PACKED_SPLIT", "0")
    panel = engine.Panel.from_host(ctx, snps, packed=layout != "int8")
    monkeypatch.delenv("SNPM_PACKED_SPLIT", raising=False)
    return panel


def _check(panel, snps, classes, cols=None, rows=None):
    got = engine.f1_counts(panel, classes, cols, rows)
    want = f1search_twin.f1_counts(snps, classes, cols, None if rows is None else (np.arange(rows.start, rows.stop) if isinstance(rows, range) else rows))
    for g, w, name in zip(got, want, ("hits", "ninfo")):
        assert g.dtype == np.int32 and g.shape == w.shape, name
        assert np.array_equal(g, w), "%s differs in %d cells" % (name, int((g != w).sum()))
        assert np.array_equal(g, g.T), name
    return got


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n_acc", [1, 2, 31, 32, 33, 65, 130])
def test_tile_edges_of_accessions_and_words_of_rows(n_acc, layout, ctx, monkeypatch):
    rng = np.random.default_rng(1000 + n_acc)
    snps = _calls(rng, 70, n_acc, other=layout == "int8")
    assert layout != "int8" or (snps == 3).any()
    panel = _panel(ctx, snps, layout, monkeypatch)
    for n_rows in (1, 63, 64, 65):
        _check(panel, snps, _classes(rng, n_rows), rows=range(5, 5 + n_rows))
    _check(panel, snps, _classes(rng, 70))
    panel.free()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_chunk_of_the_count_kernel_minus_one_exact_plus_one(layout, ctx, monkeypatch):
    rng = np.random.default_rng(2000)
    snps = _calls(rng, CHUNK + 1, 33, other=layout == "int8")
    classes = _classes(rng, CHUNK + 1)
    panel = _panel(ctx, snps, layout, monkeypatch)
    for n_rows in (CHUNK - 1, CHUNK, CHUNK + 1, STEP + 1):
        _check(panel, snps, classes[:n_rows], rows=range(0, n_rows))
    _check(panel, snps, classes[:CHUNK], rows=range(1, CHUNK + 1))
    panel.free()


@pytest.mark.parametrize("layout", ["int8", "split"])
def test_three_slabs_with_a_ragged_last_one(layout, monkeypatch):
    """SNPM_F1X_WS_MB=1: 130 accessions are 192 padded columns, 96 KiB of planes per 1024 rows -- the budget holds 10 such steps,
    cut to one whole chunk of 8192 rows per slab.  Once as a range and once as a row list with repeats; the budget changes the
    launches, not the counts."""
    step_bytes = 4 * 192 * (STEP // 64) * 8
    steps = (1 << 20) // step_bytes
    assert steps >= CHUNK // STEP and steps // (CHUNK // STEP) * (CHUNK // STEP) * STEP == CHUNK
    monkeypatch.setenv("SNPM_F1X_WS_MB", "1")
    small = engine.Context(0)
    try:
        rng = np.random.default_rng(3000)
        snps = _calls(rng, 2 * CHUNK + 1030, 130, other=layout == "int8")
        classes = _classes(rng, len(snps))
        panel = _panel(small, snps, layout, monkeypatch)
        small.profile(True)
        small.profile_reset()
        ranged = _check(panel, snps, classes)
        assert small.profile_read("win_planes")[0] == 3 and small.profile_read("f1x_count")[0] == 3
        small.profile_reset()
        order = rng.integers(0, len(snps), size=2 * CHUNK + 5).astype(np.int64)       # a row list crosses slabs too; with repeats
        order[-1] = order[0]
        _check(panel, snps, classes[:len(order)], rows=order)
        assert small.profile_read("win_planes")[0] == 3 and small.profile_read("f1x_count")[0] == 3
        small.profile(False)
        panel.free()
        # the same scan under the default budget: one slab, the same counts
        monkeypatch.delenv("SNPM_F1X_WS_MB")
        ctx = engine.default_context()
        whole = _panel(ctx, snps, layout, monkeypatch)
        ctx.profile(True)
        ctx.profile_reset()
        once = engine.f1_counts(whole, classes)
        assert ctx.profile_read("f1x_count")[0] == 1
        ctx.profile(False)
        assert all(np.array_equal(a, b) for a, b in zip(ranged, once))
        whole.free()
    finally:
        small.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_column_subset_with_a_repeat_and_unsorted_rows_with_repeats(layout, ctx, monkeypatch):
    rng = np.random.default_rng(4000)
    snps = _calls(rng, 1500, 70, other=layout == "int8")
    panel = _panel(ctx, snps, layout, monkeypatch)
    cols = rng.permutation(70)[:41].astype(np.int32)
    cols[-1] = cols[3]
    rows = rng.integers(0, 1500, size=1100).astype(np.int64)                          # unsorted, with repeats
    classes = _classes(rng, 1100)
    hits, ninfo = _check(panel, snps, classes, cols=cols, rows=rows)
    assert np.array_equal(ninfo[-1], ninfo[3]) and np.array_equal(hits[-1], hits[3]) and ninfo[3, -1] == ninfo[3, 3]
    # a row list that is a dense range gives what row0 / n_rows gives
    dense = _check(panel, snps, classes, cols=cols, rows=range(200, 1300))
    listed = _check(panel, snps, classes, cols=cols, rows=np.arange(200, 1300, dtype=np.int64))
    assert all(np.array_equal(a, b) for a, b in zip(dense, listed))
    panel.free()


def test_diagonal_other_code_all_missing_column_and_ninfo_without_classes(ctx, monkeypatch):
    rng = np.random.default_rng(5000)
    snps = _calls(rng, 300, 40, other=True)
    snps[:, 7] = -1
    snps[:, 9] = 3                      # "other": informative against anything else, never against itself
    classes = _classes(rng, 300)
    panel = _panel(ctx, snps, "int8", monkeypatch)
    hits, ninfo = _check(panel, snps, classes)
    # the cross of a column with itself: informative where it is homozygous, a hit where that is the sample's class
    assert np.array_equal(np.diag(ninfo), ((snps == 0) | (snps == 1)).sum(axis=0))
    assert np.array_equal(np.diag(hits), ((snps == 0) & (classes == 0)[:, None]).sum(axis=0) + ((snps == 1) & (classes == 1)[:, None]).sum(axis=0))
    assert not ninfo[7].any() and not ninfo[:, 7].any() and ninfo[9, 9] == 0
    assert np.array_equal(np.delete(ninfo[9], 9), np.delete(((snps >= 0) & (snps != 3)).sum(axis=0), 9))
    assert np.array_equal(hits[9], ((snps >= 0) & (snps != 3) & (classes == 2)[:, None]).sum(axis=0))       # 3 against a call: het
    # rows without a class count in ninfo only: all classes 0xFF give the same ninfo and no hit
    blind = engine.f1_counts(panel, np.full(300, 0xFF, dtype=np.uint8))
    assert np.array_equal(blind[1], ninfo) and not blind[0].any()
    with pytest.raises(AssertionError, match="sample_class holds a byte other than 0, 1, 2 or 0xFF"):
        engine.f1_counts(panel, np.full(300, 3, dtype=np.uint8))
    panel.free()


def test_a_smaller_second_call_sees_nothing_of_the_first_and_empty_calls(ctx, monkeypatch):
    rng = np.random.default_rng(6000)
    snps = _calls(rng, 3000, 130, other=True)
    big = _panel(ctx, snps, "int8", monkeypatch)
    _check(big, snps, _classes(rng, 3000))
    tiny = _calls(rng, 9, 3)
    small = _panel(ctx, tiny, "split", monkeypatch)
    _check(small, tiny, _classes(rng, 9))
    _check(big, snps, _classes(rng, 1), cols=np.array([5, 6], dtype=np.int32), rows=range(0, 1))
    none8 = np.zeros(0, dtype=np.uint8)
    empty = engine.f1_counts(big, none8, cols=np.array([1, 2, 3], dtype=np.int32), rows=range(0, 0))       # n_rows == 0: zeros
    assert all(m.shape == (3, 3) and m.dtype == np.int32 and not m.any() for m in empty)
    nothing = engine.f1_counts(big, _classes(rng, 3000), cols=np.zeros(0, dtype=np.int32))                # ncols == 0: nothing
    assert all(m.shape == (0, 0) for m in nothing)
    with pytest.raises(AssertionError, match="accession index outside the panel"):
        engine.f1_counts(big, _classes(rng, 3000), cols=np.array([0, 130], dtype=np.int32))
    with pytest.raises(AssertionError, match="row index outside the panel"):
        engine.f1_counts(big, _classes(rng, 2), rows=np.array([0, 3000], dtype=np.int64))
    with pytest.raises(AssertionError, match="row range outside the panel"):
        engine.f1_counts(big, _classes(rng, 2), rows=range(2999, 3001))
    big.free()
    small.free()


def test_split_layout_at_the_width_of_the_1001_genomes_panel(ctx, monkeypatch):
    rng = np.random.default_rng(7000)
    snps = _calls(rng, 3000, 1135)
    panel = _panel(ctx, snps, "split", monkeypatch)
    assert panel.pitch == 256 + 32                      # main part + tail: the split layout exists at this width
    _check(panel, snps, _classes(rng, 3000))
    panel.free()


@pytest.mark.parametrize("n_acc", [2, 7, 10])
def test_genotype_method_reproduces_the_reference(n_acc, ctx, golden_dir):
    case = np.load(os.path.join(golden_dir, "f1search_a%d.npz" % n_acc))
    snps, gt = case["snps"], case["gt"]
    g = snp_genotype.Genotype.from_arrays(snps, ["A%d" % i for i in range(n_acc)], np.arange(1, len(snps) + 1), ["Chr1"], [[0, len(snps)]])
    assert not g.panel(ctx).packed                      # code 3: the DB stays int8
    hits, ninfo = g.f1_counts(f1search.hard_classes(gt))
    a, b = case["pair_a"], case["pair_b"]
    assert np.array_equal(hits[a, b].astype(np.float64), case["score"]) and np.array_equal(ninfo[a, b].astype(np.int64), case["numinfo"])
    listed = np.arange(40, 200)
    sub = g.f1_counts(f1search.hard_classes(gt)[listed], np.arange(n_acc)[::-1], listed)
    want = f1search_twin.f1_counts(snps, f1search.hard_classes(gt)[listed], np.arange(n_acc)[::-1], listed)
    assert np.array_equal(sub[0], want[0]) and np.array_equal(sub[1], want[1])
    g.panel().free()


def _planted_inputs(case, fractional=False):
    inputs = parsers.ParseInputs("")
    wei = parsers.ParseInputs.get_wei_from_GT(case["s_gt"])
    if fractional:                       # likelihood-like weights: the hard-call counts are a screen then, not the score
        rng = np.random.default_rng(9)
        wei = wei * 0.9 + rng.random(wei.shape) * 0.05
    inputs.load_snp_info(case["s_chr"], case["s_pos"], case["s_gt"], wei, "NA")
    return inputs


@pytest.mark.parametrize("fractional", [False, True], ids=["hard", "pl"])
def test_f1search_end_to_end_on_the_planted_panel(fractional, ctx, tmp_path):
    case = f1search_twin.planted_case()
    pa, pb = f1search_twin.PLANTED_PARENTS
    g = snp_genotype.Genotype.from_arrays(case["snps"], case["names"], case["positions"], case["chrs"], case["chr_regions"])
    g.panel(ctx)
    inputs = _planted_inputs(case, fractional)
    search = f1search.F1Search(inputs, g, str(tmp_path / "out"), top=10, min_sites=100)
    assert np.array_equal(search.db_rows, case["db_rows"]) and np.array_equal(search.classes, case["classes"])
    want = f1search_twin.f1_counts(case["snps"], case["classes"], None, case["db_rows"])
    assert np.array_equal(search.hits, want[0]) and np.array_equal(search.ninfo, want[1])
    assert search.pairs[0] == (pa, pb, 3000, 3000) and len(search.pairs) == 10
    assert search.pairs == [tuple(p) for p in f1search.shortlist(want[0], want[1], 10, 100)]
    stats = search.stats
    assert (stats["best_pair"]["acc_1"], stats["best_pair"]["acc_2"]) == ("acc%02d" % pa, "acc%02d" % pb) and stats["in_top10_route"] is False
    singles = np.argsort(-search.result.probabilies[:40])[:10]
    assert pa not in singles and pb not in singles
    # the shortlist's exact scores: Query.f1_pairs of each pair on its own, bit for bit
    query = g.panel().query(search.db_rows, inputs.wei[search.sample_rows, ])
    for (a, b, h, n), s, ni in zip(search.pairs, search.pair_scores, search.pair_ninfo):
        one_s, one_n = query.f1_pairs(np.array([a, b], dtype=np.int32))
        assert np.array_equal(one_s.view(np.uint64), np.array([s]).view(np.uint64)) and one_n[0] == ni == n
        assert (s == h) if not fractional else (abs(s - h) > 1e-6 and abs(s - h) < 0.15 * n)
    query.free()
    lines = [ln.split("\t") for ln in open(str(tmp_path / "out") + ".f1search.scores.txt").read().splitlines()]
    assert len(lines) == 50 and lines[40][0] == "acc%02dxacc%02d" % (pa, pb) and lines[40][2] == "3000"
    assert [ln[0] for ln in lines[40:]] == ["%sx%s" % (case["names"][a], case["names"][b]) for a, b, _, _ in search.pairs]
    lik = np.array([float(ln[4]) if ln[4] else np.nan for ln in lines])
    assert int(np.nanargmin(lik)) == 40                 # likelihoods over accessions and pairs together: the true pair is the minimum
    g.panel().free()
