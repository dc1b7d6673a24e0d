"""Panel kinship on the device: ``snpm_panel_kinship_counts`` / ``k_kin_planes`` + ``k_kin_count`` against the numpy twin
(tests/kinship_twin.py), cell by cell and without a tolerance, on panels filled through the normal upload path in each of the three
layouts (int8, packed whole rows, packed split rows), at the shapes where the decomposition could break: 32 accessions per tile side
of the count kernel (a 2 x 2 register tile of pairs per lane; the plane kernel works on 64 accessions x 64 rows), 64 rows per word,
1024 rows per LDS step, 8192 rows per chunk, slabs of the row axis; and ``Genotype.kinship_given_snps`` against the reference's
goldens."""
import os
import re

import numpy as np
import pytest

import kinship_twin
from snpmatch_amd import engine
from snpmatch_amd.core import snp_genotype

pytestmark = pytest.mark.gpu

CHUNK = 8192            # rows per block of k_kin_count (KN_CHUNK_WORDS * 64 of csrc/snpm_k_kin.hpp)
LAYOUTS = ["int8", "packed", "split"]


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


def _check(panel, snps, cols=None, rows=None):
    got = engine.kinship_counts(panel, cols, rows)
    want = kinship_twin.kinship_counts(snps, cols, None if rows is None else (np.arange(rows.start, rows.stop) if isinstance(rows, range) else rows))
    for g, w, name in zip(got, want, ("ninfo", "same", "diff")):
        assert g.dtype == np.int32 and g.shape == w.shape, name
        assert np.array_equal(g, w), "%s differs in %d cells" % (name, int((g != w).sum()))
        assert np.array_equal(g, g.T), name
    return got


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n_acc", [1, 2, 31, 32, 33, 65, 130])
def test_tile_edges_of_accessions_and_words_of_rows(n_acc, layout, ctx, monkeypatch):
    rng = np.random.default_rng(1000 + n_acc)
    snps = _calls(rng, 70, n_acc)
    panel = _panel(ctx, snps, layout, monkeypatch)
    for n_rows in (1, 63, 64, 65):
        _check(panel, snps, rows=range(5, 5 + n_rows))
    _check(panel, snps)
    panel.free()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_chunk_of_the_count_kernel_minus_one_exact_plus_one(layout, ctx, monkeypatch):
    rng = np.random.default_rng(2000)
    snps = _calls(rng, CHUNK + 1, 33)
    panel = _panel(ctx, snps, layout, monkeypatch)
    for n_rows in (CHUNK - 1, CHUNK, CHUNK + 1):
        _check(panel, snps, rows=range(0, n_rows))
    _check(panel, snps, rows=range(1, CHUNK + 1))
    panel.free()


@pytest.mark.parametrize("layout", ["int8", "split"])
def test_three_slabs_with_a_ragged_last_one(layout, monkeypatch):
    """SNPM_KIN_WS_MB=1: 130 accessions are 192 padded columns, 72 KiB of planes per 1024 rows -- the budget holds 14 such steps,
    cut to one whole chunk of 8192 rows per slab"""
    monkeypatch.setenv("SNPM_KIN_WS_MB", "1")
    small = engine.Context(0)
    try:
        rng = np.random.default_rng(3000)
        snps = _calls(rng, 2 * CHUNK + 1030, 130)
        panel = _panel(small, snps, layout, monkeypatch)
        small.profile(True)
        small.profile_reset()
        _check(panel, snps)
        assert small.profile_read("kin_planes")[0] == 3 and small.profile_read("kin_count")[0] == 3
        small.profile_reset()
        order = rng.permutation(len(snps))[:2 * CHUNK + 5].astype(np.int64)           # a row list crosses slabs too
        _check(panel, snps, rows=order)
        assert small.profile_read("kin_count")[0] == 3
        small.profile(False)
        panel.free()
    finally:
        small.close()


def _kernel_constant(name):
    """a ``constexpr int`` of csrc/snpm_k_kin.hpp"""
    text = open(os.path.join(os.path.dirname(os.path.abspath(engine.__file__)), "csrc", "snpm_k_kin.hpp")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


def test_a_row_list_of_three_slabs_over_a_small_panel(monkeypatch):
    """SNPM_KIN_WS_MB=1: 33 accessions are 64 padded columns, 24 KiB of planes per 1024-row step -- the budget holds 42 steps, cut
    to the 40 of five whole chunks: a slab is 40960 rows.  The list is longer than the panel: 2 slabs + 65 entries, with repeats,
    each slab's part uploaded on its own."""
    step_words, chunk_words, pl_cols = (_kernel_constant(k) for k in ("KN_STEP_WORDS", "KN_CHUNK_WORDS", "KN_PL_COLS"))
    cols_pad = -(-33 // pl_cols) * pl_cols
    steps = max(1, (1 << 20) // (3 * cols_pad * step_words * 8))
    per_chunk = chunk_words // step_words
    if steps >= per_chunk:
        steps = steps // per_chunk * per_chunk
    slab_rows = min(steps, 65535 * per_chunk) * step_words * 64
    assert chunk_words * 64 == CHUNK and slab_rows == 40960
    monkeypatch.setenv("SNPM_KIN_WS_MB", "1")
    small = engine.Context(0)
    try:
        rng = np.random.default_rng(8000)
        snps = _calls(rng, 300, 33)
        panel = _panel(small, snps, "packed", monkeypatch)
        rows = rng.integers(0, 300, size=2 * slab_rows + 65).astype(np.int64)
        small.profile(True)
        small.profile_reset()
        _check(panel, snps, rows=rows)
        assert small.profile_read("kin_planes")[0] == 3 and small.profile_read("kin_count")[0] == 3
        small.profile(False)
        panel.free()
    finally:
        small.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_column_subset_with_a_repeat_and_unsorted_rows_with_repeats(layout, ctx, monkeypatch):
    rng = np.random.default_rng(4000)
    snps = _calls(rng, 1500, 70)
    panel = _panel(ctx, snps, layout, monkeypatch)
    cols = rng.permutation(70)[:41].astype(np.int32)
    cols[-1] = cols[3]
    rows = rng.integers(0, 1500, size=1100).astype(np.int64)                          # unsorted, with repeats
    ninfo, same, diff = _check(panel, snps, cols=cols, rows=rows)
    assert np.array_equal(ninfo[-1], ninfo[3]) and same[3, -1] == same[3, 3] and diff[3, -1] == 0
    # a row list that is a dense range gives what row0 / n_rows gives
    dense = _check(panel, snps, cols=cols, rows=range(200, 1300))
    listed = _check(panel, snps, cols=cols, rows=np.arange(200, 1300, dtype=np.int64))
    assert all(np.array_equal(a, b) for a, b in zip(dense, listed))
    panel.free()


def test_all_missing_accession_and_the_other_code_of_int8_panels(ctx, monkeypatch):
    rng = np.random.default_rng(5000)
    snps = _calls(rng, 300, 40, other=True)
    snps[:, 7] = -1
    snps[:, 9] = 3                      # "other": informative, in neither same nor diff
    panel = _panel(ctx, snps, "int8", monkeypatch)
    ninfo, same, diff = _check(panel, snps)
    assert not ninfo[7].any() and not ninfo[:, 7].any()
    assert ninfo[9, 9] == 300 and not same[9].any() and not diff[9].any()
    assert np.array_equal(ninfo[9], (snps >= 0).sum(axis=0))
    kin = kinship_twin.kinship(ninfo, same, diff)
    assert np.isnan(kin[7]).all() and np.isnan(kin[:, 7]).all() and not np.isnan(np.delete(np.delete(kin, 7, 0), 7, 1)).any()
    panel.free()


def test_a_smaller_second_call_sees_nothing_of_the_first(ctx, monkeypatch):
    rng = np.random.default_rng(6000)
    snps = _calls(rng, 3000, 130)
    big = _panel(ctx, snps, "int8", monkeypatch)
    _check(big, snps)
    tiny = _calls(rng, 9, 3)
    small = _panel(ctx, tiny, "split", monkeypatch)
    _check(small, tiny)
    _check(big, snps, cols=np.array([5, 6], dtype=np.int32), rows=range(0, 1))
    empty = engine.kinship_counts(big, cols=np.array([1, 2, 3], dtype=np.int32), rows=range(0, 0))
    assert all(m.shape == (3, 3) and not m.any() for m in empty)
    none = engine.kinship_counts(big, cols=np.zeros(0, dtype=np.int32))
    assert all(m.shape == (0, 0) for m in none)
    with pytest.raises(AssertionError, match="accession index outside the panel"):
        engine.kinship_counts(big, cols=np.array([0, 130], dtype=np.int32))
    with pytest.raises(AssertionError, match="row index outside the panel"):
        engine.kinship_counts(big, rows=np.array([0, 3000], dtype=np.int64))
    with pytest.raises(AssertionError, match="row range outside the panel"):
        engine.kinship_counts(big, rows=range(2999, 3001))
    big.free()
    small.free()


def test_split_layout_at_the_width_of_the_1001_genomes_panel(ctx, monkeypatch):
    rng = np.random.default_rng(7000)
    snps = _calls(rng, 3000, 1135)
    panel = _panel(ctx, snps, "split", monkeypatch)
    assert panel.pitch == 256 + 32                      # main part + tail: the split layout exists at this width
    _check(panel, snps)
    panel.free()


@pytest.mark.parametrize("packed", [False, True], ids=["int8", "packed"])
def test_genotype_method_reproduces_the_reference_bits(packed, ctx, golden_dir):
    case = np.load(os.path.join(golden_dir, "kinship_a7_r2500.npz"))
    snps = case["snps"]
    g = snp_genotype.Genotype.from_arrays(snps, ["A%d" % i for i in range(7)], np.arange(1, 2501), ["Chr1"], [[0, 2500]])
    assert g.panel(ctx, packed=packed).packed == packed

    def same_bits(a, b):
        nan = np.isnan(b)
        return a.dtype == np.float64 and np.array_equal(np.isnan(a), nan) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))
    assert same_bits(g.kinship_given_snps(), case["kinship"])
    assert same_bits(g.kinship_given_snps(filter_acc_ix=case["acc_ix"]), case["method_kinship"])
    # the listed rows are used (the reference would take the first len(rows) rows instead)
    rows = np.arange(1000, 2500)
    assert same_bits(g.kinship_given_snps(filter_snp_ix=rows), snp_genotype.calc_kinship_mat(snps[rows]))
    g.panel().free()
