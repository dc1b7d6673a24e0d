"""Site statistics on the device: ``snpm_panel_site_counts`` / ``k_site_counts`` against the numpy twin (tests/sitestats_twin.py),
cell by cell and without a tolerance, on panels filled through the normal upload path in each of the three layouts (int8, packed
whole rows, packed split rows), at the shapes where the decomposition could break: 32 columns per word, 16 columns per int8 load
and 64 per packed one, a row per lane up to eight lanes per row (1135 accessions), 64 / lanes rows per wave, 8 waves per block,
SNPM_SITE_MAX_GROUPS groups per call, slabs of the row axis; and ``Genotype.get_af_snps`` / ``polarize_mask`` against the
reference's goldens."""
import os

import numpy as np
import pytest

import kinship_twin
import sitestats_twin
from snpmatch_amd import engine
from snpmatch_amd.core import snp_genotype

pytestmark = pytest.mark.gpu

LAYOUTS = ["int8", "packed", "split"]
MAX_GROUPS = engine.SITE_MAX_GROUPS


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


def _groups(rng, n_acc, kind):
    if kind == "all":
        return None
    if kind == "subset":
        return [np.sort(rng.permutation(n_acc)[:max(1, n_acc * 2 // 3)])]
    if kind == "three":                     # overlapping, one empty
        return [rng.permutation(n_acc)[:max(1, n_acc // 2)], np.zeros(0, dtype=np.int64), rng.permutation(n_acc)[:max(1, n_acc * 3 // 4)]]
    if kind == "repeats":                   # goes through layers
        cols = rng.permutation(n_acc)[:max(1, n_acc // 2)]
        return [np.concatenate([cols, cols[:3], cols[:1]])]
    n = MAX_GROUPS + (kind == "max+1")
    return [rng.permutation(n_acc)[:1 + (7 * k) % n_acc] for k in range(n)]


def _check(panel, snps, groups=None, rows=None):
    got = engine.site_counts(panel, groups, rows)
    want = sitestats_twin.site_counts(snps, groups, rows)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want), "%d cells differ" % int((got != want).sum())
    return got


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n_acc", [1, 2, 31, 32, 33, 63, 64, 65, 130])
def test_word_edges_of_accessions_and_wave_edges_of_rows(n_acc, layout, ctx, monkeypatch):
    rng = np.random.default_rng(1000 + n_acc)
    snps = _calls(rng, 70, n_acc, other=layout == "int8")
    panel = _panel(ctx, snps, layout, monkeypatch)
    for n_rows in (1, 63, 64, 65):
        for kind in ("all", "subset", "three"):
            _check(panel, snps, _groups(rng, n_acc, kind), range(5, 5 + n_rows))
    for kind in ("max", "max+1", "repeats"):
        _check(panel, snps, _groups(rng, n_acc, kind))
    _check(panel, snps, _groups(rng, n_acc, "three"), rng.integers(0, 70, size=90).astype(np.int64))      # unsorted, with repeats
    panel.free()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_width_of_the_1001_genomes_panel(layout, ctx, monkeypatch):
    rng = np.random.default_rng(2000)
    snps = _calls(rng, 300, 1135, other=layout == "int8")
    snps[7] = -1
    if layout == "int8":
        snps[9] = 3                         # "other": informative, in none of c0..c2
    panel = _panel(ctx, snps, layout, monkeypatch)
    if layout == "split":
        assert panel.pitch == 256 + 32      # main part + tail: the split layout exists at this width
    got = _check(panel, snps)
    assert not got[0, 7].any() and (layout != "int8" or got[0, 9].tolist() == [0, 0, 0, 1135])
    for kind in ("subset", "three", "max", "max+1", "repeats"):
        _check(panel, snps, _groups(rng, 1135, kind), range(3, 292))
    _check(panel, snps, _groups(rng, 1135, "three"), rng.integers(0, 300, size=333).astype(np.int64))
    panel.free()


@pytest.mark.parametrize("layout", ["int8", "split"])
def test_three_slabs_with_a_ragged_last_one(layout, monkeypatch):
    """SNPM_SITE_WS_MB=1 and three groups: slab_rows = floor(2^20 / (16 * 3)) rounded down to a multiple of 64 = 21824 rows"""
    monkeypatch.setenv("SNPM_SITE_WS_MB", "1")
    small = engine.Context(0)
    try:
        rng = np.random.default_rng(3000)
        n_groups = 3
        slab_rows = max(64, (1 << 20) // (16 * n_groups) // 64 * 64)
        assert slab_rows == 21824
        snps = _calls(rng, 2 * slab_rows + 1030, 33)
        groups = _groups(rng, 33, "three")
        panel = _panel(small, snps, layout, monkeypatch)
        small.profile(True)
        small.profile_reset()
        _check(panel, snps, groups)
        assert small.profile_read("site_counts")[0] == -(-len(snps) // slab_rows) == 3
        small.profile_reset()
        order = rng.permutation(len(snps))[:2 * slab_rows + 5].astype(np.int64)          # a row list crosses slabs too
        _check(panel, snps, groups, order)
        assert small.profile_read("site_counts")[0] == 3
        small.profile(False)
        panel.free()
    finally:
        small.close()


def test_a_row_list_of_three_slabs_over_a_small_panel(monkeypatch):
    """SNPM_SITE_WS_MB=1 and three groups: slabs of 21824 rows; the list is longer than the panel: 2 slabs + 65 entries, with
    repeats, each slab's part uploaded on its own"""
    monkeypatch.setenv("SNPM_SITE_WS_MB", "1")
    small = engine.Context(0)
    try:
        rng = np.random.default_rng(8000)
        slab_rows = max(64, (1 << 20) // (16 * 3) // 64 * 64)
        assert slab_rows == 21824
        snps = _calls(rng, 300, 130)
        panel = _panel(small, snps, "split", monkeypatch)
        rows = rng.integers(0, 300, size=2 * slab_rows + 65).astype(np.int64)
        small.profile(True)
        small.profile_reset()
        _check(panel, snps, _groups(rng, 130, "three"), rows)
        assert small.profile_read("site_counts")[0] == 3
        small.profile(False)
        panel.free()
    finally:
        small.close()


def test_kinship_and_site_calls_share_the_row_buffer_of_a_context(monkeypatch):
    """one context, one row-list workspace for both scans: site counts, kinship and site counts again, each with a row list of its
    own (unsorted, with repeats, of different lengths), each equal to its twin"""
    one = engine.Context(0)
    try:
        rng = np.random.default_rng(9000)
        snps = _calls(rng, 300, 130, other=True)
        panel = _panel(one, snps, "int8", monkeypatch)
        groups = _groups(rng, 130, "three")
        _check(panel, snps, groups, rng.integers(0, 300, size=200).astype(np.int64))
        kin_rows = rng.integers(0, 300, size=129).astype(np.int64)
        got = engine.kinship_counts(panel, None, kin_rows)
        for g, w in zip(got, kinship_twin.kinship_counts(snps, None, kin_rows)):
            assert g.dtype == np.int32 and np.array_equal(g, w)
        _check(panel, snps, groups, rng.integers(0, 300, size=260).astype(np.int64))
        panel.free()
    finally:
        one.close()


def test_a_smaller_second_call_sees_nothing_of_the_first_and_the_refusals_that_need_a_panel(ctx, monkeypatch):
    rng = np.random.default_rng(6000)
    snps = _calls(rng, 3000, 130, other=True)
    big = _panel(ctx, snps, "int8", monkeypatch)
    _check(big, snps, _groups(rng, 130, "max"))
    tiny = _calls(rng, 9, 3)
    small = _panel(ctx, tiny, "split", monkeypatch)
    _check(small, tiny, [[2, 0]])
    _check(big, snps, [np.array([5, 6])], range(0, 1))
    assert engine.site_counts(big, [[1, 2, 3]], range(0, 0)).shape == (1, 0, 4)
    assert not engine.site_counts(big, [[], []], range(0, 10)).any()
    lib = ctx.lib

    def raw(cols, off, rows=None, n_rows=4):
        cols, off = np.asarray(cols, dtype=np.int32), np.asarray(off, dtype=np.int64)
        out = np.zeros((len(off) - 1, n_rows, 4), dtype=np.int32)
        rows = None if rows is None else np.asarray(rows, dtype=np.int64)
        return lib.snpm_panel_site_counts(big.h, engine.ptr(cols), engine.ptr(off), len(off) - 1, engine.ptr(rows), 0, n_rows, engine.ptr(out)), out
    assert raw([3, 9, 3], [0, 3])[0] == engine._lib.SNPM_ERR_BADARG and "listed twice in one group" in lib.snpm_last_error(ctx.h).decode()
    rc, out = raw([3, 9, 3], [0, 2, 3])                             # the same column in TWO groups is fine
    assert rc == 0 and np.array_equal(out, sitestats_twin.site_counts(snps, [[3, 9], [3]], range(0, 4)))
    with pytest.raises(AssertionError, match="accession index outside the panel"):
        engine.site_counts(big, [[0, 130]])
    with pytest.raises(AssertionError, match="accession index outside the panel"):
        engine.site_counts(big, [[-1]])
    with pytest.raises(AssertionError, match="row index outside the panel"):
        engine.site_counts(big, None, np.array([0, 3000], dtype=np.int64))
    with pytest.raises(AssertionError, match="row range outside the panel"):
        engine.site_counts(big, None, range(2999, 3001))
    big.free()
    small.free()


def test_a_whole_wave_per_row(ctx, monkeypatch):
    rng = np.random.default_rng(7000)
    snps = _calls(rng, 40, 5000, other=True)
    panel = _panel(ctx, snps, "int8", monkeypatch)
    _check(panel, snps, _groups(rng, 5000, "three"))
    panel.free()


@pytest.mark.parametrize("packed", [False, True], ids=["int8", "packed"])
def test_genotype_methods_reproduce_the_reference_bits(packed, ctx, golden_dir):
    case = np.load(os.path.join(golden_dir, "sitestats_a7_r1001.npz"))
    snps = case["snps"] if not packed else np.where(case["snps"] == 3, -1, case["snps"]).astype(np.int8)      # a packed panel has no code 3
    g = snp_genotype.Genotype.from_arrays(snps, ["A%d" % i for i in range(7)], np.arange(1, 1002), ["Chr1"], [[0, 1001]])
    assert g.panel(ctx, packed=packed).packed == packed

    def same_bits(a, b):
        nan = np.isnan(b)
        return a.dtype == np.float64 and np.array_equal(np.isnan(a), nan) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))
    pops = {"north": case["pop_north"], "south": case["pop_south"]}
    rows = case["row_ix"]
    if not packed:                          # the goldens themselves
        maf, nind = g.get_af_snps(0, return_nind=True)
        assert same_bits(maf, case["m_all"][0]) and nind.dtype == np.int64 and np.array_equal(nind, case["m_all"][1])
        assert same_bits(g.get_af_snps(1, filter_acc_ix=case["acc_ix"], return_maf=False), case["m_listed"][0])
        assert same_bits(g.get_af_snps(0, filter_snps_ix=rows, filter_acc_ix=case["acc_ix"], polarize_geno=0), case["m_listed_rows"][0])
        assert same_bits(g.get_af_snps(0, filter_snps_ix=rows, polarize_geno=2, return_maf=False), case["m_all_rows"][0])
        maf, nind = g.get_af_snps(0, True, None, pops)
        got, count = g.get_af_snps(2, True, rows, pops, 1, False)
        for pop in pops:
            assert same_bits(maf[pop], case["m_pops_" + pop][0]) and nind[pop].dtype == np.float64 and np.array_equal(nind[pop], case["m_pops_" + pop][1])
            assert same_bits(got[pop], case["m_pops_rows_" + pop][0]) and np.array_equal(count[pop], case["m_pops_rows_" + pop][1])
        head = snps[:case["polarized"].shape[1]]
        for pg in (0, 1):
            flipped = (case["polarized"][pg] != head).any(axis=1)
            mask = g.polarize_mask(None, np.arange(len(head)), pg)
            assert not (flipped & ~mask).any() and np.array_equal(mask, (head == pg).sum(axis=1) > 3.5)
    # against the host function of the same semantics, both formats
    for acc_ix, row_ix in ((None, None), (case["acc_ix"], rows)):
        sub = snps if row_ix is None else snps[row_ix]
        sub = sub if acc_ix is None else sub[:, acc_ix]
        want, num = snp_genotype.calculate_af_snp_mat(sub, 1, 1, True)
        maf, nind = g.get_af_snps(1, True, row_ix, acc_ix)
        assert same_bits(maf, want) and np.array_equal(nind, num)
        assert np.array_equal(g.polarize_mask(acc_ix, row_ix), (sub == 1).sum(axis=1) > sub.shape[1] / 2.0)
    g.panel().free()
