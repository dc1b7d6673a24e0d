"""power on the device: ``snpm_panel_sim_counts`` / ``k_win_planes`` + ``k_sim_noise`` + ``k_sim_count`` against the numpy twin
(tests/power_twin.py), cell by cell and without a tolerance, on panels filled through the normal upload path in each of the three
layouts (int8, packed whole rows, packed split rows), at the shapes where the decomposition could break: 32 accessions per tile side of
the count kernel (the full square of tile pairs; the plane kernel works on 64 accessions x 64 rows), 64 rows per word, 1024 rows per
LDS step, 8192 rows per chunk, slabs of the row axis, group boundaries anywhere (several inside one word, empty groups, 64 groups), the
four error rates (0: side A reads the DB planes, no noise launch); the sums over groups against ``kinship_counts``; and the ``Power``
study end to end on the planted panel with two near-identical accessions."""
import numpy as np
import pytest

import power_twin
from snpmatch_amd import engine
from snpmatch_amd.core import power, snp_genotype

pytestmark = pytest.mark.gpu

LAYOUTS = ["int8", "packed", "split"]
RATES = [0.0, 0.05, 0.5, 1.0]
STEP, CHUNK = 1024, 8192                    # rows per LDS step and per block of k_sim_count (F1X_STEP_WORDS / F1X_CHUNK_WORDS x 64)


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


def _check(panel, snps, grp_off, rate, seed, cols=None, rows=None):
    got = engine.sim_counts(panel, grp_off, rate, seed, cols, rows)
    listed = None if rows is None else (np.arange(rows.start, rows.stop) if isinstance(rows, range) else rows)
    want = power_twin.sim_counts(snps, grp_off, power_twin.err_threshold(rate), seed, cols, listed)
    for g, w, name in zip(got, want, ("score", "ninfo")):
        assert g.dtype == np.int32 and g.shape == w.shape, name
        assert np.array_equal(g, w), "%s differs in %d cells" % (name, int((g != w).sum()))
    return got


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n_acc", [1, 2, 31, 32, 33, 65, 130])
def test_tile_edges_of_accessions_words_steps_and_chunks_of_rows(n_acc, layout, ctx, monkeypatch):
    rng = np.random.default_rng(1000 + n_acc)
    snps = _calls(rng, CHUNK + 6, n_acc, other=layout == "int8")
    panel = _panel(ctx, snps, layout, monkeypatch)
    for k, n_rows in enumerate((0, 1, 63, 64, 65, STEP - 1, STEP, STEP + 1, CHUNK - 1, CHUNK, CHUNK + 1)):
        rate = RATES[(k + n_acc + LAYOUTS.index(layout)) % 4]                  # every rate at every layout and row count over the widths
        grp_off = [0, n_rows] if k % 2 else [0, n_rows // 3, n_rows // 3, n_rows - n_rows // 5, n_rows]
        _check(panel, snps, grp_off, rate, 50 + k, rows=range(5, 5 + n_rows) if n_rows else range(0, 0))
    panel.free()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_group_boundaries(layout, ctx, monkeypatch):
    rng = np.random.default_rng(2000)
    n = CHUNK + 8
    snps = _calls(rng, n, 33, other=layout == "int8")
    panel = _panel(ctx, snps, layout, monkeypatch)
    one = _check(panel, snps, [0, n], 0.05, 3)
    cut = _check(panel, snps, [0, 1, 63, 64, 65, STEP, CHUNK, CHUNK + 1, n], 0.05, 3)
    assert all(np.array_equal(c.sum(axis=0), o[0]) for c, o in zip(cut, one))               # the groups add up to the one group
    _check(panel, snps, [0, 70, 75, 100, 200], 0.5, 4, rows=range(3, 203))                   # three boundaries inside one word
    empty = _check(panel, snps, [0, 0, 0, 500, 500, 500, 1100, 1400, 1400], 0.05, 5, rows=range(0, 1400))
    assert not empty[1][0].any() and not empty[1][1].any() and not empty[1][3].any() and not empty[1][-1].any() and empty[1][2].any()
    many = _check(panel, snps, [0] + [g * g for g in range(1, 64)] + [4000], 0.05, 6, rows=range(0, 4000))
    assert many[0].shape[0] == 64 and many[1][0].sum() > 0 and many[1][63].sum() > 0
    with pytest.raises(AssertionError, match="n_grp must be 1 .. 64"):
        engine.sim_counts(panel, list(range(66)), 0.0, 1, rows=range(0, 65))
    with pytest.raises(AssertionError, match="grp_off must end at n"):
        engine.sim_counts(panel, [0, 10], 0.0, 1, rows=range(0, 11))
    panel.free()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_error_rates_and_the_launches_they_take(layout, ctx, monkeypatch):
    rng = np.random.default_rng(3000)
    snps = _calls(rng, 1500, 70, other=layout == "int8")
    panel = _panel(ctx, snps, layout, monkeypatch)
    ctx.profile(True)
    results = {}
    for rate in RATES:
        ctx.profile_reset()
        results[rate] = _check(panel, snps, [0, 700, 1500], rate, 9)
        assert ctx.profile_read("win_planes")[0] == 1 and ctx.profile_read("sim_count")[0] == 1
        assert ctx.profile_read("sim_noise")[0] == (0 if rate == 0 else 1)                  # rate 0: side A reads the DB planes
    ctx.profile(False)
    called = ((snps >= 0) & (snps <= 2)).sum(axis=0)
    assert np.array_equal(np.diagonal(results[0.0][0].sum(axis=0)), called)                 # no error: every call matches itself
    # a redrawn call keeps its class one time in three; 92 000 calls: a standard deviation of the kept share below 0.002
    kept = [np.diagonal(results[r][0].sum(axis=0)).sum() / called.sum() for r in RATES]
    assert kept[0] == 1 and abs(kept[1] - (1 - 0.05 * 2 / 3)) < 0.01 and abs(kept[2] - (1 - 0.5 * 2 / 3)) < 0.01 and abs(kept[3] - 1 / 3) < 0.01
    assert all(np.array_equal(results[r][1], results[0.0][1]) for r in RATES)               # errors move classes, not calls
    other_seed = engine.sim_counts(panel, [0, 700, 1500], 0.5, 10)
    assert not np.array_equal(other_seed[0], results[0.5][0]) and np.array_equal(other_seed[1], results[0.5][1])
    panel.free()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_repeated_column_and_unsorted_rows_with_repeats(layout, ctx, monkeypatch):
    rng = np.random.default_rng(4000)
    snps = _calls(rng, 1500, 70, other=layout == "int8")
    panel = _panel(ctx, snps, layout, monkeypatch)
    cols = rng.permutation(70)[:41].astype(np.int32)
    cols[-1] = cols[3]
    rows = rng.integers(0, 1500, size=1100).astype(np.int64)                          # unsorted, with repeats
    rows[-1] = rows[0]
    clean = _check(panel, snps, [0, 64, 1100], 0.0, 7, cols=cols, rows=rows)
    noisy = _check(panel, snps, [0, 64, 1100], 0.5, 7, cols=cols, rows=rows)
    # the column listed twice: one sample twice without errors, two independent samples with; as a DB column it is the same both times
    assert np.array_equal(clean[0][:, -1], clean[0][:, 3]) and not np.array_equal(noisy[0][:, -1], noisy[0][:, 3])
    assert np.array_equal(noisy[0][:, :, -1], noisy[0][:, :, 3]) and np.array_equal(noisy[1][:, -1], noisy[1][:, 3])
    # a row list that is a dense range gives what row0 / n_rows gives
    dense = _check(panel, snps, [0, 500, 1100], 0.05, 8, cols=cols, rows=range(200, 1300))
    listed = _check(panel, snps, [0, 500, 1100], 0.05, 8, cols=cols, rows=np.arange(200, 1300, dtype=np.int64))
    assert all(np.array_equal(a, b) for a, b in zip(dense, listed))
    panel.free()


@pytest.mark.parametrize("layout", ["int8", "split"])
def test_three_slabs_equal_one_slab(layout, monkeypatch):
    """SNPM_SIM_WS_MB=1: 130 accessions are 192 padded columns, 168 KiB of the seven planes per 1024 rows -- the budget holds 6 such
    steps, 6144 rows per slab.  The groups cross the slab edges.  Once as a range and once as a row list with repeats; the budget
    changes the launches, not the counts -- the hash is keyed by the position of a row in the selection, not in its slab."""
    step_bytes = 7 * 192 * (STEP // 64) * 8
    slab = (1 << 20) // step_bytes * STEP
    assert slab == 6 * STEP
    n = 2 * slab + 1030
    monkeypatch.setenv("SNPM_SIM_WS_MB", "1")
    small = engine.Context(0)
    try:
        rng = np.random.default_rng(5000)
        snps = _calls(rng, n, 130, other=layout == "int8")
        grp_off = [0, 100, slab - 1, slab, slab + 70, 2 * slab + 3, n]
        panel = _panel(small, snps, layout, monkeypatch)
        small.profile(True)
        small.profile_reset()
        ranged = _check(panel, snps, grp_off, 0.05, 11)
        assert [small.profile_read(k)[0] for k in ("win_planes", "sim_noise", "sim_count")] == [3, 3, 3]
        small.profile_reset()
        order = rng.integers(0, n, size=n).astype(np.int64)                           # a row list crosses slabs too; with repeats
        order[-1] = order[0]
        listed = _check(panel, snps, grp_off, 0.5, 12, rows=order)
        assert [small.profile_read(k)[0] for k in ("win_planes", "sim_noise", "sim_count")] == [3, 3, 3]
        small.profile(False)
        panel.free()
        # the same scans under the default budget: one slab, the same counts
        monkeypatch.delenv("SNPM_SIM_WS_MB")
        ctx = engine.default_context()
        whole = _panel(ctx, snps, layout, monkeypatch)
        ctx.profile(True)
        ctx.profile_reset()
        once = engine.sim_counts(whole, grp_off, 0.05, 11)
        assert ctx.profile_read("sim_count")[0] == 1
        ctx.profile(False)
        assert all(np.array_equal(a, b) for a, b in zip(ranged, once))
        again = engine.sim_counts(whole, grp_off, 0.5, 12, rows=order)
        assert all(np.array_equal(a, b) for a, b in zip(listed, again))
        whole.free()
    finally:
        small.close()


def test_split_layout_at_the_width_of_the_1001_genomes_panel(ctx, monkeypatch):
    rng = np.random.default_rng(7000)
    snps = _calls(rng, 2048, 1135)
    panel = _panel(ctx, snps, "split", monkeypatch)
    assert panel.pitch == 256 + 32                      # main part + tail: the split layout exists at this width
    _check(panel, snps, [0, 100, 1030, 2048], 0.05, 13)
    panel.free()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_without_errors_the_groups_sum_to_the_kinship_counts(layout, ctx, monkeypatch):
    """a panel without hets and without the code 3: sample a has a call where a is homozygous, so ninfo[a][b] is kinship's ninfo and
    score[a][b] its same -- on the same selection"""
    rng = np.random.default_rng(8000)
    snps = rng.choice(np.array([-1, 0, 1], dtype=np.int8), size=(2100, 70), p=[0.1, 0.5, 0.4])
    panel = _panel(ctx, snps, layout, monkeypatch)
    cols = rng.permutation(70)[:50].astype(np.int32)
    rows = rng.integers(0, 2100, size=1800).astype(np.int64)
    score, ninfo = _check(panel, snps, [0, 5, 1024, 1500, 1800], 0.0, 1, cols=cols, rows=rows)
    k_ninfo, k_same, k_diff = engine.kinship_counts(panel, cols, rows)
    assert np.array_equal(ninfo.sum(axis=0), k_ninfo) and np.array_equal(score.sum(axis=0), k_same)
    assert np.array_equal(ninfo.sum(axis=0) - score.sum(axis=0), k_diff)
    panel.free()


def test_other_code_missing_column_empty_calls_and_refusals(ctx, monkeypatch):
    rng = np.random.default_rng(9000)
    snps = _calls(rng, 300, 40, other=True)
    snps[:, 7] = -1
    snps[:, 9] = 3                      # "other": no sample call, but informative as a DB column
    panel = _panel(ctx, snps, "int8", monkeypatch)
    score, ninfo = _check(panel, snps, [0, 300], 0.5, 2)
    assert not ninfo[0][7].any() and not ninfo[0][:, 7].any() and not ninfo[0][9].any() and not score[0][:, 9].any()
    assert np.array_equal(ninfo[0][:, 9], ((snps >= 0) & (snps <= 2)).sum(axis=0))
    empty = engine.sim_counts(panel, [0, 0, 0], 0.5, 2, cols=np.array([1, 2, 3], dtype=np.int32), rows=range(0, 0))      # n_rows == 0: zeros
    assert all(m.shape == (2, 3, 3) and m.dtype == np.int32 and not m.any() for m in empty)
    nothing = engine.sim_counts(panel, [0, 300], 0.5, 2, cols=np.zeros(0, dtype=np.int32))                         # ncols == 0: nothing
    assert all(m.shape == (1, 0, 0) for m in nothing)
    with pytest.raises(AssertionError, match="accession index outside the panel"):
        engine.sim_counts(panel, [0, 300], 0.0, 1, cols=np.array([0, 40], dtype=np.int32))
    with pytest.raises(AssertionError, match="row index outside the panel"):
        engine.sim_counts(panel, [0, 2], 0.0, 1, rows=np.array([0, 300], dtype=np.int64))
    with pytest.raises(AssertionError, match="row range outside the panel"):
        engine.sim_counts(panel, [0, 2], 0.0, 1, rows=range(299, 301))
    # a smaller second call sees nothing of the first
    tiny = _calls(rng, 9, 3)
    small = _panel(ctx, tiny, "split", monkeypatch)
    _check(small, tiny, [0, 4, 9], 1.0, 3)
    small.free()
    panel.free()


def test_power_end_to_end_on_the_planted_twins(ctx):
    case = power_twin.planted_case()
    a, b = power_twin.PLANTED_TWINS
    g = snp_genotype.Genotype.from_arrays(case["snps"], case["names"], case["positions"], case["chrs"], case["chr_regions"])
    g.panel(ctx)
    study = power.Power(g, list(power_twin.PLANTED_LEVELS), power_twin.PLANTED_ERR, trials=1, seed=case["seed"]).run()
    rows, grp_off = power.draw_ladder(3000, power_twin.PLANTED_LEVELS, np.random.default_rng(case["seed"]))
    want = power_twin.sim_counts(case["snps"], grp_off, power_twin.err_threshold(power_twin.PLANTED_ERR), case["seed"], None, rows)
    assert np.array_equal(study.score, np.cumsum(want[0], axis=0)) and np.array_equal(study.ninfo, np.cumsum(want[1], axis=0))
    first, last = study.reports[0]
    for me, other in ((a, b), (b, a)):
        assert first["correct"][me] and first["n_ambiguous"][me] == 2 and not first["unique"][me] and first["best_other"][me] == other
        assert last["correct"][me] and last["n_ambiguous"][me] == 1 and last["unique"][me] and last["best_other"][me] == other
    assert first["unique"].sum() == 10 and last["unique"].all()
    stats = study.summary()
    assert stats["fraction_unique"] == [10 / 12, 1.0] and stats["unique_from_level"][str(case["names"][a])] == 3000
    g.panel().free()
