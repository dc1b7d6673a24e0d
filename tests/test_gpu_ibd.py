"""ibd on the device: ``snpm_panel_ibd_counts`` / ``k_win_planes`` + ``k_ibd_count`` + ``k_ibd_runs`` against the numpy twin
(tests/ibd_twin.py), cell by cell, all seven matrices and both bitsets by integer equality, on panels filled through the normal upload
path in each of the three layouts (int8, packed whole rows, packed split rows), at the shapes where the decomposition could break:
32 accessions per tile side of the count kernel, 64 rows per word with window boundaries anywhere inside it, 1024 rows per LDS step,
groups of whole windows of about 8192 rows, 32 windows per bit word, slabs of whole windows; against two other device calls; and the
``ibd`` command end to end on the planted panel."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ibd_twin as twin
from snpmatch_amd import cli, engine
from snpmatch_amd.core import ibd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = ["int8", "packed", "split"]
NAMES = engine.IBD_COUNT_NAMES
ALL = NAMES + ("used_bits", "shared_bits")


def _kernel_constant(name):
    """a ``constexpr int`` of csrc/snpm_k_f1x.hpp (the tiling k_ibd_count keeps)"""
    text = open(os.path.join(os.path.dirname(os.path.abspath(engine.__file__)), "csrc", "snpm_k_f1x.hpp")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


CHUNK = _kernel_constant("F1X_CHUNK_WORDS") * 64          # rows a group of windows aims at
STEP = _kernel_constant("F1X_STEP_WORDS") * 64            # rows per LDS step


@pytest.fixture(scope="module")
def ctx():
    return engine.default_context()


def _calls(rng, n_rows, n_acc, other=False, block=16):
    """accessions that copy one of three founders in blocks of rows, 2 % of the calls flipped, 10 % missing, 4 % het (int8 panels:
    3 % the "other" code): whole windows in which two accessions are identical, windows with a single difference, windows apart"""
    founders = rng.integers(0, 2, size=(n_rows, 3)).astype(np.int8)
    pick = np.repeat(rng.integers(0, 3, size=((n_rows + block - 1) // block, n_acc)), block, axis=0)[:n_rows]
    v = np.take_along_axis(founders, pick, axis=1)
    v = np.where(rng.random((n_rows, n_acc)) < 0.02, 1 - v, v).astype(np.int8)
    u = rng.random((n_rows, n_acc))
    v[u < 0.10] = -1
    v[(u >= 0.10) & (u < 0.14)] = 2
    if other:
        v[(u >= 0.14) & (u < 0.17)] = 3
    return v


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


def _same(got, want, what=""):
    for name in ALL:
        g, w = got[name], want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert np.array_equal(g, w), "%s %s differs in %d entries" % (what, name, int((g != w).sum()))


def _check(panel, snps, win_off, min_sites=1, ppm=1000, min_run=1, cols=None, rows=None):
    got = engine.ibd_counts(panel, win_off, min_sites, ppm, min_run, cols, rows)
    _same(got, twin.ibd_counts(snps, win_off, min_sites, ppm, min_run, cols, rows))
    assert all(np.array_equal(got[k], np.swapaxes(got[k], 0, 1)) for k in ALL)
    return got


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n_acc", [1, 2, 31, 32, 33, 65, 130])
def test_tile_edges_of_accessions_and_window_boundaries_inside_words(n_acc, layout, ctx, monkeypatch):
    rng = np.random.default_rng(1000 + n_acc)
    snps = _calls(rng, 70, n_acc, other=layout == "int8")
    assert layout != "int8" or (snps == 3).any()
    panel = _panel(ctx, snps, layout, monkeypatch)
    for k, win_off in enumerate(_window_sets(70)):
        _check(panel, snps, win_off, 1 + k % 2, (0, 1000, 100000, 1000000)[k], 1 + k % 3)
    for n_rows in (1, 63, 64, 65):
        _check(panel, snps, _window_sets(n_rows)[n_rows % 4], 1, 50000, 1, rows=range(5, 5 + n_rows))
    panel.free()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_groups_at_chunk_minus_one_exact_plus_one(layout, ctx, monkeypatch):
    """33 accessions at chunk - 1 / chunk / chunk + 1 rows, as one window (chunk + 1: a window longer than a chunk, a group of its own
    with one more step) and as windows of 100 rows (groups of 81 windows: a group boundary falls inside a bit word, which two
    groups then OR into; the boundaries fall anywhere inside the 64-row words)"""
    rng = np.random.default_rng(2000)
    snps = _calls(rng, CHUNK + 1, 33, other=layout == "int8", block=300)
    panel = _panel(ctx, snps, layout, monkeypatch)
    for n_rows in (CHUNK - 1, CHUNK, CHUNK + 1):
        _check(panel, snps, np.array([0, n_rows]), 1, 400000, 1, rows=range(0, n_rows))
        got = _check(panel, snps, _every(n_rows, 100), 20, 30000, 2, rows=range(0, n_rows))
        off_diag = ~np.eye(33, dtype=bool)
        assert (got["n_runs"][off_diag] > 0).any() and (got["w_used"] > got["w_shared"]).any()        # runs and breaks are really there
    _check(panel, snps, np.array([0, STEP - 1, STEP + 1]), 1, 400000, 1, rows=range(1, STEP + 2))      # a window across an LDS step
    panel.free()


@pytest.mark.parametrize("n_win", [31, 32, 33, 65])
def test_bit_words_fill_exactly_and_spill_by_one(n_win, ctx, monkeypatch):
    rng = np.random.default_rng(2500 + n_win)
    snps = _calls(rng, 7 * n_win, 33, block=21)
    panel = _panel(ctx, snps, LAYOUTS[n_win % 3], monkeypatch)
    got = _check(panel, snps, _every(7 * n_win, 7), 3, 0, 2)
    assert got["used_bits"].shape == (33, 33, (n_win + 31) // 32) and got["used_bits"][0, 0, -1] >> ((n_win - 1) % 32) == 1
    panel.free()


def _worker(tmp_path, env, **arrays):
    np.savez(tmp_path / "in.npz", **arrays)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ibd_slab_worker.py"), str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       capture_output=True, text=True, env=dict(os.environ, **env), timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return np.load(tmp_path / "out.npz")


@pytest.mark.parametrize("layout", ["int8", "split"])
def test_three_slabs_of_whole_windows_equal_one_slab(layout, ctx, monkeypatch, tmp_path):
    """SNPM_IBD_WS_MB=1 in a fresh child process: 130 accessions are 192 padded columns, 96 KiB of planes per 1024 rows -- the
    budget holds 10 such steps.  Three windows of 9000 rows (9 steps each) are three slabs; a slab is never cut inside a window.
    Once as a range and once as a row list with repeats; then a window larger than the budget, a slab of its own.  The budget
    changes the launches, not the result: the same scan under the default budget is one slab."""
    step_bytes = 4 * 192 * (STEP // 64) * 8
    assert (1 << 20) // step_bytes == 10
    rng = np.random.default_rng(3000)
    snps = _calls(rng, 27000, 130, other=layout == "int8", block=2000)
    win_off = np.array([0, 9000, 9000, 18000, 27000], dtype=np.int64)
    wide = np.array([0, 500, 26000, 27000], dtype=np.int64)
    order = rng.integers(0, len(snps), size=27000).astype(np.int64)                   # a row list crosses slabs too; with repeats
    order[-1] = order[0]
    z = _worker(tmp_path, {"SNPM_IBD_WS_MB": "1"}, mode="slabs", packed=layout != "int8", snps=snps, win_off=win_off, rows=order, wide=wide,
                params=np.array([20, 300000, 1]))
    assert z["launches"].tolist() == [[3, 3, 1]] * 3                  # planes and counts once per slab, the runs once per call
    want = twin.ibd_counts(snps, win_off, 20, 300000, 1)
    _same({k: z["range_" + k] for k in ALL}, want, "range")
    _same({k: z["list_" + k] for k in ALL}, twin.ibd_counts(snps, win_off, 20, 300000, 1, rows=order), "list")
    _same({k: z["wide_" + k] for k in ALL}, twin.ibd_counts(snps, wide, 20, 300000, 1), "wide")
    assert 0 < want["w_shared"][~np.eye(130, dtype=bool)].sum() < want["w_used"][~np.eye(130, dtype=bool)].sum()
    panel = _panel(ctx, snps, layout, monkeypatch)
    ctx.profile(True)
    ctx.profile_reset()
    once = engine.ibd_counts(panel, win_off, 20, 300000, 1)
    assert [ctx.profile_read(k)[0] for k in ("win_planes", "ibd_count", "ibd_runs")] == [1, 1, 1]
    ctx.profile(False)
    _same(once, {k: z["range_" + k] for k in ALL}, "one slab")
    panel.free()


def test_parameters_column_list_and_two_other_device_calls(ctx, monkeypatch):
    rng = np.random.default_rng(5000)
    snps = _calls(rng, 1500, 70, other=True, block=40)
    snps[:, 7] = -1
    panel = _panel(ctx, snps, "int8", monkeypatch)
    cols = rng.permutation(70)[:41].astype(np.int32)
    cols[3] = cols[-1] = 11                                                             # a repeated column (not the blank one)
    rows = rng.integers(0, 1500, size=1100).astype(np.int64)                          # unsorted, with repeats
    win_off = np.sort(np.concatenate([[0, 1100], rng.integers(0, 1101, size=150)])).astype(np.int64)      # ~7 rows a window, some empty
    one = _check(panel, snps, win_off, 1, 1000, 1, cols, rows)
    five = _check(panel, snps, win_off, 5, 1000, 1, cols, rows)
    assert (five["w_used"] <= one["w_used"]).all() and (five["w_used"] < one["w_used"]).any()
    assert np.array_equal(one["used_bits"][3, 40], one["shared_bits"][3, 40]) and one["d_shared"][3, 40] == 0      # the same column twice
    table = _every(1500, 25)
    by_ppm = [_check(panel, snps, table, 5, ppm, 1) for ppm in (0, 1000, 50000, 1000000)]
    assert np.array_equal(by_ppm[0]["w_shared"], by_ppm[1]["w_shared"])                # 1000 ppm of at most 25 rows: no difference allowed either
    assert (by_ppm[1]["w_shared"] <= by_ppm[2]["w_shared"]).all() and (by_ppm[1]["w_shared"] < by_ppm[2]["w_shared"]).any()
    assert np.array_equal(by_ppm[3]["w_shared"], by_ppm[3]["w_used"]) and np.array_equal(by_ppm[3]["run_max"], by_ppm[3]["w_used"])
    run1, run3 = by_ppm[2], _check(panel, snps, table, 5, 50000, 3)
    assert all(np.array_equal(run1[k], run3[k]) for k in ("w_used", "w_shared", "n_shared", "d_shared", "run_max", "used_bits", "shared_bits"))
    assert (run3["n_runs"] <= run1["n_runs"]).all() and (run3["n_runs"] < run1["n_runs"]).any() and (run3["w_in_runs"] < run1["w_in_runs"]).any()
    assert not run1["w_used"][7].any() and not run1["used_bits"][:, 7].any()          # the blank accession: no window used
    # runs_from_bits on the device's bitsets gives the device's run figures
    for a, b in ((0, 1), (2, 30), (11, 11), (69, 3)):
        for got, min_run in ((run1, 1), (run3, 3)):
            runs = ibd.runs_from_bits(got["used_bits"][a, b], got["shared_bits"][a, b], min_run)
            assert (len(runs), int(runs[:, 2].sum())) == (got["n_runs"][a, b], got["w_in_runs"][a, b])
        every = ibd.runs_from_bits(run1["used_bits"][a, b], run1["shared_bits"][a, b], 1)
        assert run1["run_max"][a, b] == (every[:, 2].max() if len(every) else 0)
    # device against device: the pair cells of window_counts for a listed subset give the call's bits for those cells
    pairs = np.array([(0, 1), (2, 30), (30, 2), (11, 11), (69, 3), (7, 8)])
    _, cells = engine.window_counts(panel, table, None, pairs)
    n, d = cells[:, :, 2].astype(np.int64) + cells[:, :, 3], cells[:, :, 3].astype(np.int64)
    used, shared = twin.states(n, d, 5, 50000)
    for i, (a, b) in enumerate(pairs.tolist()):
        assert np.array_equal(ibd.unpack_bits(run1["used_bits"][a, b], len(table) - 1), used[i])
        assert np.array_equal(ibd.unpack_bits(run1["shared_bits"][a, b], len(table) - 1), shared[i])
        assert run1["n_shared"][a, b] == n[i][shared[i]].sum() and run1["d_shared"][a, b] == d[i][shared[i]].sum()
    # ... and with one window n_shared at 1 000 000 ppm is same + diff of kinship_counts
    _, same, diff = engine.kinship_counts(panel)
    whole = engine.ibd_counts(panel, np.array([0, 1500]), 1, 1000000, 1)
    assert np.array_equal(whole["n_shared"], same + diff) and np.array_equal(whole["d_shared"], diff)
    assert np.array_equal(whole["w_used"], (same + diff > 0).astype(np.int32))
    # the bitset pointers NULL against given
    bare = engine.ibd_counts(panel, table, 5, 50000, 3, bits=False)
    assert bare["used_bits"] is None and bare["shared_bits"] is None and all(np.array_equal(bare[k], run3[k]) for k in NAMES)
    with pytest.raises(AssertionError, match="win_off must end at n"):
        engine.ibd_counts(panel, np.array([0, 1499]))
    with pytest.raises(AssertionError, match="max_diff_ppm must lie in 0 .. 1000000"):
        engine.ibd_counts(panel, np.array([0, 1500]), 1, 1000001)
    with pytest.raises(AssertionError, match="min_run must be 1 or more"):
        engine.ibd_counts(panel, np.array([0, 1500]), 1, 0, 0)
    panel.free()


def test_split_layout_at_the_width_of_the_1001_genomes_panel_and_empty_calls(ctx, monkeypatch):
    rng = np.random.default_rng(7000)
    snps = _calls(rng, 1500, 1135, block=75)
    panel = _panel(ctx, snps, "split", monkeypatch)
    assert panel.pitch == 256 + 32                      # main part + tail: the split layout exists at this width
    win_off = np.sort(np.concatenate([[0, 1500], rng.integers(0, 1501, size=39)])).astype(np.int64)       # 40 windows
    got = _check(panel, snps, win_off, 10, 30000, 2)
    assert got["used_bits"].shape == (1135, 1135, 2) and (got["n_runs"][~np.eye(1135, dtype=bool)] > 0).any()
    three = np.array([1, 2, 3], dtype=np.int32)
    empty = engine.ibd_counts(panel, np.array([0, 0, 0]), cols=three, rows=range(0, 0))                   # n_rows == 0: zeros, two windows
    assert all(empty[k].shape == (3, 3) and empty[k].dtype == np.int32 and not empty[k].any() for k in NAMES)
    assert all(empty[k].shape == (3, 3, 1) and empty[k].dtype == np.uint32 and not empty[k].any() for k in ("used_bits", "shared_bits"))
    none = engine.ibd_counts(panel, np.array([0]), cols=three, rows=range(7, 7))                          # n_win == 0: zeros, no bit word
    assert all(not none[k].any() for k in NAMES) and none["used_bits"].shape == (3, 3, 0)
    nothing = engine.ibd_counts(panel, win_off, cols=np.zeros(0, dtype=np.int32))                         # ncols == 0: nothing
    assert all(nothing[k].shape == (0, 0) for k in NAMES) and nothing["shared_bits"].shape == (0, 0, 2)
    with pytest.raises(AssertionError, match="accession index outside the panel"):
        engine.ibd_counts(panel, win_off, cols=np.array([0, 1135], dtype=np.int32))
    with pytest.raises(AssertionError, match="row index outside the panel"):
        engine.ibd_counts(panel, np.array([0, 2]), rows=np.array([0, 1500], dtype=np.int64))
    panel.free()


def test_bitsets_over_the_budget_are_refused_with_the_bytes_and_the_variable(tmp_path):
    """SNPM_IBD_BITS_MB=1 in a fresh child process: 130 x 130 cells x 10 bit words x 2 bitsets are 1 352 000 bytes, more than 1 MiB;
    one bit word per cell fits"""
    rng = np.random.default_rng(8000)
    snps = _calls(rng, 600, 130)
    small = _every(600, 20)
    z = _worker(tmp_path, {"SNPM_IBD_BITS_MB": "1"}, mode="refuse", packed=True, snps=snps, win_off=_every(600, 2), small=small, params=np.array([5, 1000, 1]))
    msg = str(z["message"])
    assert "1352000 bytes" in msg and "SNPM_IBD_BITS_MB" in msg and "1048576" in msg, msg
    _same({k: z[k] for k in ALL}, twin.ibd_counts(snps, small, 5, 1000, 1), "the call that fits")


def test_command_end_to_end_on_the_planted_panel(ctx, tmp_path):
    case = twin.planted_case()
    db, genome, out = str(tmp_path / "db.npz"), str(tmp_path / "two_chromosomes.json"), str(tmp_path / "out")
    np.savez(db, snps=case["snps"], accessions=case["names"], positions=case["positions"], chrs=case["chrs"], chr_regions=case["chr_regions"])
    with open(genome, "w") as fh:
        json.dump(case["genome"], fh)
    assert cli.main(["ibd", "-d", db, "--genome", genome, "-b", str(twin.PLANTED_BIN), "--min_run", "3", "-o", out]) == 0
    segs = [ln.split("\t") for ln in open(out + ".ibd.segments.tsv").read().splitlines()][1:]
    want_pairs = sorted(twin.PLANTED_RUNS, key=lambda ab: -sum(r[3] for r in twin.PLANTED_RUNS[ab]))
    assert segs == [["acc%02d" % a, "acc%02d" % b, "Chr%d" % (c + 1), str(1 + 1000 * lo), str(1000 * (hi + 1)), str(hi - lo + 1), str(k)]
                    for a, b in want_pairs for c, lo, hi, k in twin.PLANTED_RUNS[(a, b)]]
    z = np.load(out + ".ibd.npz")
    per_chr = [twin.ibd_counts(case["snps"], np.arange(0, hi - lo + 1, 100), 20, 1000, 3, rows=range(lo, hi)) for lo, hi in ((0, 1800), (1800, 3000))]
    for k in NAMES:
        assert np.array_equal(z[k], np.maximum(per_chr[0][k], per_chr[1][k]) if k == "run_max" else per_chr[0][k] + per_chr[1][k]), k
    for c, chrom in enumerate(("Chr1", "Chr2")):
        assert np.array_equal(z["used_bits_" + chrom], per_chr[c]["used_bits"]) and np.array_equal(z["shared_bits_" + chrom], per_chr[c]["shared_bits"])
    stats = json.load(open(out + ".ibd.json"))
    assert stats["pairs_with_a_run"] == 3 and stats["longest_run"]["shared_windows"] == 10 and stats["windows_per_chr"] == {"Chr1": 18, "Chr2": 12}
