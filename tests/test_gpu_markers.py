"""markers on the device: ``snpm_panel_marker_select`` / ``k_mk_rowplanes`` + ``k_mk_gain`` + ``k_mk_pick`` + ``k_mk_update`` against the
numpy twin (tests/markers_twin.py): every returned array by integer equality, on panels filled through the normal upload path in
each of the three layouts (int8, packed whole rows, packed split rows), at the shapes where the decomposition could break: 64
accessions per bit word and ballot, 64 rows, the row group of a gain block, the host's batches of rounds; against another device
call; and the ``markers`` command end to end on the planted panel."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import markers_twin as twin
import test_markers_cpu as cpu
from snpmatch_amd import cli, engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = ["int8", "packed", "split"]


def _kernel_constant(name):
    """a ``constexpr int`` of csrc/snpm_k_mk.hpp"""
    text = open(os.path.join(os.path.dirname(os.path.abspath(engine.__file__)), "csrc", "snpm_k_mk.hpp")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


GROUP = _kernel_constant("MK_GAIN_ROWS")          # rows of a k_mk_gain block
BATCH = _kernel_constant("MK_ROUND_BATCH")        # rounds the host enqueues between two reads of the state


@pytest.fixture(scope="module")
def ctx():
    return engine.default_context()


def _calls(rng, n_rows, n_acc, other=False):
    """45 % ref, 35 % alt, 10 % missing, 7 % het (int8 panels: 3 % of them the "other" code)"""
    u = rng.random((n_rows, n_acc))
    v = np.where(u < 0.45, 0, np.where(u < 0.80, 1, np.where(u < 0.90, -1, 2))).astype(np.int8)
    if other:
        v[u > 0.97] = 3
    return v


def _panel(ctx, snps, layout, monkeypatch):
    """the normal upload path; packed panels are split (main part + ragged tail) wherever that saves memory, SNPM_PACKED_SPLIT=0
    keeps whole rows"""
    if layout == "packed":
        monkeypatch.setenv("SNPM_PACKED_SPLIT", "0")
    panel = engine.Panel.from_host(ctx, snps, packed=layout != "int8")
    monkeypatch.delenv("SNPM_PACKED_SPLIT", raising=False)
    return panel


def _check(panel, snps, **kw):
    got, want = engine.marker_select(panel, **kw), twin.marker_select(snps, **kw)
    for k in twin.KEYS:
        g, w = got[k], want[k]
        if isinstance(w, np.ndarray):
            assert g.dtype == w.dtype and g.shape == w.shape, (k, kw)
            assert np.array_equal(g, w), "%s differs in %d entries (%r)" % (k, int((g != w).sum()), kw)
        else:
            assert g == w, (k, g, w, kw)
    return got


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n_acc", [1, 2, 63, 64, 65, 130])
def test_edges_of_the_accession_words_and_of_the_row_groups(n_acc, layout, ctx, monkeypatch):
    rng = np.random.default_rng(1000 + n_acc)
    snps = _calls(rng, 75, n_acc, other=layout == "int8")
    assert layout != "int8" or n_acc < 63 or (snps == 3).any()
    panel = _panel(ctx, snps, layout, monkeypatch)
    for k, n_rows in enumerate((1, 63, 64, 65, GROUP - 1, GROUP, GROUP + 1)):
        _check(panel, snps, depth=(1, 2, 3)[k % 3], rows=range(5, 5 + n_rows))
    got = _check(panel, snps, depth=255, rows=range(5, 75))                       # need never reaches 0: every row with gain is picked once
    if n_acc >= 2:
        assert got["stop_reason"] == 2 and got["n_chosen"] == np.count_nonzero(got["first_gain"]) and (got["need"][~np.eye(n_acc, dtype=bool)] > 0).all()
    _check(panel, snps)                                                           # cols and rows NULL: the whole panel
    panel.free()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_row_and_column_lists_with_repeats(layout, ctx, monkeypatch):
    rng = np.random.default_rng(2000)
    snps = _calls(rng, 300, 70, other=layout == "int8")
    panel = _panel(ctx, snps, layout, monkeypatch)
    rows = rng.integers(0, 300, size=90).astype(np.int64)                         # shuffled, with repeats
    rows[-1] = rows[0]
    cols = rng.permutation(70)[:41].astype(np.int32)
    cols[7] = cols[-1] = 11                                                       # a repeated column: a pair nothing separates
    for depth in (1, 2, 3):
        got = _check(panel, snps, depth=depth, rows=rows, cols=cols)
        assert got["need"][7, 40] == got["need"][40, 7] == depth and got["stop_reason"] == 2
    _check(panel, snps, depth=2, rows=rows)
    _check(panel, snps, cols=cols, rows=range(5, 205), first_gain=False)
    with pytest.raises(AssertionError, match="accession index outside the panel"):
        engine.marker_select(panel, cols=np.array([0, 70], dtype=np.int32))
    with pytest.raises(AssertionError, match="row index outside the panel"):
        engine.marker_select(panel, rows=np.array([0, 300], dtype=np.int64))
    with pytest.raises(AssertionError, match="depth must lie in 1 .. 255"):
        engine.marker_select(panel, depth=256)
    with pytest.raises(AssertionError, match="min_dist needs coord"):
        engine.marker_select(panel, min_dist=3)
    panel.free()


def _seed_with(rounds, reason, n_acc=24, n_rows=40):
    """the first seed whose panel makes the loop end with ``reason`` in exactly ``rounds`` rounds -- a round that ends the loop for
    lack of gain makes no pick, the round of the last pick ends it otherwise -- found with the twin.  For reason 2 the last column
    is a copy of the first: that pair is never resolved, so the loop runs until no row has a gain."""
    for seed in range(3000):
        snps = _calls(np.random.default_rng(seed), n_rows, n_acc)
        if reason == 2:
            snps[:, -1] = snps[:, 0]
        got = twin.marker_select(snps, first_gain=False)
        if got["stop_reason"] == reason and got["n_chosen"] + (reason == 2) == rounds:
            return snps, got
    raise AssertionError("no seed gives %d rounds with reason %d" % (rounds, reason))


def test_max_markers_and_the_ends_of_a_batch_of_rounds(ctx, monkeypatch):
    """the end of the loop in the middle of a batch, on its last round and on the first round of the next -- by the last pick (all
    resolved) and by a round without gain -- and max_markers 1, exactly the picks needed, more"""
    ctx.profile(True)
    for reason in (0, 2):
        for rounds in (BATCH - 1, BATCH, BATCH + 1):
            snps, want = _seed_with(rounds, reason)
            panel = _panel(ctx, snps, LAYOUTS[rounds % 3], monkeypatch)
            ctx.profile_reset()
            got = _check(panel, snps)
            assert got["stop_reason"] == reason and got["n_chosen"] == want["n_chosen"]
            # whole batches are enqueued, as far as min(max_markers, n_rows) goes; the rounds behind the end return at once
            enqueued = min(len(snps), -(-rounds // BATCH) * BATCH)
            assert [ctx.profile_read(k)[0] for k in ("mk_planes", "mk_gain", "mk_pick", "mk_update")] == [1, enqueued, enqueued, enqueued + 1]
            n = want["n_chosen"]
            for max_markers in (1, n - 1, n, n + 1, 10 ** 6):
                limited = _check(panel, snps, max_markers=max_markers)
                assert limited["n_chosen"] == min(n, max_markers) and limited["stop_reason"] == (reason if max_markers > n or (reason == 0 and max_markers == n) else 1)
            assert _check(panel, snps, max_markers=0)["stop_reason"] == 1
            panel.free()
    ctx.profile(False)


def test_eligibility_masks_distances_and_duplicate_rows(ctx, monkeypatch):
    rng = np.random.default_rng(4000)
    snps = _calls(rng, 120, 40, other=True)
    panel = _panel(ctx, snps, "int8", monkeypatch)
    free = _check(panel, snps)
    mask = np.ones(120, dtype=np.uint8)
    mask[free["chosen"][0]] = 0                                                   # forbid the best row
    masked = _check(panel, snps, eligible=mask)
    assert free["chosen"][0] not in masked["chosen"] and np.array_equal(masked["first_gain"], free["first_gain"])
    mask = (rng.random(120) < 0.5).astype(np.uint8) * 200                         # any non-zero byte is "eligible"
    masked = _check(panel, snps, eligible=mask, depth=2)
    assert mask[masked["chosen"]].all()
    assert _check(panel, snps, eligible=np.zeros(120, dtype=np.uint8))["stop_reason"] == 2
    coord = rng.integers(0, 1000, size=120)
    one = _check(panel, snps, coord=coord, min_dist=1001)                         # larger than the whole range: exactly one pick
    assert one["n_chosen"] == 1 and one["stop_reason"] == 2
    assert twin.same(_check(panel, snps, coord=coord, min_dist=0), free)
    spaced = _check(panel, snps, coord=coord, min_dist=25, depth=2)
    picked = np.sort(coord[spaced["chosen"]])
    assert spaced["n_chosen"] > 3 and (np.diff(picked) >= 25).all()
    twice = np.repeat(np.arange(60), 2)[rng.permutation(120)]                     # every coordinate twice, min_dist 1: one of each two at most
    got = _check(panel, snps, coord=twice, min_dist=1, depth=3)
    assert len(set(twice[got["chosen"]].tolist())) == got["n_chosen"] > 3
    far = np.array([np.iinfo(np.int64).min, np.iinfo(np.int64).max] * 60)         # the distance is exact for any two int64 values
    _check(panel, snps, coord=far, min_dist=2 ** 62, depth=2)
    # duplicate rows: at depth 1 the second copy has no gain after the first pick; at depth 2 it is picked
    rows = np.repeat(np.arange(10, 40), 2)
    d1, d2 = _check(panel, snps, rows=rows, depth=1), _check(panel, snps, rows=rows, depth=2)
    assert len(set(rows[d1["chosen"]].tolist())) == d1["n_chosen"] and d1["chosen"][0] % 2 == 0
    assert d2["chosen"][:2].tolist() == [d1["chosen"][0], d1["chosen"][0] + 1] and d2["gain_at"][0] == d2["gain_at"][1]
    panel.free()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_degenerate_panels(layout, ctx, monkeypatch):
    for fill in (-1, 1):                                                          # all missing; all one allele
        snps = np.full((70, 65), fill, dtype=np.int8)
        panel = _panel(ctx, snps, layout, monkeypatch)
        got = _check(panel, snps, depth=2)
        assert (got["n_chosen"], got["stop_reason"], got["remaining"]) == (0, 2, 2 * 65 * 32) and not got["first_gain"].any()
        panel.free()
    snps = _calls(np.random.default_rng(5000), 70, 65)
    snps[:, 64] = snps[:, 3]                                                      # two identical columns, in different bit words
    panel = _panel(ctx, snps, layout, monkeypatch)
    got = _check(panel, snps)
    assert np.argwhere(np.triu(got["need"])).tolist() == [[3, 64]] and got["stop_reason"] == 2 and got["remaining"] == 1
    empty = engine.marker_select(panel, cols=np.array([2], dtype=np.int32))       # fewer than two columns: nothing launched
    assert (empty["n_chosen"], empty["remaining"], empty["stop_reason"]) == (0, 0, 0) and empty["need"].tolist() == [[0]] and not empty["first_gain"].any()
    _check(panel, snps, rows=range(7, 7))
    _check(panel, snps, cols=np.zeros(0, dtype=np.int32))
    panel.free()


def test_workspace_reuse_and_first_gain_against_kinship_counts(ctx, monkeypatch):
    rng = np.random.default_rng(6000)
    big = _calls(rng, 1500, 1135)
    panel = _panel(ctx, big, "split", monkeypatch)
    assert panel.pitch == 256 + 32                      # main part + tail: the split layout exists at this width
    rows = np.sort(rng.choice(1500, size=900, replace=False)).astype(np.int64)
    first = _check(panel, big, rows=rows, max_markers=12)
    again = engine.marker_select(panel, rows=rows, max_markers=12)                # the same call twice: the state and the workspaces are reset
    assert twin.same(again, first) and first["n_chosen"] == 12 and first["stop_reason"] == 1
    # another device call against this one: a row's first gain is the pairs it separates, so the sum is the sum of diff over a < b
    _, _, diff = engine.kinship_counts(panel, rows=rows)
    assert int(first["first_gain"].astype(np.int64).sum()) == int(np.triu(diff.astype(np.int64), 1).sum())
    small = _calls(rng, 40, 9)
    other = _panel(ctx, small, "int8", monkeypatch)
    _check(other, small, depth=2)                                                 # a small call after a large one on the same context
    cols = rng.permutation(1135)[:100].astype(np.int32)
    sub = _check(panel, big, cols=cols, rows=range(100, 400), depth=2)
    _, _, diff = engine.kinship_counts(panel, cols=cols, rows=range(100, 400))
    assert int(sub["first_gain"].astype(np.int64).sum()) == int(np.triu(diff.astype(np.int64), 1).sum())
    other.free()
    panel.free()


def test_planes_over_the_budget_are_refused_with_both_figures(tmp_path):
    """SNPM_MK_WS_MB=1 in a fresh child process: 70 000 rows x 64 accessions are 1 120 000 bytes of row planes, more than 1 MiB;
    65 536 rows fit exactly"""
    snps = _calls(np.random.default_rng(7000), 70000, 64)
    np.savez(tmp_path / "in.npz", snps=snps, fit=np.array(65536))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "markers_ws_worker.py"), str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       capture_output=True, text=True, env=dict(os.environ, SNPM_MK_WS_MB="1"), timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    z = np.load(tmp_path / "out.npz")
    msg = str(z["message"])
    assert "1120000 bytes" in msg and "70000 candidate rows" in msg and "SNPM_MK_WS_MB" in msg and "1048576" in msg and "thin the candidates" in msg, msg
    want = twin.marker_select(snps, max_markers=5, rows=range(0, 65536))
    assert twin.same({k: (z[k] if z[k].shape else z[k].item()) for k in twin.KEYS}, want)


def test_command_end_to_end_on_the_planted_panel(ctx, tmp_path):
    case = twin.planted_case()
    db, out, sites = str(tmp_path / "db.npz"), str(tmp_path / "out"), str(tmp_path / "x.sites.tsv")
    np.savez(db, snps=case["snps"], accessions=case["names"], positions=case["positions"], chrs=case["chrs"], chr_regions=case["chr_regions"])
    cpu.write_sites(case, sites, set(twin.PLANTED_HIDDEN_ROWS))
    assert cli.main(["markers", "-d", db, "--sites", sites, "--depth", "2", "-o", out]) == 0
    stats, z = cpu.check_planted_outputs(case, out, 2)
    keep = np.array([r for r in range(600) if r not in twin.PLANTED_HIDDEN_ROWS])
    want = twin.marker_select(case["snps"], 2, rows=keep)
    assert np.array_equal(z["chosen"], want["chosen"]) and np.array_equal(z["gain_at"], want["gain_at"]) and np.array_equal(z["need"], want["need"])
    assert cli.main(["markers", "-d", db, "--min_dist_bp", "5000", "--max_markers", "20", "-o", out]) == 0
    from snpmatch_amd.core import markers
    lines = [ln.split("\t") for ln in open(out + ".markers.tsv").read().splitlines()][1:]
    holder = cpu._Holder(None)
    holder.g = type("G", (), {"chr_regions": case["chr_regions"], "positions": case["positions"]})()
    want = twin.marker_select(case["snps"], 1, 20, markers.coordinates(holder, np.arange(600), 5000), 5000)
    assert [int(ln[2]) for ln in lines] == case["positions"][want["chosen"]].tolist() and 1 < len(lines) == want["n_chosen"] <= 20
