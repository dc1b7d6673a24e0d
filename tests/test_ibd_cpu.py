"""ibd without a GPU: the numpy twin (tests/ibd_twin.py) tied to the goldens of the unmodified reference through the twins of
``kinship`` (one window over all rows: n = same + diff, d = diff) and ``windows`` (per window: n = hom_same + hom_diff, d = hom_diff),
and on a hand-made matrix with every state and run written out; ``core.ibd.runs_from_bits`` against the twin; every refusal of
``snpm_panel_ibd_counts`` that needs no device; the ``ibd`` subcommand with the twin in the place of the device on a planted panel
whose three shared stretches it must report exactly; and the kernel source and the host's plan functions themselves, compiled for
the host and run by 256 real threads per block under AddressSanitizer + UBSan (tests/ibd_host_driver.cpp on tests/host_kernel/, a
child process)."""
import glob
import json
import os

import numpy as np
import pytest

import host_kernel_util
import ibd_twin as twin
import kinship_twin
import windows_twin
from snpmatch_amd import _lib, cli, engine
from snpmatch_amd.core import ibd, snp_genotype

NAMES = ("w_used", "w_shared", "n_shared", "d_shared", "run_max", "n_runs", "w_in_runs")
ALL = NAMES + ("used_bits", "shared_bits")


def same(got, want):
    return all(np.array_equal(got[k], want[k]) and got[k].dtype == want[k].dtype for k in ALL)


# ------------------------------------------------------------------------------------------------ the twin
def test_one_window_is_same_plus_diff_and_diff_of_the_kinship_goldens(golden_dir):
    paths = sorted(glob.glob(os.path.join(golden_dir, "kinship_a[127]_r*.npz")))
    assert len(paths) == 15
    for path in paths:
        snps = np.load(path)["snps"]
        _, same_, diff = kinship_twin.kinship_counts(snps)
        n, d = twin.window_counts(snps, [0, len(snps)])
        assert np.array_equal(n[0], same_.astype(np.int64) + diff) and np.array_equal(d[0], diff)
        got = twin.ibd_counts(snps, [0, len(snps)], 1, twin.PPM, 1)
        assert np.array_equal(got["n_shared"], same_ + diff) and np.array_equal(got["d_shared"], diff)
        assert np.array_equal(got["w_used"], (same_ + diff > 0).astype(np.int32)) and np.array_equal(got["run_max"], got["w_used"])


@pytest.mark.parametrize("name", ["windows_a2_w100", "windows_a2_w300", "windows_a7_w100", "windows_a7_w300"])
def test_per_window_is_hom_same_plus_hom_diff_and_hom_diff_of_the_windows_twin(name, golden_dir):
    case = np.load(os.path.join(golden_dir, name + ".npz"))
    snps, first, last = case["snps"], case["first"], case["last"]
    assert set(np.unique(snps).tolist()) == {-1, 0, 1, 2, 3}
    rows = np.concatenate([np.arange(a, b) for a, b in zip(first, last)])
    win_off = np.concatenate([[0], np.cumsum(last - first)])
    k = snps.shape[1]
    pairs = np.array([(a, b) for a in range(k) for b in range(k)])
    _, cells = windows_twin.window_counts(snps, win_off, None, pairs, rows)
    n, d = twin.window_counts(snps, win_off, None, rows)
    assert np.array_equal(n.reshape(len(win_off) - 1, -1).T, cells[:, :, 2].astype(np.int64) + cells[:, :, 3])
    assert np.array_equal(d.reshape(len(win_off) - 1, -1).T, cells[:, :, 3])
    for a, b in ((0, 1), (1, 0), (k - 1, k - 1)):
        assert np.array_equal(twin.pair_windows(snps, win_off, a, b, None, rows), np.stack([n[:, a, b], d[:, a, b]], axis=1))


# A against B, window by window (min_win_sites 4, max_diff_ppm 250 000, min_run 2):
#   0: n 4, d 1: 1 * 1 000 000 == 250 000 * 4 exactly -> shared; n == min_win_sites
#   1: n 3 == min_win_sites - 1 (the fourth row is a het of A): unused, inside the run
#   2: n 4, d 0: shared -- the run 0 .. 2 spans three windows and holds two shared ones: exactly min_run
#   3: n 4, d 2: a break
#   4: n 5, d 1: shared -- a run of one: exactly min_run - 1
#   5: n 4, d 4: a break                      6: empty
#   7: n 4, d 0 among four more rows that count nowhere (het with het, code 3 on either side, a missing call): shared
#   8: n 4, d 0: shared -- the run 7 .. 8 is still open at the end
HAND_A = [0, 1, 0, 0,   0, 1, 1, 2,   0, 1, 1, 0,   0, 1, 0, 1,   0, 1, 0, 1, 1,   0, 0, 1, 1,   0, 2, 3, 1, -1, 0, 1, 0,   1, 1, 0, 0]
HAND_B = [0, 1, 0, 1,   0, 1, 1, 0,   0, 1, 1, 0,   1, 0, 0, 1,   0, 1, 0, 1, 0,   1, 1, 0, 0,   0, 2, 0, 1, 1, 0, 1, 3,    1, 1, 0, 0]
HAND_OFF = [0, 4, 8, 12, 16, 21, 25, 25, 33, 37]
# C is A with every third row an "other" code (even rows) or a het (odd rows)
HAND_C = [(3 if r % 2 == 0 else 2) if r % 3 == 0 else a for r, a in enumerate(HAND_A)]


def test_twin_on_a_hand_made_matrix():
    snps = np.array([HAND_A, HAND_B, HAND_C], dtype=np.int8).T
    off = np.array(HAND_OFF)
    assert len(HAND_A) == len(HAND_B) == 37 and set(HAND_C) == {-1, 0, 1, 2, 3}
    assert twin.pair_windows(snps, off, 0, 1).tolist() == [[4, 1], [3, 0], [4, 0], [4, 2], [5, 1], [4, 4], [0, 0], [4, 0], [4, 0]]
    n, d = twin.window_counts(snps, off)
    assert np.array_equal(np.stack([n[:, 0, 1], d[:, 0, 1]], axis=1), twin.pair_windows(snps, off, 0, 1))
    used, shared = twin.states(n[:, 0, 1], d[:, 0, 1], 4, 250000)
    assert used.tolist() == [True, False, True, True, True, True, False, True, True]
    assert shared.tolist() == [True, False, True, False, True, False, False, True, True]
    assert twin.runs_of(used, shared, 1) == [(0, 2, 2), (4, 4, 1), (7, 8, 2)] and twin.runs_of(used, shared, 2) == [(0, 2, 2), (7, 8, 2)]
    assert twin.runs_of(used, shared, 3) == []

    def cell(got, a, b):
        return tuple(int(got[k][a, b]) for k in NAMES)
    got = twin.ibd_counts(snps, off, 4, 250000, 2)
    #                               w_used w_shared n_shared d_shared run_max n_runs w_in_runs
    assert cell(got, 0, 1) == cell(got, 1, 0) == (7, 5, 21, 2, 2, 2, 4)
    assert got["used_bits"][0, 1].tolist() == [0b110111101] and got["shared_bits"][0, 1].tolist() == [0b110010101]
    assert cell(twin.ibd_counts(snps, off, 4, 250000, 1), 0, 1) == (7, 5, 21, 2, 2, 3, 5)
    assert cell(twin.ibd_counts(snps, off, 4, 250000, 3), 0, 1) == (7, 5, 21, 2, 2, 0, 0)          # run_max does not depend on min_run
    # one site fewer per window: window 1 is used and shared as well, the first run holds three
    assert cell(twin.ibd_counts(snps, off, 3, 250000, 2), 0, 1) == (8, 6, 24, 2, 3, 2, 5)
    # a threshold just below window 0's share: 1 * 1 000 000 > 249 999 * 4, a break; window 4 (1 of 5) stays shared
    assert cell(twin.ibd_counts(snps, off, 4, 249999, 1), 0, 1) == (7, 4, 17, 1, 2, 3, 4)
    # max_diff_ppm 0: only windows without a difference are shared -- 2, 7, 8; 1 000 000: every used window, one run of seven
    assert cell(twin.ibd_counts(snps, off, 4, 0, 2), 0, 1) == (7, 3, 12, 0, 2, 1, 2)
    assert cell(twin.ibd_counts(snps, off, 4, twin.PPM, 2), 0, 1) == (7, 7, 29, 8, 7, 1, 7)
    # the diagonal: d = 0, every used window is shared; a het, a code 3 and a missing call of the column itself count nowhere
    assert cell(got, 0, 0) == (7, 7, 30, 0, 7, 1, 7) and cell(got, 1, 1) == (8, 8, 35, 0, 8, 1, 8)
    assert np.array_equal(np.diagonal(got["used_bits"]), np.diagonal(got["shared_bits"]))
    # C: rows 0 and 3 of window 0 are a code 3 and a het, two sites remain: unused at 4, shared at 2
    assert twin.pair_windows(snps, off, 0, 2)[0].tolist() == [2, 0] and cell(twin.ibd_counts(snps, off, 2, 0, 1), 0, 2)[:2] == (8, 8)
    # a repeated column: positions 0 and 2 are both A -- their cell is A's diagonal, and B against either is the same cell
    rep = twin.ibd_counts(snps, off, 4, 250000, 2, cols=[0, 1, 0])
    assert cell(rep, 0, 2) == cell(rep, 2, 0) == cell(got, 0, 0) and cell(rep, 1, 2) == cell(rep, 1, 0) == cell(got, 0, 1)
    assert np.array_equal(rep["shared_bits"][1, 2], got["shared_bits"][0, 1])
    for args in ((4, 250000, 2), (1, 0, 1), (3, twin.PPM, 3), (2, 400000, 1)):
        both = twin.ibd_counts(snps, off, *args), twin.ibd_counts_direct(snps, off, *args)
        assert same(*both) and all(np.array_equal(both[0][k], np.swapaxes(both[0][k], 0, 1)) for k in ALL)
        assert all(both[0][k].dtype == np.int32 for k in NAMES) and both[0]["used_bits"].dtype == np.uint32
    # a row list with repeats and a range select the same way
    assert same(twin.ibd_counts(snps, [0, 5, 9], 1, 0, 1, rows=np.array([3, 3, 8, 1, 0, 36, 36, 2, 9])),
                twin.ibd_counts(snps[[3, 3, 8, 1, 0, 36, 36, 2, 9]], [0, 5, 9], 1, 0, 1))
    assert same(twin.ibd_counts(snps, [0, 5, 9], 1, 0, 1, rows=range(4, 13)), twin.ibd_counts(snps[4:13], [0, 5, 9], 1, 0, 1))


@pytest.mark.parametrize("n_win", [31, 32, 33, 64, 65])
def test_runs_from_bits_against_the_twin(n_win):
    rng = np.random.default_rng(100 + n_win)
    for trial in range(40):
        used = rng.random(n_win) < (0.2, 0.7, 1.0)[trial % 3]
        shared = used & (rng.random(n_win) < (0.5, 0.9)[trial % 2])
        if trial == 0:
            used[:], shared[:] = True, True                         # one run through every bit word
        ub, sb = twin.pack_bits(used), twin.pack_bits(shared)
        assert ub.shape == ((n_win + 31) // 32,) and np.array_equal(ibd.unpack_bits(ub, n_win), used)
        for min_run in (1, 2, 3, n_win):
            got = ibd.runs_from_bits(ub, sb, min_run)
            assert got.dtype == np.int64 and got.shape[1] == 3 and [tuple(r) for r in got.tolist()] == twin.runs_of(used, shared, min_run)
    assert ibd.runs_from_bits(np.zeros(2, dtype=np.uint32), np.zeros(2, dtype=np.uint32)).shape == (0, 3)


# ------------------------------------------------------------------------------------------------ the library's validation
def test_refusals_that_need_no_device():
    lib = _lib.load()
    out = np.zeros((7, 2, 2), dtype=np.int32)
    bits = np.zeros((2, 2, 2, 1), dtype=np.uint32)
    cols = np.zeros(2, dtype=np.int32)
    off5 = np.array([0, 2, 2, 5], dtype=np.int64)

    def call(ncols, n_rows, outs=tuple(range(7)), cols=cols, off=off5, n_win=3, min_sites=1, ppm=1000, min_run=1, with_bits=True):
        ptrs = [_lib.ptr(out[k]) if k is not None else None for k in outs] + [_lib.ptr(bits[k]) if with_bits else None for k in range(2)]
        rc = lib.snpm_panel_ibd_counts(None, _lib.ptr(cols), ncols, None, 0, n_rows, _lib.ptr(off), n_win, min_sites, ppm, min_run, *ptrs)
        return rc, lib.snpm_last_error(None).decode()
    bad = _lib.SNPM_ERR_BADARG
    assert call(-1, 5) == (bad, "negative size") and call(2, -1) == (bad, "negative size")
    assert call(2, 5, n_win=-1) == (bad, "negative number of windows")
    for m in (0, -3):
        assert call(2, 5, min_sites=m) == (bad, "min_win_sites must be 1 or more")
        assert call(2, 5, min_run=m) == (bad, "min_run must be 1 or more")
    for ppm in (-1, 1000001, 2 ** 31 - 1):
        assert call(2, 5, ppm=ppm) == (bad, "max_diff_ppm must lie in 0 .. 1000000")
    rc, msg = call(11553, 5)
    assert rc == bad and "too many accessions" in msg and "SNPM_F1X_MAX_ACCESSIONS" in msg
    rc, msg = call(2, 2 ** 31)
    assert rc == bad and "2^31 rows" in msg
    assert call(2, 5, off=None) == (bad, "win_off is NULL")
    assert call(2, 5, off=np.array([1, 2, 2, 5], dtype=np.int64)) == (bad, "win_off must start at 0")
    assert call(2, 5, off=np.array([0, 3, 2, 5], dtype=np.int64)) == (bad, "win_off must not decrease")
    assert call(2, 5, off=np.array([0, 2, 2, 4], dtype=np.int64)) == (bad, "win_off must end at n")
    assert call(2, 5, n_win=0) == (bad, "win_off must end at n")                 # no window, but rows
    for k in range(7):
        outs = tuple(None if j == k else j for j in range(7))
        assert call(2, 5, outs) == (bad, "w_used / w_shared / n_shared / d_shared / run_max / n_runs / w_in_runs is NULL")
    # sound arguments: only the panel is missing -- the extremes of the three parameters, no bitsets, nothing to write
    assert call(2, 5) == (bad, "panel is NULL") and call(2, 5, with_bits=False) == (bad, "panel is NULL")
    assert call(2, 5, ppm=0) == (bad, "panel is NULL") and call(2, 5, ppm=1000000, min_sites=2 ** 31 - 1, min_run=2 ** 31 - 1) == (bad, "panel is NULL")
    assert call(0, 5, (None,) * 7, with_bits=False) == (bad, "panel is NULL")
    assert call(2, 0, off=np.zeros(1, dtype=np.int64), n_win=0) == (bad, "panel is NULL")
    assert call(2, 0, off=np.zeros(3, dtype=np.int64), n_win=2) == (bad, "panel is NULL")      # empty windows only
    assert call(11552, 5, cols=None) == (bad, "panel is NULL")                    # the limit is inclusive
    assert "snpm_panel_ibd_counts" in _lib.SYMBOLS


class _Holder(object):
    """stands in for a Genotype whose DB went to the given kind of panel"""

    def __init__(self, panel):
        self._panel = panel

    def panel(self):
        return self._panel


def test_group_and_streamed_panels_are_refused_with_the_reason():
    off = np.array([0, 3])
    for cls, why in ((engine.GroupPanel, "spread over several GPUs"), (engine.StreamedPanel, "not a resident panel")):
        with pytest.raises(TypeError, match="ibd_counts needs every accession column on one device") as err:
            engine.ibd_counts(cls.__new__(cls), off)
        assert why in str(err.value)
    for cls, why in ((engine.GroupPanel, "spread over several GPUs by accession"), (engine.StreamedPanel, "streamed through the device")):
        with pytest.raises(TypeError, match="the shared-segment scan needs every accession column of the DB on one device") as err:
            snp_genotype.Genotype.ibd_counts(_Holder(cls.__new__(cls)), off)
        assert why in str(err.value)


# ------------------------------------------------------------------------------------------------ the command
@pytest.fixture
def planted(monkeypatch, tmp_path):
    """the planted DB as an .npz and the genome as a JSON file; the device call is the twin"""
    case = twin.planted_case()
    snps = case["snps"]
    db = str(tmp_path / "db.npz")
    np.savez(db, snps=snps, accessions=case["names"], positions=case["positions"], chrs=case["chrs"], chr_regions=case["chr_regions"])
    genome = str(tmp_path / "two_chromosomes.json")
    with open(genome, "w") as fh:
        json.dump(case["genome"], fh)
    calls = []
    stub = engine.Panel.__new__(engine.Panel)
    stub.h = None

    def device(panel, win_off, min_win_sites=20, max_diff_ppm=1000, min_run=1, cols=None, rows=None, bits=True):
        calls.append((cols, rows, np.asarray(win_off).copy(), min_win_sites, max_diff_ppm, min_run))
        return twin.ibd_counts(snps, win_off, min_win_sites, max_diff_ppm, min_run, cols, rows)
    monkeypatch.setattr(snp_genotype.Genotype, "panel", lambda self, ctx=None, packed=None: stub)
    monkeypatch.setattr(engine, "ibd_counts", device)
    return case, db, genome, calls


def _tsv(path):
    return [ln.split("\t") for ln in open(path).read().splitlines()]


def test_command_reports_exactly_the_planted_segments(planted, tmp_path):
    case, db, genome, calls = planted
    snps, win_off, win_chr = case["snps"], case["win_off"], case["win_chr"]
    assert snps.shape == (3000, 40) and len(win_off) - 1 == 30 and twin.PLANTED_SEED == 31
    # other pairs differ at about 30 % of the rows where both are homozygous
    n, d = twin.window_counts(snps, [0, len(snps)])
    decoys = np.triu(np.ones((40, 40), dtype=bool), 1)
    for a, b, _, _, _ in twin.PLANTED_COPIES:
        decoys[a, b] = False
    share = d[0][decoys] / n[0][decoys]
    assert abs(share.mean() - 0.30) < 0.005 and 0.25 < share.min() and share.max() < 0.35      # (about 2650 rows per pair: one standard deviation is 0.009)
    out = str(tmp_path / "out")
    assert cli.main(["ibd", "-d", db, "--genome", genome, "-b", str(twin.PLANTED_BIN), "--min_run", "3", "-o", out]) == 0
    # one call per chromosome, its rows a range, its windows from 0
    assert len(calls) == 2 and all(c[0] is None and c[3:] == (20, 1000, 3) for c in calls)
    assert [c[1] for c in calls] == [range(0, 1800), range(1800, 3000)]
    assert np.array_equal(calls[0][2], np.arange(0, 1801, 100)) and np.array_equal(calls[1][2], np.arange(0, 1201, 100))
    name = "acc%02d"
    want_pairs = sorted(twin.PLANTED_RUNS, key=lambda ab: -sum(r[3] for r in twin.PLANTED_RUNS[ab]))
    assert want_pairs == [(3, 17), (8, 21), (5, 30)]
    segs = _tsv(out + ".ibd.segments.tsv")
    assert segs[0] == ["acc_1", "acc_2", "chr", "start", "end", "windows", "shared_windows"]
    want_segs = [[name % a, name % b, "Chr%d" % (c + 1), str(1 + 1000 * lo), str(1000 * (hi + 1)), str(hi - lo + 1), str(k)]
                 for a, b in want_pairs for c, lo, hi, k in twin.PLANTED_RUNS[(a, b)]]
    assert want_segs[0] == ["acc03", "acc17", "Chr1", "5001", "15000", "10", "10"] and want_segs[3] == ["acc05", "acc30", "Chr1", "10001", "17000", "7", "5"]
    assert want_segs[1:3] == [["acc08", "acc21", "Chr2", "2001", "6000", "4", "4"], ["acc08", "acc21", "Chr2", "7001", "10000", "3", "3"]]
    assert segs[1:] == want_segs                                                 # exactly those: no decoy pair has a run
    pairs = _tsv(out + ".ibd.pairs.tsv")
    assert pairs[0] == ["acc_1", "acc_2", "w_used", "w_shared", "run_max", "n_runs", "w_in_runs", "d_shared", "n_shared"]
    assert [ln[:2] + ln[4:7] for ln in pairs[1:]] == [["acc03", "acc17", "10", "1", "10"], ["acc08", "acc21", "4", "2", "7"], ["acc05", "acc30", "5", "1", "5"]]
    assert [ln[2:4] + [ln[7]] for ln in pairs[1:]] == [["30", "10", "0"], ["30", "7", "0"], ["28", "5", "0"]]
    # the matrices: the twin per chromosome, summed; run_max their maximum
    z = np.load(out + ".ibd.npz")
    per_chr = [twin.ibd_counts(snps, np.arange(0, hi - lo + 1, 100), 20, 1000, 3, rows=range(lo, hi)) for lo, hi in ((0, 1800), (1800, 3000))]
    for k in NAMES:
        want = np.maximum(per_chr[0][k], per_chr[1][k]) if k == "run_max" else per_chr[0][k] + per_chr[1][k]
        assert np.array_equal(z[k], want) and z[k].dtype == np.int32
    off_diag = ~np.eye(40, dtype=bool)
    assert (z["n_runs"][off_diag] > 0).sum() == 6 and (np.diag(z["n_runs"]) == 2).all()
    assert np.diag(z["run_max"]).tolist() == [16 if a == 30 else 18 for a in range(40)]          # the blank windows of 30 are unused, not breaks
    for c, chrom in enumerate(("Chr1", "Chr2")):
        assert np.array_equal(z["used_bits_" + chrom], per_chr[c]["used_bits"]) and np.array_equal(z["shared_bits_" + chrom], per_chr[c]["shared_bits"])
        assert z["used_bits_" + chrom].shape == (40, 40, 1) and z["used_bits_" + chrom].dtype == np.uint32
    assert z["accessions"].tolist() == case["names"].tolist() and z["win_chr"].tolist() == win_chr.tolist()
    assert z["win_start"].tolist() == [1 + 1000 * w for w in range(18)] + [1 + 1000 * w for w in range(12)] and (z["win_rows"] == 100).all()
    assert np.array_equal(z["win_end"], z["win_start"] + 999)
    # the runs read back from the bitsets are the device's figures
    for (a, b), runs in twin.PLANTED_RUNS.items():
        c = runs[0][0]
        got = ibd.runs_from_bits(z["used_bits_Chr%d" % (c + 1)][a, b], z["shared_bits_Chr%d" % (c + 1)][b, a], 3)
        assert [tuple(r) for r in got.tolist()] == [r[1:] for r in runs]
        assert (len(got), int(got[:, 2].sum()), int(got[:, 2].max())) == (z["n_runs"][a, b], z["w_in_runs"][a, b], z["run_max"][a, b])
    stats = json.load(open(out + ".ibd.json"))
    assert (stats["window_size"], stats["min_win_sites"], stats["max_diff"], stats["max_diff_ppm"], stats["min_run"]) == (1000, 20, 0.001, 1000, 3)
    assert stats["windows_per_chr"] == {"Chr1": 18, "Chr2": 12} and stats["windows"] == 30 and stats["accessions"] == 40 and stats["pairs_with_a_run"] == 3
    assert stats["longest_run"] == {"acc_1": "acc03", "acc_2": "acc17", "chr": "Chr1", "start": 5001, "end": 15000, "windows": 10, "shared_windows": 10}
    # --min_run 5 (the default) drops the two short runs of acc08 / acc21; --max_diff 0.06 heals their noisy window: one run of eight
    assert cli.main(["ibd", "-d", db, "--genome", genome, "-b", "1000", "-o", out]) == 0 and calls[-1][3:] == (20, 1000, 5)
    assert [ln[:2] for ln in _tsv(out + ".ibd.pairs.tsv")[1:]] == [["acc03", "acc17"], ["acc05", "acc30"]]
    assert cli.main(["ibd", "-d", db, "--genome", genome, "-b", "1000", "--max_diff", "0.06", "-o", out]) == 0 and calls[-1][3:] == (20, 60000, 5)
    assert _tsv(out + ".ibd.segments.tsv")[2] == ["acc08", "acc21", "Chr2", "2001", "10000", "8", "8"]
    # an accession list in another order: the pair is named by the list's order
    acc_file = tmp_path / "accs.txt"
    acc_file.write_text("acc17\nacc21\nacc03\nacc08\n")
    assert cli.main(["ibd", "-d", db, "--genome", genome, "-b", "1000", "-a", str(acc_file), "--min_run", "3", "--min_win_sites", "30", "-o", out]) == 0
    assert calls[-1][0].tolist() == [17, 21, 3, 8] and calls[-1][3:] == (30, 1000, 3)
    assert [ln[:3] for ln in _tsv(out + ".ibd.segments.tsv")[1:]] == [["acc17", "acc03", "Chr1"], ["acc21", "acc08", "Chr2"], ["acc21", "acc08", "Chr2"]]
    # bad arguments: exit code 2, the device is not asked
    asked = len(calls)
    for bad in (["--max_diff", "1.5"], ["--max_diff", "-0.1"], ["--max_diff", "nan"], ["--min_run", "0"], ["--min_win_sites", "0"], ["-b", "0"]):
        assert cli.main(["ibd", "-d", db, "--genome", genome, "-o", out] + bad) == 2
    assert len(calls) == asked and ibd.potatoIBD.__doc__


# ------------------------------------------------------------------------------------------------ the kernels and the plan, on the host
def test_kernel_source_and_plan_on_the_host_under_asan_and_ubsan(tmp_path):
    """every block of k_win_planes / k_ibd_count / k_ibd_runs run by 256 real threads with a barrier, exact-size heap buffers,
    arbitrary pad bytes, stale planes, run matrices and bit workspaces: 1 / 2 / 31 / 32 / 33 / 65 accessions x 1 / 63 / 64 / 65 / 1025
    rows over the three layouts with one window, every row its own window, boundaries at 63 | 64 | 65, empty windows first, in the
    middle and last and windows of 7 rows; a window across an LDS step; a window longer than a chunk at 33 accessions; 31 / 32 / 33 /
    65 windows (the bit words fill exactly and spill by one); a group boundary inside a bit word; two and three slabs, one of a
    window larger than the budget; column lists with a repeat and unsorted row lists with a repeat (one over three slabs); the
    split layout at 1135 accessions.  The plan of every case is replayed bit by bit against the windows; the plan alone: the eight
    window sets of par_host_driver"""
    cases = host_kernel_util.run_driver("ibd_host_driver", tmp_path)
    plans = [ln for ln in cases if ln.startswith("case plan-")]
    assert len(cases) == 76 and len(plans) == 8
    assert {ln.split()[1] for ln in plans} == {"plan-bit0", "plan-bit63", "plan-many-in-a-word", "plan-empty-windows", "plan-long-window",
                                               "plan-over-budget", "plan-three-slabs", "plan-rows-own"}
    kernels = [ln for ln in cases if not ln.startswith("case plan-")]
    assert sum(" slabs=2 " in ln for ln in kernels) == 1 and sum(" slabs=3 " in ln for ln in kernels) == 3
    for acc in (1, 2, 31, 32, 33, 65):
        for rows in (1, 63, 64, 65, 1025):
            assert any(" acc=%d " % acc in ln and " rows=%d " % rows in ln for ln in kernels), (acc, rows)
    for name in ("one-window", "rows-own", "cuts-63-64-65", "empty-windows", "across-step", "bit-words"):
        assert {ln.split()[2] for ln in kernels if ln.split()[1] == name} == {"layout=0", "layout=1", "layout=2"}, name
    assert {ln.split()[6] for ln in kernels if ln.split()[1] == "bit-words"} == {"windows=31", "windows=32", "windows=33", "windows=65"}
    assert any(ln.split()[1] == "long-window" and " acc=33 " in ln and " groups=3 " in ln for ln in kernels)
    assert any(ln.split()[1] == "groups-in-a-bit-word" and " windows=5 " in ln and " groups=3 " in ln for ln in kernels)
    assert any(ln.split()[1] == "split-wide" and " acc=1135 " in ln and " layout=2 " in ln for ln in kernels)
    # both states occur: cases with shared cells off the diagonal and cases with break windows
    assert sum(" shared=0 " not in ln for ln in kernels) > 40 and sum(" breaks=0 " not in ln for ln in kernels) > 40
