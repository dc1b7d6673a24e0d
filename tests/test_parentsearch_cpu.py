"""parentsearch without a GPU: the numpy twin (tests/parentsearch_twin.py) anchored to the goldens of the unmodified reference
(``CrossIdentifier.match_insilico_f1s``: with one window over all rows hF is its score and n its numinfo less the rows without a
class), on a hand-made matrix with every count written out, and with every row its own window; every refusal of
``snpm_panel_parent_counts`` that needs no device; the ``parentsearch`` subcommand with the twin in the place of the device on a
planted F2 whose parents neither the reference's ten-best route nor the whole-genome F1 of ``f1search`` finds; and the kernel source
and the host's plan functions themselves, compiled for the host and run by 256 real threads per block under AddressSanitizer + UBSan
(tests/par_host_driver.cpp on tests/host_kernel/, a child process)."""
import json
import os

import numpy as np
import pytest

import f1search_twin
import host_kernel_util
import parentsearch_twin as twin
from oracle import snpmatch_oracle as oracle
from snpmatch_amd import _lib, cli, engine
from snpmatch_amd.core import f1search, parentsearch, snp_genotype, snpmatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFF


# ------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("n_acc", [2, 7, 10])
def test_twin_with_one_window_is_the_reference_score_and_numinfo(n_acc, golden_dir):
    case = np.load(os.path.join(golden_dir, "f1search_a%d.npz" % n_acc))
    snps, classes = case["snps"], f1search.hard_classes(case["gt"])
    assert (classes == NONE).any() and (snps == 3).any()
    win_off = np.array([0, len(snps)])
    blind = f1search_twin.f1_counts(snps[classes == NONE], np.full(int((classes == NONE).sum()), NONE, dtype=np.uint8))[1]
    score, n_tot, w_first, w_het = twin.parent_counts(snps, classes, win_off, 1)
    for a, b, want_score, want_numinfo in zip(case["pair_a"].tolist(), case["pair_b"].tolist(), case["score"].tolist(), case["numinfo"].tolist()):
        (n, ha, hb, hf), = twin.pair_windows(snps, classes, win_off, a, b).tolist()
        assert hf == want_score and n == want_numinfo - blind[a, b]
        assert n_tot[a, b] == n_tot[b, a] == n and score[a, b] == score[b, a] == (max(ha, hb, hf) if n else 0)
        assert w_first[a, b] + w_first[b, a] + w_het[a, b] == (1 if n else 0) and w_het[a, b] == (1 if n and hf > max(ha, hb) else 0)
    direct = twin.parent_counts_direct(snps, classes, win_off, 1)
    assert all(np.array_equal(x, y) for x, y in zip(direct, (score, n_tot, w_first, w_het)))


#           window 0          | 2 | window 3  | window 4                (window 1 is empty)
HAND_A = [0, 0, 1, 1,           0,  0, 1, 1,    0, 2, -1, 0, 1]
HAND_B = [0, 1, 0, 0,           1,  1, 0, 1,    1, 2, 1, 1, 0]
HAND_C = [3, 0, 3, 1,           3,  2, 0, 3,    3, 3, 1, 0, 2]
HAND_S = [0, 0, 0, 2,           2,  2, 2, 1,    1, 2, 1, NONE, 0]
HAND_OFF = [0, 4, 4, 5, 8, 13]


def test_twin_on_a_hand_made_matrix():
    snps = np.array([HAND_A, HAND_B, HAND_C], dtype=np.int8).T
    classes, win_off = np.array(HAND_S, dtype=np.uint8), np.array(HAND_OFF)
    # the pair (A, B), window by window: n, hA, hB, hF
    #   0: rows ref/ref, ref/alt, alt/ref, alt/ref under classes ref, ref, ref, het -> 4, 2, 2, 2: hA == hB and hF == hom, hom wins, A first
    #   1: empty                      2: one het row, 1 < min_win_sites = 2: unused
    #   3: het, het, alt/alt under het, het, alt -> 3, 1, 1, 3: the F1
    #   4: ref/alt under alt; 2 with 2 and a missing call uninformative; a row without a class; alt/ref under ref -> 2, 0, 2, 0: B
    assert twin.pair_windows(snps, classes, win_off, 0, 1).tolist() == [[4, 2, 2, 2], [0, 0, 0, 0], [1, 0, 0, 1], [3, 1, 1, 3], [2, 0, 2, 0]]
    score, n_tot, w_first, w_het = twin.parent_counts(snps, classes, win_off, 2)
    assert (score[0, 1], n_tot[0, 1], w_first[0, 1], w_first[1, 0], w_het[0, 1]) == (7, 9, 1, 1, 1)
    assert (score[1, 0], n_tot[1, 0], w_het[1, 0]) == (7, 9, 1)
    # the diagonal: hA = hB = hF on the rows where the column is homozygous and the sample has a class
    assert (score[0, 0], n_tot[0, 0], w_first[0, 0], w_het[0, 0]) == (3, 9, 3, 0)
    assert (score[1, 1], n_tot[1, 1], w_first[1, 1], w_het[1, 1]) == (6, 10, 3, 0)
    # C carries the "other" code 3: informative against any other call, never the sample's class, never informative against itself;
    # a het call of A matches a het sample (window 4)
    assert twin.pair_windows(snps, classes, win_off, 2, 2).tolist() == [[2, 1, 1, 1], [0, 0, 0, 0], [0, 0, 0, 0], [1, 0, 0, 0], [1, 1, 1, 1]]
    assert twin.pair_windows(snps, classes, win_off, 0, 2).tolist() == [[4, 2, 1, 1], [0, 0, 0, 0], [1, 0, 0, 1], [3, 1, 1, 2], [3, 1, 0, 1]]
    assert (score[0, 2], n_tot[0, 2], w_first[0, 2], w_first[2, 0], w_het[0, 2]) == (2 + 2 + 1, 10, 2, 0, 1)          # window 4: hF == hom, hom wins, A fits better
    # min_win_sites = 1 uses the single-row window as well: the F1 for (A, B)
    one = twin.parent_counts(snps, classes, win_off, 1)
    assert (one[0][0, 1], one[1][0, 1], one[3][0, 1]) == (8, 10, 2)
    # a repeated column: positions 0 and 2 are both A -- every used window is a tie, which goes to the smaller position
    rep = twin.parent_counts(snps, classes, win_off, 2, cols=[0, 1, 0])
    assert (rep[0][0, 2], rep[1][0, 2], rep[2][0, 2], rep[2][2, 0], rep[3][0, 2]) == (3, 9, 3, 0, 0)
    # B at position 1 against A at position 2: the tie of window 0 now goes to B, window 4 is B's anyway
    assert (rep[2][1, 2], rep[2][2, 1], rep[3][1, 2]) == (2, 0, 1) and np.array_equal(rep[0][:2, :2], score[:2, :2])
    for got, want in ((twin.parent_counts(snps, classes, win_off, m), twin.parent_counts_direct(snps, classes, win_off, m)) for m in (1, 2, 3)):
        assert all(np.array_equal(x, y) and x.dtype == np.int32 for x, y in zip(got, want))
    for m in (score, n_tot, w_het):
        assert np.array_equal(m, m.T)
    used = sum((twin.parent_counts(snps[lo:hi], classes[lo:hi], [0, hi - lo], 2)[1] > 0).astype(int) for lo, hi in zip(HAND_OFF, HAND_OFF[1:]))
    off_diag = ~np.eye(3, dtype=bool)
    assert np.array_equal((w_first + w_first.T + w_het)[off_diag], used[off_diag]) and np.array_equal(np.diag(w_first), np.diag(used))


def test_every_row_its_own_window_counts_the_compatible_rows():
    rng = np.random.default_rng(21)
    snps = rng.choice(np.array([-1, 0, 1, 2, 3], dtype=np.int8), size=(400, 6), p=[.1, .4, .35, .1, .05])
    classes = rng.choice(np.array([0, 1, 2, NONE], dtype=np.uint8), size=400, p=[.4, .3, .25, .05])
    score, n_tot, w_first, w_het = twin.parent_counts(snps, classes, np.arange(401), 1)
    c = np.where(snps < 0, -1, np.where(snps > 2, 3, snps)).astype(np.int64)
    s = classes.astype(np.int64)
    for a in range(6):
        for b in range(6):
            x, y = c[:, a], c[:, b]
            f1 = np.where((x == 0) & (y == 0), 0, np.where((x == 1) & (y == 1), 1, np.where((x >= 0) & (y >= 0) & (x != y), 2, -1)))
            ni = (f1 >= 0) & (s <= 2)
            assert n_tot[a, b] == ni.sum() and score[a, b] == (ni & ((x == s) | (y == s) | (f1 == s))).sum()
            assert w_het[a, b] == (ni & (f1 == s) & (x != s) & (y != s)).sum()


# ------------------------------------------------------------------------------------------------ the library's validation
def test_refusals_that_need_no_device():
    lib = _lib.load()
    out = np.zeros((4, 2, 2), dtype=np.int32)
    cols = np.zeros(2, dtype=np.int32)
    good = np.array([0, 1, 2, NONE, 0], dtype=np.uint8)
    off5 = np.array([0, 2, 2, 5], dtype=np.int64)

    def call(ncols, n_rows, outs=(0, 1, 2, 3), cols=cols, cls=good, off=off5, n_win=3, min_sites=1):
        ptrs = [_lib.ptr(out[k]) if k is not None else None for k in outs]
        rc = lib.snpm_panel_parent_counts(None, _lib.ptr(cols), ncols, None, 0, n_rows, _lib.ptr(cls), _lib.ptr(off), n_win, min_sites, *ptrs)
        return rc, lib.snpm_last_error(None).decode()
    bad = _lib.SNPM_ERR_BADARG
    assert call(-1, 5) == (bad, "negative size") and call(2, -1) == (bad, "negative size")
    assert call(2, 5, n_win=-1) == (bad, "negative number of windows")
    for m in (0, -3):
        assert call(2, 5, min_sites=m) == (bad, "min_win_sites must be 1 or more")
    rc, msg = call(11553, 5)
    assert rc == bad and "too many accessions" in msg and "SNPM_F1X_MAX_ACCESSIONS" in msg
    rc, msg = call(2, 2 ** 31)
    assert rc == bad and "2^31 rows" in msg
    assert call(2, 5, off=None) == (bad, "win_off is NULL")
    assert call(2, 5, off=np.array([1, 2, 2, 5], dtype=np.int64)) == (bad, "win_off must start at 0")
    assert call(2, 5, off=np.array([0, 3, 2, 5], dtype=np.int64)) == (bad, "win_off must not decrease")
    assert call(2, 5, off=np.array([0, 2, 2, 4], dtype=np.int64)) == (bad, "win_off must end at n")
    assert call(2, 5, n_win=0) == (bad, "win_off must end at n")                 # no window, but rows
    for outs in ((None, 1, 2, 3), (0, None, 2, 3), (0, 1, None, 3), (0, 1, 2, None)):
        assert call(2, 5, outs) == (bad, "score / n_tot / w_first / w_het is NULL")
    assert call(2, 5, cls=None) == (bad, "sample_class is NULL")
    for byte in (3, 4, 0x7F, 0xFE):
        cls = good.copy()
        cls[3] = byte
        assert call(2, 5, cls=cls) == (bad, "sample_class holds a byte other than 0, 1, 2 or 0xFF")
    assert call(2, 5) == (bad, "panel is NULL")                                   # sound arguments: only the panel is missing
    assert call(0, 5, (None, None, None, None)) == (bad, "panel is NULL")
    assert call(2, 0, cls=None, off=np.zeros(1, dtype=np.int64), n_win=0) == (bad, "panel is NULL")
    assert call(2, 0, cls=None, off=np.zeros(3, dtype=np.int64), n_win=2) == (bad, "panel is NULL")      # empty windows only
    assert call(11552, 5, cols=None) == (bad, "panel is NULL")                    # the limit is inclusive
    assert "snpm_panel_parent_counts" in _lib.SYMBOLS


def test_group_and_streamed_panels_are_refused_with_the_reason():
    cls8, off = np.zeros(3, dtype=np.uint8), np.array([0, 3])
    for cls, why in ((engine.GroupPanel, "spread over several GPUs"), (engine.StreamedPanel, "not a resident panel")):
        with pytest.raises(TypeError, match="parent_counts needs every accession column on one device") as err:
            engine.parent_counts(cls.__new__(cls), cls8, off)
        assert why in str(err.value)
    for cls, why in ((engine.GroupPanel, "spread over several GPUs by accession"), (engine.StreamedPanel, "streamed through the device")):
        with pytest.raises(TypeError, match="the parent search needs every accession column of the DB on one device") as err:
            snp_genotype.Genotype.parent_counts(_Holder(cls.__new__(cls)), cls8, off)
        assert why in str(err.value)


class _Holder(object):
    """stands in for a Genotype whose DB went to the given kind of panel"""

    def __init__(self, panel):
        self._panel = panel

    def panel(self):
        return self._panel


def test_window_tracks_are_the_twin_and_the_tie_follows_the_position():
    rng = np.random.default_rng(22)
    snps = rng.choice(np.array([-1, 0, 1, 2, 3], dtype=np.int8), size=(500, 2), p=[.1, .4, .35, .1, .05])
    classes = rng.choice(np.array([0, 1, 2, NONE], dtype=np.uint8), size=500, p=[.4, .3, .25, .05])
    win_off = np.array([0, 0, 3, 9, 9, 64, 65, 300, 500])
    counts, state = parentsearch.window_tracks(snps[:, 0], snps[:, 1], classes, win_off, 5)
    assert np.array_equal(counts, twin.pair_windows(snps, classes, win_off, 0, 1)) and state.dtype == np.int8
    _, _, w_first, w_het = twin.parent_counts(snps, classes, win_off, 5)
    assert [(state == k).sum() for k in range(3)] == [w_first[0, 1], w_first[1, 0], w_het[0, 1]] and (state == 3).sum() == (counts[:, 0] < 5).sum() >= 4
    same = parentsearch.window_tracks(snps[:, 0], snps[:, 0], classes, win_off, 5)[1]
    swapped = parentsearch.window_tracks(snps[:, 0], snps[:, 0], classes, win_off, 5, a_first_on_tie=False)[1]
    assert set(same.tolist()) == {0, 3} and set(swapped.tolist()) == {1, 3}


# ------------------------------------------------------------------------------------------------ the command
class _FakeDevice(object):
    def likelihood(self, scores, ninfo, truncate=False, amin=None):
        return oracle.calculate_likelihoods(scores, ninfo, "calc" if amin is None else amin)


@pytest.fixture
def planted(monkeypatch, tmp_path):
    """the planted DB as an .npz, the sample as a .bed and the genome as a JSON file; the device calls are the twin and the oracle"""
    case = twin.planted_case()
    snps = case["snps"]
    db = str(tmp_path / "db.npz")
    np.savez(db, snps=snps, accessions=case["names"], positions=case["positions"], chrs=case["chrs"], chr_regions=case["chr_regions"])
    bed = str(tmp_path / "sample.bed")
    with open(bed, "w") as fh:
        for c, p, t in zip(case["s_chr"], case["s_pos"], case["s_gt"]):
            fh.write("%s\t%d\t%s\n" % (c, p, t))
    genome = str(tmp_path / "two_chromosomes.json")
    with open(genome, "w") as fh:
        json.dump(case["genome"], fh)
    calls = []
    stub = engine.Panel.__new__(engine.Panel)
    stub.h = None

    def device(panel, sample_class, win_off, min_win_sites=1, cols=None, rows=None):
        calls.append((cols, rows, np.asarray(win_off).copy(), min_win_sites))
        rows = np.arange(rows.start, rows.stop) if isinstance(rows, range) else rows
        return twin.parent_counts(snps, sample_class, win_off, min_win_sites, cols, rows)

    def single(self, filter_pos_ix=None, mask_acc_ix=None, _filter_mask=None):
        self.get_common_positions()
        db_rows, sample_rows = self.commonSNPs
        score, ninfo = oracle.genotyper_scores(self.inputs.wei[sample_rows], snps[db_rows], match=oracle.match_gts_accs_graph)
        return snpmatch.GenotyperOutput(self.g.g.accessions, score, ninfo, snpmatch.get_fraction(len(db_rows), len(self.inputs.pos)), len(db_rows), self.inputs.dp)
    monkeypatch.setattr(snp_genotype.Genotype, "panel", lambda self, ctx=None, packed=None: stub)
    monkeypatch.setattr(engine, "parent_counts", device)
    monkeypatch.setattr(snpmatch.Genotyper, "genotyper", single)
    monkeypatch.setattr(snpmatch, "_device", lambda: _FakeDevice())
    return case, db, bed, genome, calls


def _one_hot(classes):
    wei = np.zeros((len(classes), 3))
    for c, col in ((0, 0), (1, 2), (2, 1)):
        wei[np.asarray(classes) == c, col] = 1.0
    return wei


def test_command_finds_the_parents_of_the_planted_f2(planted, tmp_path):
    case, db, bed, genome, calls = planted
    snps, classes, win_off = case["snps"], case["classes"], case["win_off"]
    pa, pb = twin.PLANTED_PARENTS
    mosaic = twin.PLANTED_MOSAIC
    assert len(mosaic) == 12 and (mosaic.count("AA"), mosaic.count("BB"), mosaic.count("AB")) == (3, 3, 6) and len(win_off) == 13
    # 1. neither parent is among the ten best single accessions: the 45 crosses of the reference's route never hold the true pair
    s, n = oracle.genotyper_scores(_one_hot(classes), snps, match=oracle.match_gts_accs_graph)
    ten = np.argsort(-(s / n))[:10]
    assert pa not in ten and pb not in ten and set(ten.tolist()) <= set(range(20, 32))
    # 2. scored as a whole-genome F1 the true pair is not first: a pair of decoys is
    hits, ninfo = f1search_twin.f1_counts(snps, classes)
    first = f1search.shortlist(hits, ninfo, 1, 100)[0]
    assert first[:2] != (pa, pb) and set(first[:2]) <= set(range(20, 32)) and hits[pa, pb] * first[3] < first[2] * ninfo[pa, pb]
    # 3. parentsearch puts it first with score == n, and 4. its windows are the planted pattern
    out = str(tmp_path / "out")
    assert cli.main(["parentsearch", "-i", bed, "-d", db, "--genome", genome, "-b", str(twin.PLANTED_BIN), "-o", out]) == 0
    assert len(calls) == 1 and calls[0][0] is None and np.array_equal(np.asarray(calls[0][1]), np.arange(3000))
    assert np.array_equal(calls[0][2], win_off) and calls[0][3] == 5
    stats = json.load(open(out + ".parentsearch.json"))
    best = stats["best_pair"]
    assert (best["acc_1"], best["acc_2"]) == ("acc%02d" % pa, "acc%02d" % pb) and best["score"] == best["n"] == 3000 and best["fraction"] == 1.0
    assert (best["windows_A"], best["windows_B"], best["windows_AB"], best["windows_unused"]) == (3, 3, 6, 0)
    assert stats["in_top10_route"] is False and stats["matched_rows"] == 3000 and stats["windows"] == 12 and stats["candidates"] == 40
    assert stats["best_single"]["accession"] == "acc%02d" % ten[0] and len(stats["shortlist"]) == 10 and stats["shortlist"][0] == best
    second = stats["shortlist"][1]
    assert second["score"] < second["n"] < 3000
    fracs = [(p["score"], p["n"]) for p in stats["shortlist"]]
    assert all(h1 * n2 >= h2 * n1 for (h1, n1), (h2, n2) in zip(fracs, fracs[1:]))
    z = np.load(out + ".parentsearch.npz")
    want = twin.parent_counts(snps, classes, win_off, 5)
    assert z["accessions"].tolist() == case["names"].tolist() and all(np.array_equal(z[k], w) and z[k].dtype == np.int32
                                                                      for k, w in zip(("score", "n_tot", "w_first", "w_het"), want))
    assert np.array_equal(z["win_off"], win_off) and z["win_chr"].tolist() == [0] * 6 + [1] * 6
    lines = [ln.split("\t") for ln in open(out + ".parentsearch.windows.tsv").read().splitlines()]
    assert lines[0] == ["chr", "window", "pair", "n", "hA", "hB", "hF", "state"] and len(lines) == 1 + 10 * 12
    mine = lines[1:13]
    assert [ln[7] for ln in mine] == [{"AA": "A", "BB": "B", "AB": "AB"}[m] for m in mosaic]
    assert all(ln[2] == "acc%02dxacc%02d" % (pa, pb) and ln[3] == "250" for ln in mine) and [ln[0] for ln in mine] == ["Chr1"] * 6 + ["Chr2"] * 6
    assert [[int(v) for v in ln[3:7]] for ln in mine] == twin.pair_windows(snps, classes, win_off, pa, pb).tolist()
    for k, p in enumerate(stats["shortlist"]):                  # every listed pair's track agrees with its cells of the matrices
        states = [ln[7] for ln in lines[1 + 12 * k:13 + 12 * k]]
        assert [states.count(t) for t in ("A", "B", "AB", "NA")] == [p["windows_A"], p["windows_B"], p["windows_AB"], p["windows_unused"]]
    # a candidate list in another order: the pair is named by the list's order, the tie rule by its positions
    acc_file = tmp_path / "cands.txt"
    acc_file.write_text("acc17\nacc21\nacc03\nacc05\n")
    assert cli.main(["parentsearch", "-i", bed, "-d", db, "--genome", genome, "-b", str(twin.PLANTED_BIN), "-a", str(acc_file), "--top", "3",
                     "--min_sites", "2000", "--min_win_sites", "1", "-o", out]) == 0
    stats = json.load(open(out + ".parentsearch.json"))
    best = stats["best_pair"]
    assert (best["acc_1"], best["acc_2"]) == ("acc17", "acc03") and (best["windows_A"], best["windows_B"], best["windows_AB"]) == (3, 3, 6)
    assert stats["candidates"] == 4 and calls[-1][0].tolist() == [17, 21, 3, 5] and calls[-1][3] == 1
    assert cli.main(["parentsearch", "-i", bed, "-d", db, "--genome", genome, "--top", "17", "-o", out]) == 2
    assert cli.main(["parentsearch", "-i", bed, "-d", db, "--genome", genome, "--min_win_sites", "0", "-o", out]) == 2


# ------------------------------------------------------------------------------------------------ the kernels and the plan, on the host
def test_kernel_source_and_plan_on_the_host_under_asan_and_ubsan(tmp_path):
    """every block of k_win_planes / k_par_count run by 256 real threads with a barrier, exact-size heap buffers, arbitrary pad bytes,
    stale planes: 1 / 2 / 31 / 32 / 33 / 65 accessions x 1 / 63 / 64 / 65 / 1025 rows over the three layouts with one window, every
    row its own window, boundaries at 63 | 64 | 65, empty windows and windows of 7 rows; a window across an LDS step; a window longer
    than a chunk at 33 accessions; two and three slabs, one of a window larger than the budget; column lists with a repeat and
    unsorted row lists with a repeat (one over three slabs); the split layout at 1135 accessions.  The plan of every case is replayed
    bit by bit against the classes and the windows; the plan alone: a boundary at bit 0, at bit 63, several inside one word, empty
    windows first, in the middle and last, a window longer than a chunk, a window larger than the budget, a budget of three slabs"""
    cases = host_kernel_util.run_driver("par_host_driver", tmp_path)
    plans = [ln for ln in cases if ln.startswith("case plan-")]
    assert len(cases) == 71 and len(plans) == 8
    assert {ln.split()[1] for ln in plans} == {"plan-bit0", "plan-bit63", "plan-many-in-a-word", "plan-empty-windows", "plan-long-window",
                                               "plan-over-budget", "plan-three-slabs", "plan-rows-own"}
    kernels = [ln for ln in cases if not ln.startswith("case plan-")]
    assert sum(" slabs=2 " in ln for ln in kernels) == 1 and sum(" slabs=3 " in ln for ln in kernels) == 3
    for acc in (1, 2, 31, 32, 33, 65):
        for rows in (1, 63, 64, 65, 1025):
            assert any(" acc=%d " % acc in ln and " rows=%d " % rows in ln for ln in kernels), (acc, rows)
    for name in ("one-window", "rows-own", "cuts-63-64-65", "empty-windows", "across-step", "long-window"):
        assert {ln.split()[2] for ln in kernels if ln.split()[1] == name} == {"layout=0", "layout=1", "layout=2"} or name == "long-window"
    assert any(ln.split()[1] == "long-window" and " acc=33 " in ln and " groups=3 " in ln for ln in kernels)
