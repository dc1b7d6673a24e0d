"""f1search without a GPU: the numpy twin (tests/f1search_twin.py) against the goldens of the unmodified reference
(``CrossIdentifier.match_insilico_f1s`` on one-hot weights: every score and numinfo, no tolerance), against ``oracle.insilico_f1_pairs``
and on a hand-made matrix; ``hard_classes`` against the reference's weights; ``shortlist`` on ties and on ``min_sites``; every refusal
of ``snpm_panel_f1_counts`` that needs no device; the ``f1search`` subcommand with the twin in the place of the device on a planted
panel whose true parents the reference's ten-best route cannot find; and the kernel source itself, compiled for the host and run by
256 real threads per block under AddressSanitizer + UBSan (tests/f1x_host_driver.cpp on tests/host_kernel/, a child process)."""
import glob
import itertools
import json
import os

import numpy as np
import pytest

import f1search_twin
import host_kernel_util
from oracle import snpmatch_oracle as oracle
from snpmatch_amd import _lib, cli, engine
from snpmatch_amd.core import f1search, snp_genotype, snpmatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["f1search_a%d" % a for a in (2, 7, 10)]


def one_hot(classes):
    """[ref, het, alt] weights of hard classes, as ``get_wei_from_GT`` lays them out: class 1 is column 2, class 2 column 1"""
    wei = np.zeros((len(classes), 3))
    for c, col in ((0, 0), (1, 2), (2, 1)):
        wei[np.asarray(classes) == c, col] = 1.0
    return wei


def test_every_golden_is_listed(golden_dir):
    assert sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(golden_dir, "f1search_a*.npz"))) == sorted(CASES)


@pytest.mark.parametrize("name", CASES)
def test_twin_and_hard_classes_reproduce_the_reference(name, golden_dir):
    case = np.load(os.path.join(golden_dir, name + ".npz"))
    snps, gt, wei = case["snps"], case["gt"], case["wei"]
    n_acc = snps.shape[1]
    assert snps.dtype == np.int8 and set(np.unique(snps).tolist()) == {-1, 0, 1, 2, 3}
    assert set(gt.tolist()) == {"0/0", "1/1", "0/1", "1/0", "1/2", "./."} and len(case["score"]) == n_acc * (n_acc - 1) // 2
    classes = f1search.hard_classes(gt)
    assert classes.dtype == np.uint8 and np.array_equal(one_hot(classes), wei)           # the reference's own get_wei_from_GT
    assert np.array_equal(classes[gt == "1/2"], np.zeros((gt == "1/2").sum())) and (classes[gt == "./."] == 0xFF).all()
    hits, ninfo = f1search_twin.f1_counts(snps, classes)
    assert hits.dtype == np.int32 and ninfo.dtype == np.int32 and np.array_equal(hits, hits.T) and np.array_equal(ninfo, ninfo.T)
    a, b = case["pair_a"], case["pair_b"]
    assert case["score"].dtype == np.float64 and np.array_equal(hits[a, b].astype(np.float64), case["score"])
    assert np.array_equal(ninfo[a, b].astype(np.int64), case["numinfo"])
    direct = f1search_twin.f1_counts_direct(snps, classes)
    assert np.array_equal(direct[0], hits) and np.array_equal(direct[1], ninfo)


def test_the_planted_rows_and_columns_are_in_the_goldens(golden_dir):
    for name in CASES:
        case = np.load(os.path.join(golden_dir, name + ".npz"))
        snps, gt = case["snps"], case["gt"]
        classes = f1search.hard_classes(gt)
        at = {(int(a), int(b)): k for k, (a, b) in enumerate(zip(case["pair_a"], case["pair_b"]))}
        k01 = at.get((0, 1), at.get((1, 0)))
        # row 0: 2 with 2 under a het sample; row 1: 3 with 3 -- neither is informative for the cross of 0 and 1
        assert (snps[0, :2] == 2).all() and classes[0] == 2 and (snps[1, :2] == 3).all()
        rest = f1search_twin.f1_counts(snps[2:], classes[2:])
        assert case["numinfo"][k01] == rest[1][0, 1] and case["score"][k01] == rest[0][0, 1] and case["numinfo"][k01] > 0
        if snps.shape[1] >= 7:
            k56 = at.get((5, 6), at.get((6, 5)))
            assert case["numinfo"][k56] == 0 and case["score"][k56] == 0            # a pair with no informative row ...
            assert all(case["numinfo"][at.get((5, c), at.get((c, 5)))] > 0 for c in (0, 1, 3))     # ... of members that have some
            assert (snps[:, 2] == -1).all()                                         # an accession without a call
            assert not any(case["numinfo"][k] for (a, b), k in at.items() if 2 in (a, b))


def test_twin_equals_the_oracle_on_random_one_hot_weights():
    rng = np.random.default_rng(5)
    snps = rng.choice(np.array([-1, 0, 1, 2, 3], dtype=np.int8), size=(700, 9), p=[.1, .4, .35, .1, .05])
    classes = rng.choice(np.array([0, 1, 2, 0xFF], dtype=np.uint8), size=700, p=[.4, .3, .25, .05])
    score, numinfo = oracle.insilico_f1_pairs(snps, one_hot(classes))
    hits, ninfo = f1search_twin.f1_counts(snps, classes)
    pairs = list(itertools.combinations(range(9), 2))
    assert [hits[p] for p in pairs] == score.tolist() and [ninfo[p] for p in pairs] == numinfo.tolist()
    cols, rows = np.array([4, 0, 4, 8]), rng.integers(0, 700, size=300)
    sub = f1search_twin.f1_counts(snps, classes[rows], cols, rows)
    want = f1search_twin.f1_counts_direct(snps[rows][:, cols], classes[rows])
    assert np.array_equal(sub[0], want[0]) and np.array_equal(sub[1], want[1])


def test_twin_on_a_hand_made_matrix():
    snps = np.array([[0, 0, -1, 3], [1, 0, 1, 3], [2, 1, 1, -1], [1, 1, 0, 2]], dtype=np.int8)
    classes = np.array([0, 2, 1, 0xFF], dtype=np.uint8)
    hits, ninfo = f1search_twin.f1_counts(snps, classes)
    # e.g. (0, 1): rows ref, het, het, alt -> informative 4; classes ref, het, alt, none -> hits at rows 0 and 1
    assert ninfo.tolist() == [[3, 4, 3, 3], [4, 4, 3, 3], [3, 3, 3, 2], [3, 3, 2, 0]]
    assert hits.tolist() == [[1, 2, 0, 1], [2, 2, 2, 1], [0, 2, 1, 1], [1, 1, 1, 0]]
    none = f1search_twin.f1_counts(snps, np.full(4, 0xFF, dtype=np.uint8))
    assert not none[0].any() and np.array_equal(none[1], ninfo)
    sub = f1search_twin.f1_counts(snps, classes[[3, 3, 1]], cols=[2, 0, 2], rows=[3, 3, 1])       # repeats count as listed
    # rows 3, 3, 1 of columns 2, 0, 2: het, het, alt for the pair and ref, ref, alt for a column with itself; classes none, none, het
    assert sub[1].tolist() == [[3, 3, 3], [3, 3, 3], [3, 3, 3]] and not sub[0].any()
    alt = f1search_twin.f1_counts(snps, np.array([2, 0, 1], dtype=np.uint8), cols=[2, 0, 2], rows=[3, 3, 1])
    assert alt[0].tolist() == [[2, 2, 2], [2, 1, 2], [2, 2, 2]]


def test_shortlist_ranks_exactly_and_breaks_ties():
    def mats(cells, n=5):
        hits, ninfo = np.zeros((n, n), dtype=np.int32), np.zeros((n, n), dtype=np.int32)
        for (a, b), (h, m) in cells.items():
            hits[a, b] = hits[b, a] = h
            ninfo[a, b] = ninfo[b, a] = m
        return hits, ninfo
    # equal fractions 1/2 = 2/4 = 3/6: the larger ninfo first; the same ninfo: the smaller (a, b) first
    hits, ninfo = mats({(0, 1): (1, 2), (0, 2): (3, 6), (1, 2): (2, 4), (3, 4): (3, 6), (0, 4): (5, 6)})
    assert f1search.shortlist(hits, ninfo, top=10, min_sites=1) == [(0, 4, 5, 6), (0, 2, 3, 6), (3, 4, 3, 6), (1, 2, 2, 4), (0, 1, 1, 2)]
    assert f1search.shortlist(hits, ninfo, top=2, min_sites=1) == [(0, 4, 5, 6), (0, 2, 3, 6)]
    assert f1search.shortlist(hits, ninfo, top=10, min_sites=5) == [(0, 4, 5, 6), (0, 2, 3, 6), (3, 4, 3, 6)]
    assert f1search.shortlist(hits, ninfo, top=10, min_sites=7) == [] and f1search.shortlist(hits, ninfo, top=3, min_sites=0)[0] == (0, 4, 5, 6)
    # fractions that fp64 cannot tell apart are told apart: (2^30 - 1) / 2^30 against (2^30 - 2) / (2^30 - 1), both round-trip near 1
    big = 2 ** 30
    hits, ninfo = mats({(0, 1): (big - 2, big - 1), (2, 3): (big - 1, big), (1, 4): (big - 3, big - 2)})
    assert f1search.shortlist(hits, ninfo, top=3, min_sites=100) == [(2, 3, big - 1, big), (0, 1, big - 2, big - 1), (1, 4, big - 3, big - 2)]
    assert f1search.shortlist(hits, ninfo, top=1, min_sites=100) == [(2, 3, big - 1, big)]
    # the diagonal (a line crossed with itself) is never listed
    hits, ninfo = mats({(0, 0): (9, 9), (1, 1): (9, 9), (0, 1): (1, 9)}, n=2)
    assert f1search.shortlist(hits, ninfo, top=5, min_sites=1) == [(0, 1, 1, 9)]
    for top in (0, 17):
        with pytest.raises(ValueError, match="top must be 1 .. 16"):
            f1search.shortlist(hits, ninfo, top=top)


# ------------------------------------------------------------------------------------------------ the library's validation
def test_refusals_that_need_no_device():
    lib = _lib.load()
    out = np.zeros((2, 2, 2), dtype=np.int32)
    cols = np.zeros(2, dtype=np.int32)
    good = np.array([0, 1, 2, 0xFF, 0], dtype=np.uint8)

    def call(ncols, n_rows, outs=(0, 1), cols=cols, cls=good):
        ptrs = [_lib.ptr(out[k]) if k is not None else None for k in outs]
        rc = lib.snpm_panel_f1_counts(None, _lib.ptr(cols), ncols, None, 0, n_rows, _lib.ptr(cls), *ptrs)
        return rc, lib.snpm_last_error(None).decode()
    assert call(-1, 5) == (_lib.SNPM_ERR_BADARG, "negative size")
    assert call(2, -1) == (_lib.SNPM_ERR_BADARG, "negative size")
    rc, msg = call(11553, 5)
    assert rc == _lib.SNPM_ERR_BADARG and "too many accessions" in msg and "SNPM_F1X_MAX_ACCESSIONS" in msg
    rc, msg = call(2, 2 ** 31)
    assert rc == _lib.SNPM_ERR_BADARG and "2^31 rows" in msg
    for outs in ((None, 1), (0, None)):
        assert call(2, 5, outs) == (_lib.SNPM_ERR_BADARG, "hits / ninfo is NULL")
    assert call(2, 5, cls=None) == (_lib.SNPM_ERR_BADARG, "sample_class is NULL")
    for bad in (3, 4, 0x7F, 0xFE):
        cls = good.copy()
        cls[3] = bad
        assert call(2, 5, cls=cls) == (_lib.SNPM_ERR_BADARG, "sample_class holds a byte other than 0, 1, 2 or 0xFF")
    assert call(2, 5) == (_lib.SNPM_ERR_BADARG, "panel is NULL")                  # sound arguments: only the panel is missing
    assert call(0, 5, (None, None)) == (_lib.SNPM_ERR_BADARG, "panel is NULL")
    assert call(2, 0, cls=None) == (_lib.SNPM_ERR_BADARG, "panel is NULL")
    assert call(11552, 5, cols=None) == (_lib.SNPM_ERR_BADARG, "panel is NULL")  # the limit is inclusive
    header = open(os.path.join(ROOT, "include", "snpmatch_hip.h")).read()
    assert "#define SNPM_F1X_MAX_ACCESSIONS 11552" in header and engine.F1X_MAX_ACCESSIONS == 11552
    assert 11552 ** 2 < 2 ** 27 and (11552 // 32) * (11552 // 32 + 1) // 2 < 2 ** 16
    assert "snpm_panel_f1_counts" in _lib.SYMBOLS


def test_group_and_streamed_panels_are_refused_with_the_reason():
    cls8 = np.zeros(3, dtype=np.uint8)
    for cls, why in ((engine.GroupPanel, "spread over several GPUs"), (engine.StreamedPanel, "not a resident panel")):
        with pytest.raises(TypeError, match="f1_counts needs every accession column on one device") as err:
            engine.f1_counts(cls.__new__(cls), cls8)
        assert why in str(err.value)
    for cls, why in ((engine.GroupPanel, "spread over several GPUs by accession"), (engine.StreamedPanel, "streamed through the device")):
        with pytest.raises(TypeError, match="the exhaustive F1 search needs every accession column of the DB on one device") as err:
            snp_genotype.Genotype.f1_counts(_Holder(cls.__new__(cls)), cls8)
        assert why in str(err.value)


class _Holder(object):
    """stands in for a Genotype whose DB went to the given kind of panel"""

    def __init__(self, panel):
        self._panel = panel

    def panel(self):
        return self._panel


# ------------------------------------------------------------------------------------------------ the command
class _FakeQuery(object):
    """``Query.f1_pairs`` by the oracle"""

    def __init__(self, snps, db_rows, wei):
        self.snps, self.db_rows, self.wei = snps, np.asarray(db_rows), np.asarray(wei)

    def f1_pairs(self, acc_idx):
        return oracle.insilico_f1_pairs(self.snps[self.db_rows][:, np.asarray(acc_idx)], self.wei)

    def free(self):
        pass


class _FakeDevice(object):
    def likelihood(self, scores, ninfo, truncate=False, amin=None):
        return oracle.calculate_likelihoods(scores, ninfo, "calc" if amin is None else amin)


@pytest.fixture
def planted(monkeypatch, tmp_path):
    """the planted DB as an .npz and the sample as a .bed; the device calls are the twin and the oracle"""
    case = f1search_twin.planted_case()
    snps = case["snps"]
    db = str(tmp_path / "db.npz")
    np.savez(db, snps=snps, accessions=case["names"], positions=case["positions"], chrs=case["chrs"], chr_regions=case["chr_regions"])
    bed = str(tmp_path / "sample.bed")
    with open(bed, "w") as fh:
        for c, p, t in zip(case["s_chr"], case["s_pos"], case["s_gt"]):
            fh.write("%s\t%d\t%s\n" % (c, p, t))
    calls = []

    class FakePanel(engine.Panel):
        def query(self, db_rows, wei):
            return _FakeQuery(snps, db_rows, wei)
    stub = FakePanel.__new__(FakePanel)
    stub.h = None

    def twin(panel, sample_class, cols=None, rows=None):
        calls.append((cols, rows))
        rows = np.arange(rows.start, rows.stop) if isinstance(rows, range) else rows
        return f1search_twin.f1_counts(snps, sample_class, cols, rows)

    def single(self, filter_pos_ix=None, mask_acc_ix=None, _filter_mask=None):
        self.get_common_positions()
        db_rows, sample_rows = self.commonSNPs
        score, ninfo = oracle.genotyper_scores(self.inputs.wei[sample_rows], snps[db_rows], match=oracle.match_gts_accs_graph)
        return snpmatch.GenotyperOutput(self.g.g.accessions, score, ninfo, snpmatch.get_fraction(len(db_rows), len(self.inputs.pos)), len(db_rows), self.inputs.dp)
    monkeypatch.setattr(snp_genotype.Genotype, "panel", lambda self, ctx=None, packed=None: stub)
    monkeypatch.setattr(engine, "f1_counts", twin)
    monkeypatch.setattr(snpmatch.Genotyper, "genotyper", single)
    monkeypatch.setattr(snpmatch, "_device", lambda: _FakeDevice())
    return case, db, bed, calls


def test_command_finds_the_pair_the_ten_best_route_cannot(planted, tmp_path):
    case, db, bed, calls = planted
    snps, rows, classes = case["snps"], case["db_rows"], case["classes"]
    pa, pb = f1search_twin.PLANTED_PARENTS
    # the fixture proves something: on their own both parents rank below ten other lines, and none of the 45 crosses of those
    # ten reaches the true pair
    wei = one_hot(classes)
    s, n = oracle.genotyper_scores(wei, snps[rows], match=oracle.match_gts_accs_graph)
    ten = np.argsort(-(s / n))[:10]
    assert pa not in ten and pb not in ten and set(ten.tolist()) <= set(range(20, 32))
    route_s, route_n = oracle.insilico_f1_pairs(snps[rows][:, ten], wei)
    true_s, true_n = oracle.insilico_f1_pairs(snps[rows][:, [pa, pb]], wei)
    assert true_s[0] == true_n[0] == 3000 and (route_s / route_n).max() < 0.97
    out = str(tmp_path / "out")
    assert cli.main(["f1search", "-i", bed, "-d", db, "-o", out]) == 0
    assert len(calls) == 1 and calls[0][0] is None and np.array_equal(np.asarray(calls[0][1]), rows)
    stats = json.load(open(out + ".f1search.json"))
    best = stats["best_pair"]
    assert (best["acc_1"], best["acc_2"]) == ("acc%02d" % pa, "acc%02d" % pb) and best["hits"] == best["ninfo"] == 3000
    assert best["score"] == 3000.0 and best["numinfo"] == 3000 and best["fraction"] == 1.0
    assert stats["in_top10_route"] is False and stats["matched_rows"] == 3000 and stats["candidates"] == 40
    assert stats["class_rows"] == {k: int((classes == c).sum()) for k, c in (("ref", 0), ("alt", 1), ("het", 2), ("none", 0xFF))}
    assert stats["best_single"]["accession"] == "acc%02d" % ten[0] and stats["best_single"]["fraction"] == float(s[ten[0]] / n[ten[0]])
    assert len(stats["shortlist"]) == 10 and stats["shortlist"][0] == best
    fracs = [(p["hits"], p["ninfo"]) for p in stats["shortlist"]]
    assert all(h1 * n2 >= h2 * n1 for (h1, n1), (h2, n2) in zip(fracs, fracs[1:]))
    assert all(p["score"] == p["hits"] and p["numinfo"] == p["ninfo"] for p in stats["shortlist"])       # a hard-called sample: the screen is the score
    z = np.load(out + ".f1search.npz")
    hits, ninfo = f1search_twin.f1_counts(snps, classes, None, rows)
    assert z["accessions"].tolist() == case["names"].tolist() and np.array_equal(z["hits"], hits) and np.array_equal(z["ninfo"], ninfo)
    assert z["hits"].dtype == np.int32 and z["class_rows"].tolist() == [stats["class_rows"][k] for k in ("ref", "alt", "het", "none")]
    lines = [ln.split("\t") for ln in open(out + ".f1search.scores.txt").read().splitlines()]
    assert len(lines) == 50 and all(len(ln) == 8 for ln in lines) and [ln[0] for ln in lines[:40]] == case["names"].tolist()
    assert lines[40][0] == "acc%02dxacc%02d" % (pa, pb) and lines[40][1:4] == ["3000.0", "3000", "1.0"] and lines[40][6] == "3000"
    assert [ln[0] for ln in lines[40:]] == ["%sx%s" % (p["acc_1"], p["acc_2"]) for p in stats["shortlist"]]
    # a candidate list: the pairs are those of its members, named by the DB's accessions
    acc_file = tmp_path / "cands.txt"
    acc_file.write_text("acc17\nacc21\nacc03\nacc05\n")
    assert cli.main(["f1search", "-i", bed, "-d", db, "-a", str(acc_file), "--top", "3", "--min_sites", "2000", "-o", out]) == 0
    stats = json.load(open(out + ".f1search.json"))
    assert (stats["best_pair"]["acc_1"], stats["best_pair"]["acc_2"]) == ("acc17", "acc03") and len(stats["shortlist"]) == 3 and stats["candidates"] == 4
    assert np.load(out + ".f1search.npz")["accessions"].tolist() == ["acc17", "acc21", "acc03", "acc05"] and calls[-1][0].tolist() == [17, 21, 3, 5]
    assert cli.main(["f1search", "-i", bed, "-d", db, "--top", "17", "-o", out]) == 2
    acc_file.write_text("acc17\nacc17\n")
    assert cli.main(["f1search", "-i", bed, "-d", db, "-a", str(acc_file), "-o", out]) == 2


# ------------------------------------------------------------------------------------------------ the kernels, on the host
def test_kernel_source_on_the_host_under_asan_and_ubsan(tmp_path):
    """every block of k_win_planes / k_f1x_count run by 256 real threads with a barrier, exact-size heap buffers, arbitrary pad
    bytes, stale planes: 1 / 2 / 31 / 32 / 33 / 65 / 130 accessions x 1 / 63 / 64 / 65 rows in the three layouts, one row past an LDS
    step and past a chunk in each layout, classes with 0xFF, two and three slabs, column lists with a repeat and unsorted row lists
    with a repeat (one over three slabs), the split layout at 1135 accessions; and the slab plan alone at the grid.y cap and below
    one step"""
    cases = host_kernel_util.run_driver("f1x_host_driver", tmp_path)
    assert len(cases) == 44 and sum(ln.startswith("case plan-") for ln in cases) == 2
    assert sum("slabs=2" in ln for ln in cases) == 2 and sum("slabs=3" in ln for ln in cases) == 2
    assert not any("noclass=0 " in ln for ln in cases if "rows=1 " not in ln and not ln.startswith("case plan-"))
