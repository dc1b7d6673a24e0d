"""power without a GPU: the numpy twin (tests/power_twin.py) against a per-row brute-force loop and against the oracle's score / numinfo
of the simulated sample's one-hot weights; the hash of csrc/snpm_k_sim.hpp (printed by the host driver) against the twin's numpy
restatement; the ladder draw, the vectorised likelihoods against the oracle's ``calculate_likelihoods`` and the level report on a
hand-made matrix; every refusal of ``snpm_panel_sim_counts`` that needs no device; the ``power`` subcommand with the twin in the place
of the device on a planted panel with two near-identical accessions; and the kernel source itself, compiled for the host and run by 256
real threads per block under AddressSanitizer + UBSan (tests/sim_host_driver.cpp on tests/host_kernel/, a child process)."""
import json
import os
import re

import numpy as np
import pytest

import host_kernel_util
import power_twin
from oracle import snpmatch_oracle as oracle
from snpmatch_amd import _lib, cli, engine
from snpmatch_amd.core import power, snp_genotype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF = power_twin.err_threshold(0.5)


def _calls(rng, n_rows, n_acc):
    return rng.choice(np.array([-1, 0, 1, 2, 3], dtype=np.int8), size=(n_rows, n_acc), p=[0.1, 0.4, 0.3, 0.12, 0.08])


# ------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("err_thr", [0, power_twin.err_threshold(0.05), HALF, 1 << 32])
def test_twin_equals_a_per_row_loop(err_thr):
    rng = np.random.default_rng(11)
    snps = _calls(rng, 160, 6)
    grp_off = [0, 0, 1, 63, 64, 64, 130, 130]
    rows = rng.integers(0, 160, size=130)
    cols = [5, 0, 3, 3, 1]
    got = power_twin.sim_counts(snps, grp_off, err_thr, 77, cols, rows)
    want = power_twin.sim_counts_direct(snps, grp_off, err_thr, 77, cols, rows)
    assert got[0].dtype == np.int32 and got[0].shape == (7, 5, 5)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert not got[0][0].any() and not got[1][4].any() and got[1].sum() > 0       # empty groups first and in the middle
    whole = power_twin.sim_counts(snps, [0, 130], err_thr, 77, cols, rows)
    assert np.array_equal(got[0].sum(axis=0), whole[0][0]) and np.array_equal(got[1].sum(axis=0), whole[1][0])        # groups add
    # a column listed twice: equal samples without errors, independent ones with (the hash is keyed by the position in the list)
    same = np.array_equal(got[0][:, 2], got[0][:, 3])
    assert same == (err_thr == 0) and np.array_equal(got[0][:, :, 2], got[0][:, :, 3]) and np.array_equal(got[1][:, 2], got[1][:, 3])


def test_twin_without_errors_is_the_identity_count():
    rng = np.random.default_rng(12)
    snps = _calls(rng, 300, 7)
    score, ninfo = power_twin.sim_counts(snps, [0, 300], 0, 0)
    called = (snps >= 0) & (snps <= 2)
    assert np.array_equal(np.diagonal(score[0]), called.sum(axis=0)) and np.array_equal(np.diagonal(ninfo[0]), called.sum(axis=0))
    assert ninfo[0][0, 1] == (called[:, 0] & (snps[:, 1] >= 0)).sum() and not np.array_equal(ninfo[0], ninfo[0].T)     # code 3 counts on side b only
    assert np.array_equal(score[0], score[0].T)                                 # equal codes: symmetric without errors
    noisy = power_twin.sim_counts(snps, [0, 300], 1 << 32, 0)
    assert np.array_equal(noisy[1], ninfo) and not np.array_equal(noisy[0], score) and not np.array_equal(noisy[0][0], noisy[0][0].T)
    # every call redrawn from three classes: about a third keeps its class
    assert abs(np.diagonal(noisy[0][0]).sum() / called.sum() - 1 / 3) < 0.05


def _one_hot(classes):
    """[ref, het, alt] weights of hard classes, as ``get_wei_from_GT`` lays them out"""
    wei = np.zeros((len(classes), 3))
    for c, col in ((0, 0), (1, 2), (2, 1)):
        wei[np.asarray(classes) == c, col] = 1.0
    return wei


@pytest.mark.parametrize("err_thr", [0, power_twin.err_threshold(0.2)])
def test_twin_equals_the_oracle_on_the_samples_one_hot_weights(err_thr):
    """sample a IS a hard-called sample with calls at the rows where column a has one: ScoreList / NumInfoSites of the oracle's own
    chunk loop over those rows"""
    rng = np.random.default_rng(13)
    snps = _calls(rng, 2300, 5)
    score, ninfo = power_twin.sim_counts(snps, [0, 2300], err_thr, 5)
    classes = power_twin.sample_classes(snps, err_thr, 5)
    assert err_thr == 0 or (classes != np.where((snps >= 0) & (snps <= 2), snps, 0xFF)).sum() > 100
    for a in range(5):
        has = np.flatnonzero(classes[:, a] != power_twin.NO_CALL)
        assert 0 < len(has) < 2300
        s, n = oracle.genotyper_scores(_one_hot(classes[has, a]), snps[has], match=oracle.match_gts_accs_graph)
        assert np.array_equal(score[0][a].astype(np.float64), s) and np.array_equal(ninfo[0][a].astype(np.int64), n)


def test_threshold_of_an_error_rate():
    assert engine.sim_err_threshold(0) == 0 and engine.sim_err_threshold(1.0) == 1 << 32 and engine.sim_err_threshold(0.5) == 1 << 31
    assert engine.sim_err_threshold(0.001) == int(0.001 * 2 ** 32) == power_twin.err_threshold(0.001)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="err_rate must lie in 0 .. 1"):
            engine.sim_err_threshold(bad)


# ------------------------------------------------------------------------------------------------ ladder, likelihoods, report
def test_ladder_is_nested_sorted_inside_groups_and_stages_no_row_twice():
    rows, grp_off = power.draw_ladder(1000, [10, 100, 400], np.random.default_rng(3))
    assert grp_off.tolist() == [0, 10, 100, 400] and len(rows) == 400 and len(set(rows.tolist())) == 400
    perm = np.random.default_rng(3).permutation(1000)
    for lo, hi in zip(grp_off[:-1], grp_off[1:]):
        assert np.array_equal(rows[lo:hi], np.sort(perm[lo:hi]))
    pool = np.arange(500, 530)
    rows, grp_off = power.draw_ladder(1000, [10, 100], np.random.default_rng(3), pool)       # a level above the candidates is cut
    assert grp_off.tolist() == [0, 10, 30] and sorted(rows.tolist()) == pool.tolist()
    assert power.parse_levels("100,1000, 10000") == [100, 1000, 10000]
    for bad in ("", "10,10", "100,50", "0,5", ",".join(str(i) for i in range(1, 66))):
        with pytest.raises(ValueError):
            power.parse_levels(bad)


def test_likelihoods_are_those_of_calculate_likelihoods_row_by_row():
    """the same formula evaluated over a matrix: numpy's log of an array and of a scalar may differ in the last bit (different
    vector paths), the products and the sum then by a few ulp -- 1e-12 relative is far above that and far below any decision"""
    rng = np.random.default_rng(14)
    ninfo = rng.integers(0, 3000, size=(40, 9))
    score = (ninfo * rng.random((40, 9))).astype(np.int64)
    score[0], ninfo[1] = 0, 0
    score[1] = 0
    score[2] = ninfo[2]
    score[3, :4] = ninfo[3, :4]
    lik, lrt = power.likelihoods(score, ninfo)
    for r in range(40):
        if r in (0, 1):
            assert np.isnan(lik[r]).all() and np.isnan(lrt[r]).all()
            continue
        want_lik, want_lrt = oracle.calculate_likelihoods(score[r], ninfo[r])
        assert np.array_equal(np.isnan(lik[r]), np.isnan(want_lik)) and np.array_equal(np.isnan(lrt[r]), np.isnan(want_lrt))
        assert np.allclose(lik[r], want_lik, rtol=1e-12, atol=0, equal_nan=True) and np.allclose(lrt[r], want_lrt, rtol=1e-12, atol=0, equal_nan=True)
    assert (lik[2][ninfo[2] > 0] == 1).all() and (lrt[2][ninfo[2] > 0] == 1).all()
    with pytest.raises(AssertionError, match="provided y is greater than n"):
        power.likelihoods(np.array([[2]]), np.array([[1]]))


def test_level_report_on_a_hand_made_matrix():
    # sample 0: perfect on itself, 1 is a duplicate, 2 far off; sample 1: better on 0 than on itself; sample 2: no call at all
    score = np.array([[100, 100, 50], [99, 90, 40], [0, 0, 0]])
    ninfo = np.array([[100, 100, 100], [100, 100, 100], [0, 0, 0]])
    r = power.level_report(score, ninfo, 3.841)
    assert r["n_sites"].tolist() == [100, 100, 0] and r["score_self"].tolist() == [100, 90, 0]
    assert r["correct"].tolist() == [True, False, False] and r["n_ambiguous"].tolist() == [2, 1, 0] and r["unique"].tolist() == [False, False, False]
    assert r["best_other"].tolist() == [1, 0, -1] and r["best_other_ratio"][0] == 1.0 and r["best_other_ratio"][1] == 1.0 and np.isnan(r["best_other_ratio"][2])
    alone = power.level_report(np.array([[100, 50], [50, 100]]), np.full((2, 2), 100), 3.841)
    assert alone["unique"].tolist() == [True, True] and alone["best_other"].tolist() == [1, 0] and (alone["best_other_ratio"] > 3.841).all()
    one = power.level_report(np.array([[7]]), np.array([[7]]))
    assert one["unique"].tolist() == [True] and one["best_other"].tolist() == [-1]


# ------------------------------------------------------------------------------------------------ the library's validation
def test_refusals_that_need_no_device():
    lib = _lib.load()
    out = np.zeros((2, 2, 2, 2), dtype=np.int32)
    cols = np.zeros(2, dtype=np.int32)
    good = np.array([0, 2, 2, 5], dtype=np.int64)

    def call(ncols, n_rows, grp=good, n_grp=3, err_thr=0, outs=(0, 1), cols=cols):
        ptrs = [_lib.ptr(out[k]) if k is not None else None for k in outs]
        rc = lib.snpm_panel_sim_counts(None, _lib.ptr(cols), ncols, None, 0, n_rows, _lib.ptr(grp), n_grp, err_thr, 9, *ptrs)
        return rc, lib.snpm_last_error(None).decode()
    bad = _lib.SNPM_ERR_BADARG
    assert call(-1, 5) == (bad, "negative size") and call(2, -1) == (bad, "negative size")
    rc, msg = call(11553, 5)
    assert rc == bad and "too many accessions" in msg and "SNPM_SIM_MAX_ACCESSIONS" in msg
    rc, msg = call(2, 2 ** 31)
    assert rc == bad and "2^31 rows" in msg
    for n_grp in (0, -1, 65):
        assert call(2, 5, n_grp=n_grp) == (bad, "n_grp must be 1 .. 64")
    rc, msg = call(11552, 5, n_grp=17, grp=np.zeros(18, dtype=np.int64), cols=None)
    assert rc == bad and "n_grp * ncols * ncols" in msg and 17 * 11552 ** 2 >= 2 ** 31 > 16 * 11552 ** 2
    assert call(2, 5, grp=None) == (bad, "grp_off is NULL")
    assert call(2, 5, grp=np.array([1, 2, 2, 5])) == (bad, "grp_off must start at 0")
    assert call(2, 5, grp=np.array([0, 3, 2, 5])) == (bad, "grp_off must not decrease")
    assert call(2, 6) == (bad, "grp_off must end at n") and call(2, 4) == (bad, "grp_off must end at n")
    assert call(2, 5, err_thr=2 ** 32 + 1) == (bad, "err_thr must be 0 .. 2^32")
    for outs in ((None, 1), (0, None)):
        assert call(2, 5, outs=outs) == (bad, "score / ninfo is NULL")
    assert call(2, 5) == (bad, "panel is NULL")                                   # sound arguments: only the panel is missing
    assert call(2, 5, err_thr=2 ** 32) == (bad, "panel is NULL")                  # the limits are inclusive
    assert call(0, 5, outs=(None, None)) == (bad, "panel is NULL")
    assert call(2, 0, grp=np.zeros(65, dtype=np.int64), n_grp=64) == (bad, "panel is NULL")
    assert call(11552, 5, n_grp=16, grp=np.array([0] * 16 + [5]), cols=None) == (bad, "panel is NULL")
    header = open(os.path.join(ROOT, "include", "snpmatch_hip.h")).read()
    assert "#define SNPM_SIM_MAX_ACCESSIONS 11552" in header and engine.SIM_MAX_ACCESSIONS == 11552 and engine.SIM_MAX_GROUPS == 64
    assert "snpm_panel_sim_counts" in _lib.SYMBOLS
    kernel = open(os.path.join(ROOT, "snpmatch_amd", "csrc", "snpm_k_sim.hpp")).read()
    assert "#define SNPM_SIM_MAX_ACCESSIONS 11552" in kernel and "constexpr int SIM_MAX_GROUPS = 64;" in kernel and "asm" not in kernel
    assert not re.search(r"\b(float|double)\b", kernel)                          # integers only on the device


class _Holder(object):
    """stands in for a Genotype whose DB went to the given kind of panel"""

    def __init__(self, panel):
        self._panel = panel

    def panel(self):
        return self._panel


def test_group_and_streamed_panels_are_refused_with_the_reason():
    for cls, why in ((engine.GroupPanel, "spread over several GPUs"), (engine.StreamedPanel, "not a resident panel")):
        with pytest.raises(TypeError, match="sim_counts needs every accession column on one device") as err:
            engine.sim_counts(cls.__new__(cls), [0, 3], 0.0, 1)
        assert why in str(err.value)
    for cls, why in ((engine.GroupPanel, "spread over several GPUs by accession"), (engine.StreamedPanel, "streamed through the device")):
        with pytest.raises(TypeError, match="the power study needs every accession column of the DB on one device") as err:
            snp_genotype.Genotype.sim_counts(_Holder(cls.__new__(cls)), [0, 3], 0.0, 1)
        assert why in str(err.value)


# ------------------------------------------------------------------------------------------------ the command
@pytest.fixture
def planted(monkeypatch, tmp_path):
    """the planted DB as an .npz; the device call is the twin"""
    case = power_twin.planted_case()
    snps = case["snps"]
    db = str(tmp_path / "db.npz")
    np.savez(db, snps=snps, accessions=case["names"], positions=case["positions"], chrs=case["chrs"], chr_regions=case["chr_regions"])
    calls = []
    stub = engine.Panel.__new__(engine.Panel)
    stub.h = None

    def twin(panel, grp_off, err_rate, seed, cols=None, rows=None):
        calls.append((np.asarray(grp_off).tolist(), err_rate, seed, cols, rows))
        rows = np.arange(rows.start, rows.stop) if isinstance(rows, range) else rows
        return power_twin.sim_counts(snps, grp_off, power_twin.err_threshold(err_rate), seed, cols, rows)
    monkeypatch.setattr(snp_genotype.Genotype, "panel", lambda self, ctx=None, packed=None: stub)
    monkeypatch.setattr(engine, "sim_counts", twin)
    return case, db, calls


def test_command_on_the_planted_twins(planted, tmp_path):
    case, db, calls = planted
    a, b = power_twin.PLANTED_TWINS
    names = case["names"].tolist()
    out = str(tmp_path / "out")
    argv = ["power", "-d", db, "-n", "40,3000", "-p", str(power_twin.PLANTED_ERR), "--trials", "1", "--seed", "7", "-o", out]
    assert cli.main(argv) == 0
    assert len(calls) == 1 and calls[0][0] == [0, 40, 3000] and calls[0][1:4] == (power_twin.PLANTED_ERR, 7, None)
    rows, grp_off = power.draw_ladder(3000, [40, 3000], np.random.default_rng(7))
    assert np.array_equal(np.asarray(calls[0][4]), rows)
    lines = [ln.split("\t") for ln in open(out + ".power.tsv").read().splitlines()]
    assert lines[0] == ["trial", "level", "n_markers", "accession", "n_sites", "score_self", "correct", "n_ambiguous", "unique", "best_other", "best_other_ratio"]
    assert len(lines) == 1 + 2 * 12 and all(len(ln) == 11 for ln in lines)
    table = {(int(ln[1]), ln[3]): ln for ln in lines[1:]}
    for lev, unique, n_amb in ((40, "0", "2"), (3000, "1", "1")):
        for me, other in ((a, b), (b, a)):
            ln = table[(lev, names[me])]
            assert ln[6] == "1" and ln[7] == n_amb and ln[8] == unique and ln[9] == names[other]
    assert table[(40, names[a])][4:6] == ["38", "38"] and float(table[(40, names[a])][10]) == 1.0
    assert table[(3000, names[a])][4:6] == ["2889", "2881"] and table[(3000, names[b])][4:6] == ["2889", "2883"]
    assert 3.841 < float(table[(3000, names[a])][10]) < 6 and 3.841 < float(table[(3000, names[b])][10]) < 8
    assert all(ln[8] == "1" for ln in lines[1:] if ln[3] not in (names[a], names[b]))            # every other accession: unique from 40 markers on
    stats = json.load(open(out + ".power.json"))
    assert stats["levels"] == [40, 3000] and stats["n_markers"] == [40, 3000] and stats["trials"] == 1 and stats["accessions"] == 12
    assert stats["fraction_correct"] == [1.0, 1.0] and stats["fraction_unique"] == [10 / 12, 1.0]
    assert stats["unique_from_level"][names[a]] == 3000 and stats["unique_from_level"][names[b]] == 3000 and stats["unique_from_level"][names[0]] == 40
    assert stats["never_unique"] == [] and stats["confused_at_largest_level"] == []
    z = np.load(out + ".power.npz")
    score, ninfo = power_twin.sim_counts(case["snps"], grp_off, power_twin.err_threshold(power_twin.PLANTED_ERR), 7, None, rows)
    assert z["accessions"].tolist() == names and z["score"].dtype == np.int32 and z["levels"].tolist() == [40, 3000]
    assert np.array_equal(z["score"], np.cumsum(score, axis=0)) and np.array_equal(z["ninfo"], np.cumsum(ninfo, axis=0))
    # only the first level: the twins stay confused, and the summary names the pair in both directions
    assert cli.main(["power", "-d", db, "-n", "40", "-p", "0", "--trials", "2", "--seed", "7", "-o", out]) == 0
    stats = json.load(open(out + ".power.json"))
    assert calls[-1][2] == 8 and calls[-2][2] == 7 and stats["never_unique"] == [names[a], names[b]]
    both = [(c["sample"], c["taken_for"]) for c in stats["confused_at_largest_level"]]
    assert (names[a], names[b]) in both and (names[b], names[a]) in both
    # an accession list and a region: the call's columns and the candidate rows
    acc_file = tmp_path / "accs.txt"
    acc_file.write_text("%s\n%s\n%s\n" % (names[9], names[2], names[4]))
    assert cli.main(["power", "-d", db, "-a", str(acc_file), "--bed", "Chr1,100,5100", "-n", "10,500", "--trials", "1", "-o", out]) == 0
    assert calls[-1][3].tolist() == [9, 2, 4] and calls[-1][0] == [0, 10, 100] and np.asarray(calls[-1][4]).max() < 100
    assert np.load(out + ".power.npz")["accessions"].tolist() == [names[9], names[2], names[4]]
    assert cli.main(["power", "-d", db, "-n", "100,50", "-o", out]) == 2
    assert cli.main(["power", "-d", db, "-n", "100", "-p", "1.5", "-o", out]) == 2


# ------------------------------------------------------------------------------------------------ the kernels, on the host
def test_kernel_source_on_the_host_under_asan_and_ubsan(tmp_path):
    """every block of k_win_planes / k_sim_noise / k_sim_count run by 256 real threads with a barrier, exact-size heap buffers,
    arbitrary pad bytes, stale planes: 1 / 2 / 31 / 32 / 33 / 65 / 130 accessions x 0 / 1 / 63 / 64 / 65 / 1023 / 1024 / 1025 / 8191 /
    8192 / 8193 rows over the three layouts and the four error rates; one group, boundaries at 1 / 63 / 64 / 65 / 1024 / 8192 / 8193,
    three boundaries inside one word, empty groups first, in the middle and last, 64 groups; column lists with a repeat and unsorted
    row lists with repeats; two and three slabs; the split layout at 1135 accessions; the slab plan alone.  The hash table it prints
    is the C++ definition's: the twin's numpy restatement must give the same values"""
    cases = host_kernel_util.run_driver("sim_host_driver", tmp_path)
    hashes = [ln for ln in cases if ln.startswith("case hash ")]
    assert len(hashes) == 4 * 3 * 7
    seen = set()
    for ln in hashes:
        seed, a, k, h = (int(v) for v in re.match(r"case hash seed=(\d+) a=(\d+) k=(\d+) h=(\d+) ok", ln).groups())
        assert int(power_twin.sim_hash(seed, a, k)) == h == power_twin._scalar_hash(seed, a, k)
        seen.add((seed, a, k))
    assert (0, 0, 0) in seen and any(k >= 2 ** 32 for _, _, k in seen) and len({ln.split("h=")[1] for ln in hashes}) == len(hashes)
    runs = [ln for ln in cases if not ln.startswith(("case hash ", "case plan-"))]
    assert len(runs) == 77 + 12 + 2 + 4 + 3 + 3 + 2 and len(cases) == len(runs) + len(hashes) + 3
    assert sum(ln.startswith("case shape ") for ln in runs) == 77 and {re.search(r"layout=(\d)", ln).group(1) for ln in runs} == {"0", "1", "2"}
    assert sum("slabs=3" in ln for ln in runs) == 2 and sum("slabs=2" in ln for ln in runs) == 1
    assert sum("groups=64 " in ln for ln in runs) == 2 and sum("acc=1135 " in ln for ln in runs) == 2
    for thr in (0, power_twin.err_threshold(0.05), HALF, 1 << 32):
        assert sum("thr=%d " % thr in ln for ln in runs) >= 15
    assert not any("changed=0 " in ln for ln in runs if "thr=0 " not in ln and "rows=0 " not in ln and "rows=1 " not in ln)
