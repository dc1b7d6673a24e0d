"""Panel windows without a GPU: the numpy twin (tests/windows_twin.py), ``snp_genotype.het_from_counts`` / ``mismatch_from_counts``, the
``Genotype`` methods and the ``windows`` subcommand against the goldens of the unmodified reference (fp64 bits, ``nan`` where the
reference has ``nan``) with the twin in the place of the device call; the twin against a brute-force count; every refusal of
``snpm_panel_window_counts`` that needs no device; ``Genome.get_window_rows`` against ``get_bins_genome``; and the kernel source
itself, compiled for the host and run by real threads under AddressSanitizer + UBSan (tests/win_host_driver.cpp on
tests/host_kernel/, a child process), whose slab plans ``engine.window_slabs`` must reproduce."""
import glob
import json
import os

import numpy as np
import pytest

import host_kernel_util
import windows_twin
from snpmatch_amd import _lib, cli, engine
from snpmatch_amd.core import genomes, snp_genotype, windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["windows_a%d_w%d" % (a, w) for a in (2, 7) for w in (100, 300)]


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(b)
    return (a.dtype == np.float64 and a.shape == b.shape and np.array_equal(np.isnan(a), nan) and
            np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64)))


def toy_genome(golden_dir):
    return genomes.Genome(os.path.join(golden_dir, "windows_toy_genome.json"))


def selection(case):
    """the rows that lie in a window, window after window, and their offsets"""
    first, last = case["first"], case["last"]
    rows = np.concatenate([np.arange(a, b) for a, b in zip(first, last)])
    return rows, np.concatenate([[0], np.cumsum(last - first)])


def test_every_golden_is_listed(golden_dir):
    assert sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(golden_dir, "windows_*.npz"))) == sorted(CASES)


@pytest.mark.parametrize("name", CASES)
def test_twin_and_host_functions_against_the_reference(name, golden_dir):
    case = np.load(os.path.join(golden_dir, name + ".npz"))
    snps, pairs, listed = case["snps"], case["pairs"], case["listed"]
    assert snps.dtype == np.int8 and set(np.unique(snps).tolist()) == {-1, 0, 1, 2, 3}
    rows, win_off = selection(case)
    acc, pair = windows_twin.window_counts(snps, win_off, None, pairs, rows)
    assert acc.dtype == np.int32 and pair.dtype == np.int32 and acc.shape == (len(win_off) - 1, snps.shape[1], 4)
    for own in (snp_genotype.het_from_counts(acc), snp_genotype.het_from_counts(acc, 5), windows_twin.het(acc)):
        assert same_bits(own, case["het"])
    assert same_bits(snp_genotype.het_from_counts(windows_twin.window_counts(snps, win_off, listed, None, rows)[0]), case["het_listed"])
    assert same_bits(snp_genotype.mismatch_from_counts(pair), case["mismatch"]) and same_bits(windows_twin.mismatch(pair), case["mismatch"])
    # a higher minimum only blanks cells; the counts of a pair and its mirror are the same; summed over the windows they are kinship's
    more = snp_genotype.het_from_counts(acc, 9)
    assert np.array_equal(np.isnan(more), acc[:, :, 3] <= 9) and same_bits(more[~np.isnan(more)], case["het"][~np.isnan(more)])
    assert np.array_equal(pair[0], pair[1]) and np.array_equal(pair[2, :, 0], pair[2, :, 1])
    v = snps[rows].astype(int)
    hom = (v[:, 0] >= 0) & (v[:, 0] <= 1) & (v[:, 1] >= 0) & (v[:, 1] <= 1)
    assert pair[0, :, 2].sum() == (hom & (v[:, 0] == v[:, 1])).sum() and pair[0, :, 3].sum() == (hom & (v[:, 0] != v[:, 1])).sum()


def test_the_planted_windows_are_in_the_goldens(golden_dir):
    for name, acc, five, six, apart, gone, empty in (("windows_a7_w100", 0, "Chr1,201,300", "Chr1,301,400", "Chr1,501,600", "Chr1,101,200", "Chr1,401,500"),
                                                     ("windows_a2_w300", 1, "Chr1,601,900", "Chr2,1,300", "Chr2,601,900", "Chr2,301,600", "Chr1,901,1200")):
        case = np.load(os.path.join(golden_dir, name + ".npz"))
        at = {t: k for k, t in enumerate(case["index"].tolist())}
        rows, win_off = selection(case)
        counts, pair = windows_twin.window_counts(case["snps"], win_off, None, case["pairs"], rows)
        assert counts[at[five], acc, 3] == 5 and np.isnan(case["het"][at[five], acc])                   # y_min = 5: nan at 5 ...
        assert counts[at[six], acc, 3] == 6 and case["het"][at[six], acc] == counts[at[six], acc, 2] / 6.0 > 0      # ... a value at 6
        assert pair[0, at[apart], 0] == 0 and counts[at[apart], 0, 3] > 0 and np.isnan(case["mismatch"][0, at[apart]])
        assert win_off[at[gone] + 1] > win_off[at[gone]] and not counts[at[gone], :, 3].any() and np.isnan(case["het"][at[gone]]).all()
        assert win_off[at[empty] + 1] == win_off[at[empty]] and np.isnan(case["het"][at[empty]]).all() and np.isnan(case["mismatch"][:, at[empty]]).all()
        assert len(rows) < len(case["snps"]) and rows.max() < len(case["snps"]) - 2                       # rows past the last window of Chr2
        assert (case["snps"][rows] == 3).any()                                                           # code 3: informative for het, outside the mismatch


def test_twin_counts_against_a_brute_force_loop():
    rng = np.random.default_rng(61)
    for n_rows, n_acc, cols, rows, off, pairs in ((9, 5, None, None, [0, 0, 4, 4, 9, 9], [(0, 1), (1, 0), (3, 3)]),
                                                  (12, 37, [30, 2, 9, 17, 36, 2], None, [0, 12], [(0, 5), (1, 5), (5, 1)]),
                                                  (10, 33, None, [7, 7, 0, 9, 3, 3, 8], [0, 1, 2, 7], None),
                                                  (1, 4, None, None, [0, 1], [(0, 3)]), (6, 1, None, [], [0, 0], [(0, 0)])):
        snps = rng.choice(np.array([-1, 0, 1, 2, 3], dtype=np.int8), size=(n_rows, n_acc), p=[0.12, 0.42, 0.32, 0.09, 0.05])
        acc, pair = windows_twin.window_counts(snps, off, cols, pairs, rows)
        want_a, want_p = windows_twin.brute_counts(snps, off, cols, pairs, rows)
        assert np.array_equal(acc, want_a) and (pair is None or np.array_equal(pair, want_p))
    # hand-made: code 3 counts in ninfo only; het against het is equal and not homozygous
    snps = np.array([[2, 2, 3], [0, 1, 3], [1, 1, -1], [3, 0, 0], [-1, 2, 2]], dtype=np.int8)
    acc, pair = windows_twin.window_counts(snps, [0, 5], None, [(0, 1), (1, 2), (0, 2)])
    assert acc[0].tolist() == [[1, 1, 1, 4], [1, 2, 2, 5], [1, 0, 1, 4]]
    assert pair[:, 0].tolist() == [[3, 2, 1, 1], [2, 2, 1, 0], [0, 0, 0, 0]]
    assert windows_twin.mismatch(pair)[0, 0] == 1.0 - 2.0 / 3.0 and np.isnan(snp_genotype.mismatch_from_counts(pair)[2, 0])
    assert snp_genotype.het_from_counts(acc, 3)[0].tolist() == [0.25, 0.4, 0.25] and np.isnan(snp_genotype.het_from_counts(acc, 4)[0, [0, 2]]).all()


# ------------------------------------------------------------------------------------------------ the library's validation
def test_refusals_that_need_no_device():
    lib = _lib.load()
    cols, pa, pb = np.zeros(4, dtype=np.int32), np.zeros(2, dtype=np.int32), np.ones(2, dtype=np.int32)
    acc, pair, off = np.full((3, 4, 4), 7, dtype=np.int32), np.full((2, 3, 4), 7, dtype=np.int32), np.array([0, 2, 2, 5], dtype=np.int64)
    P = _lib.ptr

    def call(ncols=4, n_pairs=2, n_rows=5, off=off, n_win=3, acc=acc, pair=pair, pa=pa, pb=pb):
        rc = lib.snpm_panel_window_counts(None, P(cols), ncols, P(pa), P(pb), n_pairs, None, 0, n_rows, P(off), n_win, P(acc), P(pair))
        return rc, lib.snpm_last_error(None).decode()
    for bad in ({"ncols": -1}, {"n_pairs": -1}, {"n_rows": -1}, {"n_win": -1}):
        assert call(**bad) == (_lib.SNPM_ERR_BADARG, "negative size")
    assert call(off=None) == (_lib.SNPM_ERR_BADARG, "win_off is NULL")
    assert call(off=np.array([1, 2, 2, 5], dtype=np.int64)) == (_lib.SNPM_ERR_BADARG, "win_off must start at 0")
    assert call(off=np.array([0, 3, 2, 5], dtype=np.int64)) == (_lib.SNPM_ERR_BADARG, "win_off must not decrease")
    assert call(off=np.array([0, 2, 2, 4], dtype=np.int64)) == (_lib.SNPM_ERR_BADARG, "win_off must end at n")
    assert call(n_rows=6) == (_lib.SNPM_ERR_BADARG, "win_off must end at n")
    assert call(acc=None, pair=None) == (_lib.SNPM_ERR_BADARG, "acc_counts and pair_counts are both NULL")
    assert call(pa=None) == call(pb=None) == (_lib.SNPM_ERR_BADARG, "pair_a / pair_b is NULL")
    big = np.array([0, 2 ** 31], dtype=np.int64)
    assert call(n_rows=2 ** 31, off=big, n_win=1) == (_lib.SNPM_ERR_BADARG, "2^31 rows or more: the counts would not fit int32")
    rc, msg = call(ncols=engine.WIN_MAX_ACCESSIONS + 1)
    assert rc == _lib.SNPM_ERR_BADARG and "too many accessions" in msg and "SNPM_WIN_MAX_ACCESSIONS" in msg
    # sound arguments: only the panel is missing (one output is enough; none is needed without windows or columns; the limits are inclusive)
    assert call() == (_lib.SNPM_ERR_BADARG, "panel is NULL")
    assert call(acc=None) == call(pair=None) == call(n_pairs=0, pa=None, pb=None) == (_lib.SNPM_ERR_BADARG, "panel is NULL")
    assert call(n_win=0, off=np.array([0], dtype=np.int64), n_rows=0, acc=None, pair=None) == (_lib.SNPM_ERR_BADARG, "panel is NULL")
    assert call(ncols=0, n_pairs=0, acc=None, pair=None) == (_lib.SNPM_ERR_BADARG, "panel is NULL")
    assert call(ncols=engine.WIN_MAX_ACCESSIONS, n_rows=2 ** 31 - 1, off=np.array([0, 2 ** 31 - 1], dtype=np.int64), n_win=1) == (_lib.SNPM_ERR_BADARG, "panel is NULL")
    assert (acc == 7).all() and (pair == 7).all()
    header = open(os.path.join(ROOT, "include", "snpmatch_hip.h")).read()
    assert "#define SNPM_WIN_MAX_ACCESSIONS 4194240" in header and engine.WIN_MAX_ACCESSIONS == 4194240 == 65535 * 64 >= 16384
    kernel = open(os.path.join(ROOT, "snpmatch_amd", "csrc", "snpm_k_win.hpp")).read()
    assert "#define SNPM_WIN_MAX_ACCESSIONS 4194240" in kernel
    assert "snpm_panel_window_counts" in _lib.SYMBOLS


class _Holder(object):
    """stands in for a Genotype whose DB went to the given kind of panel"""

    def __init__(self, panel):
        self._panel = panel

    def panel(self):
        return self._panel


def test_group_and_streamed_panels_are_refused_with_the_reason_and_the_python_checks():
    for cls, why in ((engine.GroupPanel, "spread over several GPUs"), (engine.StreamedPanel, "not a resident panel")):
        with pytest.raises(TypeError, match="every accession column on one device") as err:
            engine.window_counts(cls.__new__(cls), [0, 5])
        assert why in str(err.value)
    for cls, why in ((engine.GroupPanel, "spread over several GPUs by accession"), (engine.StreamedPanel, "streamed through the device")):
        with pytest.raises(TypeError, match="every accession column of the DB on one device") as err:
            snp_genotype.Genotype.window_counts(_Holder(cls.__new__(cls)), [0, 5])
        assert why in str(err.value)
    panel = engine.Panel.__new__(engine.Panel)
    panel.h, panel.n_snp, panel.n_acc = None, 60, 40
    with pytest.raises(TypeError, match="must be integers"):
        engine.window_counts(panel, [0, 60], np.array([0.5]))
    with pytest.raises(TypeError, match="integer indices into the column list"):
        engine.window_counts(panel, [0, 60], None, np.array([[0.5, 1.0]]))
    with pytest.raises(ValueError, match="neither acc_counts nor pairs"):
        engine.window_counts(panel, [0, 60], acc_counts=False)
    with pytest.raises(ValueError, match="n_win \\+ 1 entries"):
        engine.window_counts(panel, [])
    with pytest.raises(ValueError, match="step 1"):
        engine.window_counts(panel, [0, 5], None, None, range(0, 10, 2))


# ------------------------------------------------------------------------------------------------ the windows of a genome
def _bins_as_arrays(genome, g, bin_len):
    bins = list(genome.get_bins_genome(g, bin_len))
    return ([b[0] for b in bins], [b[1][0] for b in bins], [b[1][1] for b in bins], [list(b[2]) for b in bins])


def test_window_rows_against_get_bins_genome(golden_dir):
    case = np.load(os.path.join(golden_dir, "windows_a2_w100.npz"))
    g = snp_genotype.MemGenotype(case["snps"], ["A", "B"], case["positions"], ["Chr1", "Chr2"], case["chr_regions"])
    toy = toy_genome(golden_dir)
    for bin_len in (100, 300, 7, 1000, 5000):
        chr_ix, start, end, first, last = toy.get_window_rows(g, bin_len)
        want = _bins_as_arrays(toy, g, bin_len)
        assert (chr_ix.tolist(), start.tolist(), end.tolist()) == want[:3] and [list(range(a, b)) for a, b in zip(first, last)] == want[3]
        assert all(a.dtype == np.int64 for a in (chr_ix, start, end, first, last))
    for key, bin_len in (("windows_a2_w100", 100), ("windows_a7_w300", 300)):      # the reference's own member lists
        case = np.load(os.path.join(golden_dir, key + ".npz"))
        got = toy.get_window_rows(g, bin_len)
        assert all(np.array_equal(a, case[k]) for a, k in zip(got, ("chr_ix", "start", "end", "first", "last")))
    # TAIR10 with random positions; a DB without Chr3 and with its chromosomes in another order
    tair = genomes.Genome("athaliana_tair10")
    rng = np.random.default_rng(62)
    names, parts, regions, at = ["Chr2", "Chr1", "Chr5", "Chr4"], [], [], 0
    for name in names:
        length = int(tair.chrlen[tair.get_chr_ind(name)])
        pos = np.sort(rng.choice(np.arange(1, length + 1), size=int(rng.integers(1500, 4000)), replace=False))
        parts.append(pos)
        regions.append([at, at + len(pos)])
        at += len(pos)
    g = snp_genotype.MemGenotype(np.zeros((at, 1), dtype=np.int8), ["A"], np.concatenate(parts), names, regions)
    for bin_len in (300000, 123457):
        chr_ix, start, end, first, last = tair.get_window_rows(g, bin_len)
        want = _bins_as_arrays(tair, g, bin_len)
        assert (chr_ix.tolist(), start.tolist(), end.tolist()) == want[:3] and [list(range(a, b)) for a, b in zip(first, last)] == want[3]
        gone = chr_ix == tair.get_chr_ind("Chr3")
        assert gone.any() and (first[gone] == last[gone]).all()
        for c in set(chr_ix[~gone].tolist()):
            w = np.flatnonzero(chr_ix == c)
            assert np.array_equal(first[w][1:], last[w][:-1])       # the windows of a chromosome follow each other in the rows
    # a chromosome of the DB that the genome does not have: its rows are in no window, and Chr2 has windows without rows
    other = snp_genotype.MemGenotype(np.zeros((7, 1), dtype=np.int8), ["A"], np.array([5, 150, 990, 3, 8, 20, 640]), ["Chr1", "Chr9"], [[0, 3], [3, 7]])
    chr_ix, start, end, first, last = toy.get_window_rows(other, 100)
    want = _bins_as_arrays(toy, other, 100)
    assert (chr_ix.tolist(), start.tolist(), end.tolist()) == want[:3] and [list(range(a, b)) for a, b in zip(first, last)] == want[3]
    assert (last - first).sum() == 3 and last.max() == 3 and (first[chr_ix == 1] == last[chr_ix == 1]).all()
    bad = snp_genotype.MemGenotype(np.zeros((3, 1), dtype=np.int8), ["A"], np.array([5, 4, 9]), ["Chr1"], [[0, 3]])
    with pytest.raises(ValueError, match="not sorted"):
        toy.get_window_rows(bad, 100)


# ------------------------------------------------------------------------------------------------ Genotype and the command
def _genotype(case, monkeypatch):
    """the golden's DB as a Genotype whose device call is the twin; the calls are recorded"""
    snps = case["snps"]
    names = ["acc%02d" % i for i in range(snps.shape[1])]
    g = snp_genotype.Genotype.from_arrays(snps, names, case["positions"], ["Chr1", "Chr2"], case["chr_regions"])
    calls = []

    def twin(panel, win_off, cols=None, pairs=None, rows=None, acc_counts=True):
        calls.append((np.asarray(win_off).tolist(), cols, pairs, rows))
        a, p = windows_twin.window_counts(snps, win_off, cols, pairs, rows)
        return (a if acc_counts else None), p
    stub = engine.Panel.__new__(engine.Panel)
    stub.h = None
    monkeypatch.setattr(snp_genotype.Genotype, "panel", lambda self, ctx=None, packed=None: stub)
    monkeypatch.setattr(engine, "window_counts", twin)
    return g, names, calls


@pytest.mark.parametrize("name", CASES)
def test_genotype_methods_with_the_twin_as_device(name, golden_dir, monkeypatch):
    case = np.load(os.path.join(golden_dir, name + ".npz"))
    win = int(name.split("_w")[1])
    g, names, calls = _genotype(case, monkeypatch)
    toy = toy_genome(golden_dir)
    frame = g.calculate_heterozygosity_windows(toy, win)
    regions = case["chr_regions"].tolist()
    assert len(calls) == 2 and [c[3] for c in calls] == [range(0, regions[0][1]), range(regions[1][0], int(case["last"][-1]))]      # a range per chromosome
    assert list(frame.index) == case["index"].tolist() and list(frame.columns) == list(range(case["snps"].shape[1])) and all(str(t) == "float64" for t in frame.dtypes)
    assert same_bits(frame.to_numpy(), case["het"])
    listed = g.calculate_heterozygosity_windows(toy, win, case["listed"])
    assert list(listed.columns) == case["listed"].tolist() and same_bits(listed.to_numpy(), case["het_listed"])
    for i, (x, y) in enumerate(case["pairs"].tolist()):
        frame = g.mismatch_between_accs(x, y, win, toy)
        assert list(frame.columns) == ["chr", "start", "end", "mismatch"] and all(str(t) == "object" for t in frame.dtypes)
        assert list(frame["chr"]) == [["Chr1", "Chr2"][c] for c in case["chr_ix"]] and list(frame["start"]) == case["start"].tolist() and list(frame["end"]) == case["end"].tolist()
        assert same_bits(frame["mismatch"].to_numpy(dtype=np.float64), case["mismatch"][i])
        assert calls[-1][1].tolist() == [x, y] and calls[-1][2] == [[0, 1]]
        n_calls = len(calls)
        assert same_bits(g.mismatch_between_accs(x, y), case["mismatch_rows"][i]) and len(calls) == n_calls      # host work: no device call
    with pytest.raises(AssertionError, match="interger"):
        g.mismatch_between_accs(0, 1, 100.0, toy)
    with pytest.raises(AssertionError, match="genome class"):
        g.mismatch_between_accs(0, 1, 100, "athaliana_tair10")
    with pytest.raises(AssertionError, match="genome class"):
        g.calculate_heterozygosity_windows("athaliana_tair10", 100)


def test_command_line_writes_its_files(golden_dir, tmp_path, monkeypatch):
    case = np.load(os.path.join(golden_dir, "windows_a7_w100.npz"))
    g, names, calls = _genotype(case, monkeypatch)
    monkeypatch.setattr(snp_genotype, "Genotype", lambda hdf5_file, hdf5_acc_file: g)
    db = tmp_path / "db.npz"
    db.write_bytes(b"")
    out, toy_json = str(tmp_path / "out"), os.path.join(golden_dir, "windows_toy_genome.json")
    rows, win_off = selection(case)
    # all accessions, no pairs
    assert cli.main(["windows", "-d", str(db), "--genome", toy_json, "-b", "100", "-o", out]) == 0
    z = np.load(out + ".windows.npz")
    counts = windows_twin.window_counts(case["snps"], win_off, None, None, rows)[0]
    assert np.array_equal(z["counts"], counts) and same_bits(z["het"], case["het"]) and z["accessions"].tolist() == names
    assert z["chr"].tolist() == [["Chr1", "Chr2"][c] for c in case["chr_ix"]] and np.array_equal(z["start"], case["start"]) and np.array_equal(z["end"], case["end"])
    assert np.array_equal(z["n_rows"], case["last"] - case["first"]) and "pairs" not in z.files and not os.path.exists(out + ".pair_windows.tsv")
    lines = open(out + ".het_windows.tsv").read().splitlines()
    assert lines[0].split("\t") == ["window"] + names and [ln.split("\t")[0] for ln in lines[1:]] == case["index"].tolist()
    assert same_bits(np.array([[float(v) for v in ln.split("\t")[1:]] for ln in lines[1:]]), case["het"])           # repr precision: the bits come back
    stats = json.load(open(out + ".windows.json"))
    assert stats["windows"] == 17 and stats["windows_without_rows"] == 2 and stats["min_sites"] == 5 and stats["pairs"] == []
    judged = counts[:, 0, 3] > 5
    assert stats["accessions"]["acc00"] == {"windows_judged": int(judged.sum()), "mean_het": float(case["het"][judged, 0].mean())}
    # the duplicates file of kinship as the pair list, an accession list, another threshold
    pairs_file = tmp_path / "x.duplicates.tsv"
    pairs_file.write_text("acc_1\tacc_2\tsame\tdiff\tninfo\tidentity\tkinship\nacc05\tacc02\t9\t0\t9\t1.0\t1.0\nacc02\tacc05\t9\t0\t9\t1.0\t1.0\nacc06\tacc06\t1\t0\t1\t1.0\t1.0\n")
    acc_file = tmp_path / "accs.txt"
    acc_file.write_text("acc06\nacc02\nacc00\nacc05\n")
    assert cli.main(["windows", "-d", str(db), "-a", str(acc_file), "--pairs", str(pairs_file), "--genome", toy_json, "-b", "100", "--min_sites", "2", "-o", out]) == 0
    assert calls[-1][1].tolist() == [6, 2, 0, 5] and calls[-1][2].tolist() == [[3, 1], [1, 3], [0, 0]]
    want_a, want_p = windows_twin.window_counts(case["snps"], win_off, [6, 2, 0, 5], [(3, 1), (1, 3), (0, 0)], rows)
    z = np.load(out + ".windows.npz")
    assert np.array_equal(z["counts"], want_a) and np.array_equal(z["pair_counts"], want_p) and z["pairs"].tolist() == [["acc05", "acc02"], ["acc02", "acc05"], ["acc06", "acc06"]]
    assert same_bits(z["het"], windows_twin.het(want_a, 2)) and same_bits(z["mismatch"], windows_twin.mismatch(want_p)) and same_bits(z["mismatch"][0], case["mismatch"][3])
    lines = [ln.split("\t") for ln in open(out + ".pair_windows.tsv").read().splitlines()]
    assert lines[0] == ["acc_1", "acc_2", "chr", "start", "end", "n", "eq", "mismatch", "hom_same", "hom_diff"] and len(lines) == 1 + 3 * 17
    assert lines[1][:5] == ["acc05", "acc02", "Chr1", "1", "100"] and [int(v) for v in lines[1][5:7] + lines[1][8:]] == want_p[0, 0].tolist()
    assert same_bits(np.array([float(ln[7]) for ln in lines[1:18]]), case["mismatch"][3])
    stats = json.load(open(out + ".windows.json"))
    ok = want_p[2, :, 0] > 2
    assert stats["pairs"][2] == {"acc_1": "acc06", "acc_2": "acc06", "windows_judged": int(ok.sum()), "windows_identical": int(ok.sum())}
    assert stats["pairs"][0]["windows_identical"] == int((windows_twin.mismatch(want_p)[0][want_p[0, :, 0] > 2] == 0).sum())
    # --pairs_only: the columns are the pairs' members, in the order they are first named
    assert cli.main(["windows", "-d", str(db), "--pairs", str(pairs_file), "--pairs_only", "--genome", toy_json, "-b", "100", "-o", out]) == 0
    assert calls[-1][1].tolist() == [5, 2, 6] and calls[-1][2].tolist() == [[0, 1], [1, 0], [2, 2]]
    z = np.load(out + ".windows.npz")
    assert z["accessions"].tolist() == ["acc05", "acc02", "acc06"] and np.array_equal(z["pair_counts"], want_p) and z["counts"].shape == (17, 3, 4)


def test_command_line_refusals(golden_dir, tmp_path, monkeypatch, caplog):
    case = np.load(os.path.join(golden_dir, "windows_a7_w300.npz"))
    g, names, calls = _genotype(case, monkeypatch)
    monkeypatch.setattr(snp_genotype, "Genotype", lambda hdf5_file, hdf5_acc_file: g)
    db = tmp_path / "db.npz"
    db.write_bytes(b"")
    out, toy_json = str(tmp_path / "out"), os.path.join(golden_dir, "windows_toy_genome.json")
    pairs_file = tmp_path / "pairs.tsv"
    pairs_file.write_text("acc01 acc03\nacc01 nobody\n")
    acc_file = tmp_path / "accs.txt"
    acc_file.write_text("acc01\nacc02\n")
    base = ["windows", "-d", str(db), "--genome", toy_json, "-o", out]
    assert cli.main(base + ["--pairs", str(pairs_file)]) == 2 and "not among the selected accessions: nobody" in caplog.text
    assert cli.main(base + ["--pairs", str(pairs_file), "-a", str(acc_file)]) == 2 and "not among the selected accessions: acc03, nobody" in caplog.text
    assert cli.main(base + ["--pairs_only"]) == 2 and "--pairs_only needs --pairs" in caplog.text
    assert cli.main(base + ["-b", "0"]) == 2 and "at least 1" in caplog.text
    assert cli.main(base + ["--min_sites", "-1"]) == 2 and "must not be negative" in caplog.text
    pairs_file.write_text("acc01\n")
    assert cli.main(base + ["--pairs", str(pairs_file)]) == 2 and "expected two accession names" in caplog.text
    pairs_file.write_text("acc_1\tacc_2\n")
    assert cli.main(base + ["--pairs", str(pairs_file)]) == 2 and "names no pair" in caplog.text
    assert not calls and not os.path.exists(out + ".windows.npz")
    assert windows.read_pairs(str(pairs_file)) == []


# ------------------------------------------------------------------------------------------------ the kernels, on the host
def test_kernel_source_on_the_host_under_asan_and_ubsan(tmp_path):
    """every block of k_win_planes and k_win_count (256 threads) run by real threads with a barrier, exact-size heap buffers,
    arbitrary pad bytes, stale workspaces: 1 / 2 / 63 / 64 / 65 / 130 / 1135 accessions over the four layouts on a table with window
    edges at bits 0, 1, 63, 64 and 65 of a word, empty windows first, in the middle and last and a one-row window; no row, one row;
    one window holding all rows; a window longer than a plane step; columns only, pairs only, both; pairs (a, a), (a, b) and (b, a);
    a column list with a repeat; a row list that is unsorted with a repeat; groups of 1 to 64 lanes per cell; two and three slabs
    with a window across every slab edge.  The slab plan of every case is the library's, and engine.window_slabs agrees with it."""
    cases = host_kernel_util.run_driver("win_host_driver", tmp_path)
    field = lambda ln, key: ln.split(key + "=")[1].split()[0]      # noqa: E731
    runs = [ln for ln in cases if not ln.startswith("case plan")]
    plans = [ln for ln in cases if ln.startswith("case plan")]
    assert len(runs) == 28 + 4 + 4 + 3 + 4 + 6 and len(plans) == 5
    edges = [ln for ln in runs if ln.startswith("case edges ")]
    assert {(int(field(ln, "acc")), int(field(ln, "layout"))) for ln in edges} == {(a, l) for a in (1, 2, 63, 64, 65, 130, 1135) for l in range(4)}
    assert {int(field(ln, "outs")) for ln in edges} == {1, 2, 3} and {int(field(ln, "rows")) for ln in runs} >= {0, 1, 64, 65}
    assert sum(int(field(ln, "slabs")) == 2 for ln in runs) == 2 and sum(int(field(ln, "slabs")) == 3 for ln in runs) == 4
    assert sum(int(field(ln, "list")) for ln in runs) >= 5 and any(int(field(ln, "cols")) < int(field(ln, "acc")) for ln in runs)
    lgs = 0
    for ln in runs:
        lgs |= int(field(ln, "lgs"))
    assert lgs == 127                        # every group size, 1 to 64 lanes
    for ln in plans:                        # the Python form of the plan, on the driver's table
        ws, ncols, cells, n_rows, stride, n_win = (int(field(ln, k)) for k in ("ws", "ncols", "cells", "rows", "stride", "nwin"))
        off = [min(w * stride, n_rows) for w in range(n_win)] + [n_rows]
        want = [tuple(int(v) for v in s.split(":")) for s in field(ln, "slabs").split(",")]
        assert engine.window_slabs(ws, ncols, cells, off, n_rows) == want, ln
    assert len(field(plans[1], "slabs").split(",")) == 24 and field(plans[2], "slabs") == "0:1:0:4"      # 1135 x 11M at 256 MiB; an empty last window is in no slab
