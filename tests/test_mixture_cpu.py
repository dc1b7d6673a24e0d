"""mixture without a GPU: the numpy twin (tests/mixture_twin.py) against the three-loop form, on a hand-made matrix and on random
panels; ``mix_fill_masks`` against bit slices formed in numpy; ``fit_pairs`` against the plain Python loop; ``read_allele_depths`` on
the golden VCF and on in-test text, with every refusal; every refusal of ``snpm_panel_mix_counts`` that needs no device; the
``mixture`` subcommand with the twin in the place of the device on a planted pool; and the kernel source itself, compiled for the
host and run by 256 real threads per block under AddressSanitizer + UBSan (tests/mix_host_driver.cpp on tests/host_kernel/, a child
process)."""
import gzip
import json
import os
import re

import numpy as np
import pytest

import host_kernel_util
import mixture_twin
from snpmatch_amd import _lib, cli, engine
from snpmatch_amd.core import mixture, snp_genotype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES = np.array([-1, 0, 1, 2, 3], dtype=np.int8)


# ------------------------------------------------------------------------------------------------ the twin
def test_twin_on_a_hand_made_matrix():
    snps = np.array([[0, 0, 1], [1, 0, -1], [1, 1, 0], [0, 2, 0], [3, 1, 1], [1, 1, 1]], dtype=np.int8)
    alt, ref = np.array([1, 2, 3, 4, 5, 6]), np.array([10, 20, 30, 40, 50, 60])
    table = mixture_twin.mix_counts(snps, alt, ref)
    assert table.dtype == np.int32 and table.shape == (2, 2, 2, 3, 3)
    # alt reads, [ca][cb] of each ordered pair: e.g. (0, 1): rows 0 (0, 0), 1 (1, 0), 2 (1, 1), 5 (1, 1); row 3 has a het, row 4 "other"
    assert table[0, :, :, 0, 1].tolist() == [[1, 0], [2, 9]] and table[1, :, :, 0, 1].tolist() == [[10, 0], [20, 90]]
    assert table[0, :, :, 0, 2].tolist() == [[4, 1], [3, 6]] and table[1, :, :, 0, 2].tolist() == [[40, 10], [30, 60]]
    assert table[0, :, :, 1, 2].tolist() == [[0, 1], [3, 11]] and table[1, :, :, 1, 2].tolist() == [[0, 10], [30, 110]]
    # the diagonal: every column on its own, nothing off the diagonal of the 2 x 2
    assert table[0, :, :, 0, 0].tolist() == [[5, 0], [0, 11]] and table[0, :, :, 1, 1].tolist() == [[3, 0], [0, 14]]
    assert table[1, :, :, 2, 2].tolist() == [[70, 0], [0, 120]]
    assert np.array_equal(table, mixture_twin.mix_counts_direct(snps, alt, ref))
    sub = mixture_twin.mix_counts(snps, alt[[5, 5, 1]], ref[[5, 5, 1]], cols=[1, 0, 1], rows=[5, 5, 1])      # repeats count as listed
    assert sub[0, :, :, 0, 1].tolist() == [[0, 2], [0, 12]] and np.array_equal(sub[:, :, :, 0, 2], sub[:, :, :, 0, 0])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_twin_equals_the_direct_form_and_is_symmetric(seed):
    rng = np.random.default_rng(seed)
    snps = rng.choice(CODES, size=(90, 7), p=[.1, .4, .35, .1, .05])
    alt, ref = rng.integers(0, 256, 90), rng.integers(0, 16, 90)
    table = mixture_twin.mix_counts(snps, alt, ref)
    assert np.array_equal(table, mixture_twin.mix_counts_direct(snps, alt, ref))
    assert np.array_equal(table, table.transpose(0, 2, 1, 4, 3))                # T[w][ca][cb][a][b] == T[w][cb][ca][b][a]
    for c in (0, 1):                                                            # the diagonal gives the singles
        for w, reads in enumerate((alt, ref)):
            assert np.array_equal(np.diagonal(table[w, c, c]), ((snps == c) * reads[:, None]).sum(axis=0))
        assert not np.diagonal(table[:, c, 1 - c], axis1=1, axis2=2).any()
    cols, rows = np.array([4, 0, 4, 6]), rng.integers(0, 90, size=50)
    sub = mixture_twin.mix_counts(snps, alt[rows], ref[rows], cols, rows)
    assert np.array_equal(sub, mixture_twin.mix_counts_direct(snps[rows][:, cols], alt[rows], ref[rows]))


# ------------------------------------------------------------------------------------------------ the fit
def test_fit_pairs_equals_the_scalar_loop():
    rng = np.random.default_rng(11)
    snps = rng.choice(np.array([-1, 0, 1], dtype=np.int8), size=(4000, 9), p=[.06, .5, .44])
    f = 0.7 * snps[:, 2].clip(0) + 0.3 * snps[:, 5].clip(0)
    depth = rng.poisson(4.0, 4000)
    alt = rng.binomial(depth, f * 0.98 + 0.01)
    table = mixture_twin.mix_counts(snps, alt, depth - alt)
    table[0, 0, 0, 8, 8] = 2 ** 31 - 1                                          # the largest cell the table can hold
    grid = mixture.alpha_grid(0.01)
    assert len(grid) == 51 and grid[0] == 0.0 and grid[-1] == 0.5
    fit = mixture.fit_pairs(table, 0.01, grid)
    for a in range(9):
        for b in range(9):
            alpha, ll, ll0, lls = mixture_twin.fit_scalar(table[:, :, :, a, b], 0.01, grid)
            ranked = sorted(lls, reverse=True)
            if a != b:                      # no tie between the two best LLs of the scalar form at the tolerance of the comparison
                assert ranked[0] - ranked[1] > 1e-13 * abs(ranked[0]), (a, b)
                assert fit["alpha"][a, b] == alpha, (a, b)
            assert fit["ll"][a, b] == pytest.approx(ll, rel=1e-13, abs=0.0)
            assert fit["ll"][a, b] - fit["llr"][a, b] == pytest.approx(ll0, rel=1e-13, abs=0.0)
            assert fit["reads"][a, b] == int(table[:, :, :, a, b].astype(np.int64).sum())
        assert fit["single_ll"][a] == pytest.approx(mixture_twin.fit_scalar(table[:, :, :, a, a], 0.01, grid)[2], rel=1e-13, abs=0.0)
        assert fit["single_reads"][a] == fit["reads"][a, a]
    assert fit["alpha"][2, 5] == pytest.approx(0.3, abs=0.03) and fit["alpha"][5, 2] == 0.5 and fit["reads"].dtype == np.int64
    assert mixture.shortlist(fit, 200, 3)[0] == (2, 5) and mixture.verdict_of(fit, [(2, 5)]) == "mixture"
    # blocks of accession rows: a temporary budget of one row at a time gives the same bits
    small = mixture.FIT_BLOCK_BYTES
    try:
        mixture.FIT_BLOCK_BYTES = 8 * 51 * 9
        again = mixture.fit_pairs(table, 0.01, grid)
    finally:
        mixture.FIT_BLOCK_BYTES = small
    assert all(np.array_equal(fit[k], again[k]) for k in fit)


def test_shortlist_ties_go_to_the_lower_columns_and_min_reads_counts():
    n = 4
    fit = {"reads": np.full((n, n), 100, dtype=np.int64), "ll": np.full((n, n), -50.0), "llr": np.zeros((n, n)), "alpha": np.zeros((n, n)),
           "single_ll": np.full(n, -50.0), "single_reads": np.full(n, 100, dtype=np.int64)}
    fit["ll"][2, 1] = -40.0
    fit["reads"][0, 3] = 99
    assert mixture.shortlist(fit, 100, 4) == [(2, 1), (0, 1), (0, 2), (1, 0)]
    assert (0, 3) not in mixture.shortlist(fit, 100, 100) and len(mixture.shortlist(fit, 100, 100)) == 11
    assert mixture.shortlist(fit, 101, 5) == [] and mixture.verdict_of(fit, []) == "no_call" and mixture.best_single(fit, 101) is None
    assert mixture.best_single(fit, 100) == 0
    for step in (0.0, -0.1, 0.3, 0.0001, 0.6):
        with pytest.raises(ValueError, match="--grid must divide 0.5"):
            mixture.alpha_grid(step)


# ------------------------------------------------------------------------------------------------ the reader
def test_read_allele_depths_on_the_golden_vcf(golden_dir):
    path = os.path.join(golden_dir, "701_501.filter.vcf.gz")
    want = {"records": 0, "kept": 0, "multi": 0, "no_ad": 0, "zero": 0}
    first = []
    with gzip.open(path, "rt") as fh:
        for line in fh:
            if line.startswith("#"):
                continue
            f = line.rstrip("\n").split("\t")
            want["records"] += 1
            keys, vals = f[8].split(":"), f[9].split(":")
            ad = vals[keys.index("AD")] if "AD" in keys and keys.index("AD") < len(vals) else None
            if "," in f[4] or f[4] == ".":
                want["multi"] += 1
            elif ad is None or not re.fullmatch(r"\d+,\d+", ad):
                want["no_ad"] += 1
            elif sum(int(x) for x in ad.split(",")) < 1:
                want["zero"] += 1
            else:
                want["kept"] += 1
                first.append((f[0], int(f[1]), ad))
    got = mixture.read_allele_depths(path)
    assert want["records"] == 10000 and want["kept"] > 5000
    assert got["records"] == want["records"] and len(got["pos"]) == want["kept"] and got["sample"] == "701_501"
    assert got["dropped"] == {"multi_allelic": want["multi"], "no_ad": want["no_ad"], "zero_depth": want["zero"]}
    assert [ad for _, _, ad in first[:3]] == ["3,0", "4,0", "3,0"]
    assert got["ref"][:3].tolist() == [3, 4, 3] and got["alt"][:3].tolist() == [0, 0, 0] and got["pos"][:3].tolist() == [13226, 21006, 42291]
    assert got["chr"].tolist() == [c for c, _, _ in first] and got["pos"].tolist() == [p for _, p, _ in first]
    assert ["%d,%d" % (r, a) for r, a in zip(got["ref"], got["alt"])] == [ad for _, _, ad in first]
    assert got["pos"].dtype == np.int64 and got["ref"].dtype == np.int64 and (got["ref"] + got["alt"] >= 1).all()
    assert mixture.read_allele_depths(path, "701_501")["pos"].tolist() == got["pos"].tolist()


VCF_HEAD = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tone\ttwo\n"
VCF_BODY = [
    "Chr1\t10\t.\tA\tT\t9\t.\tDP=3\tGT:AD:DP\t0/0:3,0:3\t0/1:1,2:3",
    "Chr1\t20\t.\tA\tT,G\t9\t.\tDP=3\tGT:AD:DP\t0/1:1,1,1:3\t0/2:1,0,2:3",          # two ALT alleles
    "Chr1\t30\t.\tA\tT\t9\t.\tDP=3\tGT:AD:DP\t./.:.,.:.\t./.:0,4:4",                # '.' entries / a count without a called GT
    "Chr1\t40\t.\tA\tT\t9\t.\tDP=3\tGT:AD:DP\t./.\t1/1:0,7:7",                      # the entry ends before AD
    "Chr1\t50\t.\tA\tT\t9\t.\tDP=3\tGT:DP\t0/0:3\t0/0:3",                           # FORMAT without AD
    "Chr1\t60\t.\tA\tT\t9\t.\tDP=0\tGT:AD:DP\t./.:0,0:0\t0/0:300,1:301",            # no read / more than a byte holds
    "Chr2\t70\t.\tA\tT\t9\t.\tDP=3\tGT:AD:DP\t1/1:0,5:5",                           # the second sample column is missing
    "Chr2\t80\t.\tA\t.\t9\t.\tDP=3\tGT:AD:DP\t0/0:5:5\t0/0:6:6",                    # no ALT allele: one AD entry
    "Chr2\t90\t.\tA\tT\t9\t.\tDP=3\tGT:AD:DP\t0/1:2,x:3\t0/1:2,3:5",                # not an integer
]


def test_read_allele_depths_on_in_test_text_and_every_refusal(tmp_path):
    vcf = tmp_path / "two.vcf"
    vcf.write_text(VCF_HEAD + "\n".join(VCF_BODY) + "\n")
    one = mixture.read_allele_depths(str(vcf))
    assert one["sample"] == "one" and one["records"] == 9
    assert (one["chr"].tolist(), one["pos"].tolist(), one["ref"].tolist(), one["alt"].tolist()) == (["Chr1", "Chr2"], [10, 70], [3, 0], [0, 5])
    assert one["dropped"] == {"multi_allelic": 2, "no_ad": 4, "zero_depth": 1}
    for which in (1, "1", "two"):
        two = mixture.read_allele_depths(str(vcf), which)
        assert two["sample"] == "two" and two["pos"].tolist() == [10, 30, 40, 60, 90]
        assert two["ref"].tolist() == [1, 0, 0, 300, 2] and two["alt"].tolist() == [2, 4, 7, 1, 3]
        assert two["dropped"] == {"multi_allelic": 2, "no_ad": 2, "zero_depth": 0}
    gz = tmp_path / "two.vcf.gz"
    with gzip.open(str(gz), "wt") as fh:
        fh.write(VCF_HEAD + "\n".join(VCF_BODY) + "\n")
    assert mixture.read_allele_depths(str(gz), "two")["alt"].tolist() == [2, 4, 7, 1, 3]
    with pytest.raises(ValueError, match="has no sample column named three"):
        mixture.read_allele_depths(str(vcf), "three")
    with pytest.raises(ValueError, match="has 2 sample columns: --sample 2 is outside"):
        mixture.read_allele_depths(str(vcf), 2)
    plain = tmp_path / "plain.vcf"
    plain.write_text(VCF_HEAD + VCF_BODY[4] + "\n")
    with pytest.raises(ValueError, match="no record's FORMAT carries AD"):
        mixture.read_allele_depths(str(plain))
    with pytest.raises(ValueError, match="a BED file holds genotype calls, not read counts"):
        mixture.read_allele_depths(str(tmp_path / "sample.bed"))
    with pytest.raises(ValueError, match="the .npz cache of a parsed sample keeps GT and PL"):
        mixture.read_allele_depths(str(tmp_path / "sample.vcf.snpmatch.npz"))
    with pytest.raises(ValueError, match="mixture reads a VCF"):
        mixture.read_allele_depths(str(tmp_path / "sample.txt"))
    headless = tmp_path / "headless.vcf"
    headless.write_text(VCF_BODY[0] + "\n")
    with pytest.raises(ValueError, match="no #CHROM line"):
        mixture.read_allele_depths(str(headless))


# ------------------------------------------------------------------------------------------------ the library's validation
def test_refusals_that_need_no_device():
    lib = _lib.load()
    out = np.zeros((2, 2, 2, 2, 2), dtype=np.int32)
    cols = np.zeros(2, dtype=np.int32)
    five = np.array([0, 1, 15, 255, 3], dtype=np.uint8)

    def call(ncols, n_rows, table=out, cols=cols, alt=five, ref=five):
        rc = lib.snpm_panel_mix_counts(None, _lib.ptr(cols), ncols, None, 0, n_rows, _lib.ptr(alt), _lib.ptr(ref), _lib.ptr(table))
        return rc, lib.snpm_last_error(None).decode()
    assert call(-1, 5) == (_lib.SNPM_ERR_BADARG, "negative size")
    assert call(2, -1) == (_lib.SNPM_ERR_BADARG, "negative size")
    rc, msg = call(11553, 5)
    assert rc == _lib.SNPM_ERR_BADARG and "too many accessions" in msg and "SNPM_MIX_MAX_ACCESSIONS" in msg
    rc, msg = call(2, 2 ** 31)
    assert rc == _lib.SNPM_ERR_BADARG and "2^31 rows" in msg
    assert call(2, 5, table=None) == (_lib.SNPM_ERR_BADARG, "table is NULL")
    assert call(2, 5, alt=None) == (_lib.SNPM_ERR_BADARG, "alt / ref is NULL")
    assert call(2, 5, ref=None) == (_lib.SNPM_ERR_BADARG, "alt / ref is NULL")
    # n_rows * the largest count < 2^31: 8421505 * 255 = 2^31 + 127 is refused, one row fewer (2^31 - 128) passes on to the panel check
    n = 8421505
    assert (n - 1) * 255 < 2 ** 31 <= n * 255
    deep, flat = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    deep[n - 2] = 255
    rc, msg = call(2, n, alt=deep, ref=flat)
    assert rc == _lib.SNPM_ERR_BADARG and "reaches 2^31" in msg and "int32" in msg
    rc, msg = call(2, n, alt=flat, ref=deep)
    assert rc == _lib.SNPM_ERR_BADARG and "reaches 2^31" in msg
    assert call(2, n - 1, alt=deep, ref=flat) == (_lib.SNPM_ERR_BADARG, "panel is NULL")
    deep[n - 2] = 254                       # 8421505 * 254 < 2^31
    assert call(2, n, alt=deep, ref=flat) == (_lib.SNPM_ERR_BADARG, "panel is NULL")
    assert call(2, 5) == (_lib.SNPM_ERR_BADARG, "panel is NULL")                  # sound arguments: only the panel is missing
    assert call(0, 5, table=None) == (_lib.SNPM_ERR_BADARG, "panel is NULL")
    assert call(2, 0, alt=None, ref=None) == (_lib.SNPM_ERR_BADARG, "panel is NULL")
    assert call(11552, 5, cols=None) == (_lib.SNPM_ERR_BADARG, "panel is NULL")  # the limit is inclusive
    header = open(os.path.join(ROOT, "include", "snpmatch_hip.h")).read()
    assert "#define SNPM_MIX_MAX_ACCESSIONS 11552" in header and engine.MIX_MAX_ACCESSIONS == 11552
    assert (11552 // 32) * (11552 // 32 + 1) // 2 < 2 ** 16
    assert "snpm_panel_mix_counts" in _lib.SYMBOLS


def test_group_and_streamed_panels_and_bad_counts_are_refused_with_the_reason():
    three = np.zeros(3, dtype=np.uint8)
    for cls, why in ((engine.GroupPanel, "spread over several GPUs"), (engine.StreamedPanel, "not a resident panel")):
        with pytest.raises(TypeError, match="mix_counts needs every accession column on one device") as err:
            engine.mix_counts(cls.__new__(cls), three, three)
        assert why in str(err.value)
    for cls, why in ((engine.GroupPanel, "spread over several GPUs by accession"), (engine.StreamedPanel, "streamed through the device")):
        with pytest.raises(TypeError, match="the mixture scan needs every accession column of the DB on one device") as err:
            snp_genotype.Genotype.mix_counts(_Holder(cls.__new__(cls)), three, three)
        assert why in str(err.value)
    stub = engine.Panel.__new__(engine.Panel)
    stub.ctx, stub.n_acc, stub.n_snp, stub.h = None, 4, 3, None
    with pytest.raises(AssertionError, match="one alt count per selected row: 2 counts, 3 rows"):
        engine.mix_counts(stub, three[:2], three)
    with pytest.raises(AssertionError, match="ref counts are integers 0 .. 255"):
        engine.mix_counts(stub, three, np.array([0, 256, 1]))
    with pytest.raises(AssertionError, match="alt counts are integers 0 .. 255"):
        engine.mix_counts(stub, np.array([0.5, 1, 1]), three)


class _Holder(object):
    """stands in for a Genotype whose DB went to the given kind of panel"""

    def __init__(self, panel):
        self._panel = panel

    def panel(self):
        return self._panel


# ------------------------------------------------------------------------------------------------ the command
@pytest.fixture
def twin_device(monkeypatch):
    """``engine.mix_counts`` by the twin on the DB the Genotype was loaded from; records (cols, rows, largest count) of every call"""
    return mixture_twin.install_twin(monkeypatch)


def run_planted(alpha, tmp_path, extra=()):
    case = mixture_twin.planted_case(alpha)
    db, vcf = mixture_twin.write_planted(case, tmp_path)
    out = str(tmp_path / "out")
    rc = cli.main(["mixture", "-i", vcf, "-d", db, "-o", out] + list(extra))
    return case, rc, out


def test_command_finds_the_planted_pool(twin_device, tmp_path):
    case, rc, out = run_planted(0.2, tmp_path)
    assert rc == 0 and len(twin_device) == 1 and twin_device[0][0] is None
    stats = json.load(open(out + ".mixture.json"))
    major, minor = "acc%02d" % mixture_twin.PLANTED_MAJOR, "acc%02d" % mixture_twin.PLANTED_MINOR
    best = stats["best_pair"]
    assert (best["major"], best["minor"]) == (major, minor) and stats["verdict"] == "mixture" and abs(best["alpha"] - 0.2) <= 0.05
    assert 2 * best["llr"] > 100 and stats["best_single"]["accession"] == major and stats["shortlist"][0] == best and len(stats["shortlist"]) == 10
    # rows: 6040 records, those without a read dropped by the reader, the 40 the DB does not have unmatched, none too deep for 15
    depth = case["alt"] + case["ref"]
    rows = stats["rows"]
    assert rows["records"] == 6040 and rows["dropped_zero_depth"] == int((depth == 0).sum()) and rows["with_reads"] == int((depth > 0).sum())
    assert rows["matched"] == rows["with_reads"] - 40 and rows["dropped_too_deep"] == 0 and rows["used"] == rows["matched"] and rows["dropped_not_selected"] == 0
    assert twin_device[0][2] == int(max(case["alt"].max(), case["ref"].max())) and stats["sample"] == "pool" and stats["candidates"] == 40
    z = np.load(out + ".mixture.npz")
    assert z["accessions"].tolist() == case["names"].tolist() and z["table"].dtype == np.int32 and z["table"].shape == (2, 2, 2, 40, 40)
    assert z["alpha"][7, 23] == best["alpha"] and z["ll"][7, 23] == best["ll"] and z["llr"][7, 23] == best["llr"] and z["reads"][7, 23] == best["reads"]
    assert int(z["table"][:, :, :, 7, 23].sum()) == best["reads"] and z["reads"].dtype == np.int64
    fit = mixture.fit_pairs(z["table"], 0.01, mixture.alpha_grid(0.01))
    assert all(np.array_equal(fit[k], z[k]) for k in ("alpha", "ll", "llr", "reads"))
    lines = [ln.split("\t") for ln in open(out + ".mixture.scores.txt").read().splitlines()]
    assert lines[0] == ["major", "minor", "alpha", "ll", "llr", "reads", "ll_per_read"] and len(lines) == 11
    assert lines[1][:3] == [major, minor, "%.4f" % best["alpha"]] and float(lines[1][3]) == best["ll"] and int(lines[1][5]) == best["reads"]
    per_read = [float(ln[6]) for ln in lines[1:]]
    assert per_read == sorted(per_read, reverse=True)


def test_command_calls_a_pure_sample_single_and_an_even_pool_mixture_or_f1(twin_device, tmp_path):
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    _, rc, out = run_planted(0.0, tmp_path / "a")
    stats = json.load(open(out + ".mixture.json"))
    assert rc == 0 and stats["verdict"] == "single" and stats["best_single"]["accession"] == "acc%02d" % mixture_twin.PLANTED_MAJOR
    assert stats["best_pair"]["major"] == "acc%02d" % mixture_twin.PLANTED_MAJOR and 2 * stats["best_pair"]["llr"] < 3.841 and "note" not in stats
    _, rc, out = run_planted(0.5, tmp_path / "b")
    stats = json.load(open(out + ".mixture.json"))
    assert rc == 0 and stats["verdict"] == "mixture_or_f1" and stats["best_pair"]["alpha"] >= 0.4 and "f1search" in stats["note"]
    assert {stats["best_pair"]["major"], stats["best_pair"]["minor"]} == {"acc07", "acc23"}


def test_command_options_and_routing(twin_device, tmp_path):
    case = mixture_twin.planted_case(0.2)
    db, vcf = mixture_twin.write_planted(case, tmp_path)
    out = str(tmp_path / "out")
    base = ["mixture", "-i", vcf, "-d", db, "-o", out]
    for bad in (["--err", "0"], ["--err", "0.5"], ["--grid", "0.03"], ["--grid", "0"], ["--max_depth", "0"], ["--max_depth", "256"],
                ["--min_reads", "0"], ["--top", "0"], ["--sample", "nobody"], ["--sample", "1"], ["--bed", "Chr1,1,100", "--sites", vcf]):
        assert cli.main(base + bad) == 2, bad
    assert not twin_device
    bed = tmp_path / "sample.bed"
    bed.write_text("Chr1\t10\t0/0\n")
    assert cli.main(["mixture", "-i", str(bed), "-d", db, "-o", out]) == 2 and not twin_device
    # --max_depth drops rows and counts them; the counts that travel stay below it
    depth = case["alt"] + case["ref"]
    assert cli.main(base + ["--max_depth", "4", "--sample", "pool"]) == 0
    stats = json.load(open(out + ".mixture.json"))
    in_db = np.isin(case["pos"], case["positions"]) & (depth > 0)              # (positions of the two chromosomes do not collide)
    assert stats["rows"]["dropped_too_deep"] == int((depth[in_db] > 4).sum()) > 0 and stats["rows"]["used"] == int((depth[in_db] <= 4).sum())
    assert twin_device[-1][2] <= 4 and stats["max_depth"] == 4 and stats["best_pair"]["major"] == "acc07"
    # -a: the candidates in the order of the list; a list that names one twice is refused
    acc = tmp_path / "cands.txt"
    acc.write_text("acc23\nacc02\nacc07\nacc11\n")
    assert cli.main(base + ["-a", str(acc), "--top", "3"]) == 0
    stats = json.load(open(out + ".mixture.json"))
    assert twin_device[-1][0].tolist() == [23, 2, 7, 11] and stats["candidates"] == 4 and len(stats["shortlist"]) == 3
    assert (stats["best_pair"]["major"], stats["best_pair"]["minor"]) == ("acc07", "acc23")
    assert np.load(out + ".mixture.npz")["accessions"].tolist() == ["acc23", "acc02", "acc07", "acc11"]
    acc.write_text("acc23\nacc23\n")
    n_calls = len(twin_device)
    assert cli.main(base + ["-a", str(acc)]) == 2 and len(twin_device) == n_calls
    # --bed: the rows of the region only (Chr1 positions 10 .. 30000: DB rows 0 .. 2999)
    assert cli.main(base + ["--bed", "Chr1,1,30001"]) == 0
    stats = json.load(open(out + ".mixture.json"))
    rows = np.asarray(twin_device[-1][1])
    assert len(rows) == stats["rows"]["used"] and rows.max() < 3000 and stats["rows"]["dropped_not_selected"] == stats["rows"]["matched"] - stats["rows"]["used"] > 0
    # --sites: the listed rows only
    sites = tmp_path / "sites.tsv"
    sites.write_text("chr\tpos\nChr1\t10\nChr1\t20\nChr2\t17\n")
    assert cli.main(base + ["--sites", str(sites), "--min_reads", "1"]) == 0
    rows = np.asarray(twin_device[-1][1])
    assert set(rows.tolist()) <= {0, 1, 3001} and json.load(open(out + ".mixture.json"))["rows"]["used"] == len(rows)


# ------------------------------------------------------------------------------------------------ the kernels, on the host
def _slices(counts, bits, step_words):
    """the words mix_fill_masks must write for one weight: [steps][bits][step_words] of uint64"""
    step_rows = step_words * 64
    steps = (len(counts) + step_rows - 1) // step_rows
    padded = np.zeros(steps * step_rows, dtype=np.uint64)
    padded[:len(counts)] = counts
    out = np.zeros((steps, bits, step_words), dtype=np.uint64)
    for j in range(bits):
        bit = ((padded >> np.uint64(j)) & np.uint64(1)).reshape(steps, step_words, 64)
        out[:, j, :] = (bit << np.arange(64, dtype=np.uint64)).sum(axis=2, dtype=np.uint64)
    return out


def test_kernel_source_on_the_host_under_asan_and_ubsan(tmp_path):
    """every block of k_win_planes / k_mix_count<2 / 4 / 8> run by 256 real threads with a barrier, exact-size heap buffers,
    arbitrary pad bytes, stale planes, against brute-force sums: 1 / 2 / 31 / 32 / 33 / 65 / 130 accessions x 1 / 63 / 64 / 65 rows in
    the three layouts with a largest count of 3 / 4 / 15 / 16 / 255, one row past an LDS step and past a chunk in each layout, a
    shape that crosses a tile, a step and a chunk at each BITS, two and three slabs, column lists with a repeat and unsorted row lists
    with a repeat (one over three slabs); the slab plan at the grid.y cap and below one step, the choice of BITS; and the words of
    mix_fill_masks against bit slices formed here"""
    cases = host_kernel_util.run_driver("mix_host_driver", tmp_path)
    assert len(cases) == 55 and sum(ln.startswith("case plan-") for ln in cases) == 8
    assert sum("slabs=2" in ln for ln in cases) == 2 and sum("slabs=3" in ln for ln in cases) == 2
    crossing = [ln for ln in cases if ln.startswith("case tile-step-chunk")]
    assert sorted(re.search(r"bits=(\d)", ln).group(1) for ln in crossing) == ["2", "4", "8"] and all("acc=33" in ln and "rows=9217" in ln for ln in crossing)
    for bits in ("2", "4", "8"):
        assert sum(" bits=%s " % bits in ln for ln in cases if not ln.startswith("case masks")) >= 8
    masks = [ln for ln in cases if ln.startswith("case masks")]
    assert len(masks) == 3
    for ln in masks:
        m = re.fullmatch(r"case masks bits=(\d+) rows=(\d+) step_words=(\d+) words=([0-9a-f]*) ok", ln)
        bits, n_rows, step_words, text = int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4)
        got = np.array([int(text[k:k + 16], 16) for k in range(0, len(text), 16)], dtype=np.uint64)
        k = np.arange(n_rows, dtype=np.uint64)
        alt, ref = (np.uint64(7) * k + np.uint64(3)) % np.uint64(1 << bits), (np.uint64(13) * k + np.uint64(5)) % np.uint64(1 << bits)
        want = np.stack([_slices(alt, bits, step_words), _slices(ref, bits, step_words)], axis=1)        # [step][weight][slice][word]
        assert got.shape == (want.size,) and np.array_equal(got, want.reshape(-1)), ln[:60]
        # ... which are the twin's sums: the popcount form of the table of one all-ref column against itself
        total = sum(int(np.sum([bin(int(w)).count("1") for w in want[:, 0, j].reshape(-1)])) << j for j in range(bits))
        assert total == int(mixture_twin.mix_counts(np.zeros((n_rows, 1), dtype=np.int8), alt, ref)[0, 0, 0, 0, 0])
