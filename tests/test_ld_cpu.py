"""Panel LD without a GPU: the numpy twin (tests/ld_twin.py) against the reference's goldens (``nan`` where the reference has ``nan``,
never above 1, within 1e-12) and against a brute-force count; ``snp_genotype.ld_from_counts`` equal to the twin as fp64 bits and
``snp_genotype.calculate_ld`` against the goldens; ``snpm_ld_prune`` through the library against the twin's greedy loop, and under
AddressSanitizer + UBSan as a stand-alone program (tests/ld_prune_asan_driver.cpp); every refusal of ``snpm_panel_ld_band`` that
needs no device; ``Genotype.calculate_ld`` and the ``ld`` subcommand with the twin in the place of the device call; and the kernel
source itself, compiled for the host and run by real threads under AddressSanitizer + UBSan (tests/ld_host_driver.cpp on
tests/host_kernel/, a child process)."""
import glob
import json
import os
import subprocess

import numpy as np
import pytest

import host_kernel_util
import ld_twin
from snpmatch_amd import _lib, cli, engine
from snpmatch_amd.core import ld, snp_genotype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["ld_a%d_r%d" % (a, r) for a in (2, 7, 130) for r in (1, 2, 200)]
BOUND = 1e-12                               # the project's bound for a dense fp64 form against exact integers; measured by the generator: 6.9e-15


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(b)
    return (a.dtype == np.float64 and a.shape == b.shape and np.array_equal(np.isnan(a), nan) and
            np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64)))


def golden(golden_dir, name):
    case = np.load(os.path.join(golden_dir, name + ".npz"))
    snps = case["snps"]
    n = len(snps)
    ref = np.full((n, n), np.nan)
    ref[np.triu_indices(n)] = case["r2_upper"]
    ref.T[np.triu_indices(n)] = case["r2_upper"]
    return snps, ref


def mixed_panel(rng, n_rows, n_acc):
    return rng.choice(np.array([-1, 0, 1, 2, 3], dtype=np.int8), size=(n_rows, n_acc), p=[0.12, 0.42, 0.32, 0.09, 0.05])


def test_every_golden_is_listed(golden_dir):
    assert sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(golden_dir, "ld_*.npz"))) == sorted(CASES)


@pytest.mark.parametrize("name", CASES)
def test_twin_and_host_functions_against_the_reference(name, golden_dir):
    snps, ref = golden(golden_dir, name)
    n = len(snps)
    assert snps.dtype == np.int8 and set(np.unique(snps).tolist()) <= {0, 1, 2}
    nan = np.isnan(ref)
    twin = ld_twin.dense(snps, np.arange(n), None, v_alt=1, v_het=2, min_n=1)       # the reference takes the codes as numbers
    assert np.array_equal(np.isnan(twin), nan) and (twin[~nan] <= 1.0).all()
    assert not (~nan).any() or np.abs(twin[~nan] - ref[~nan]).max() <= BOUND
    own = snp_genotype.calculate_ld(snps.astype(np.float64))
    assert own.dtype == np.float64 and np.array_equal(np.isnan(own), nan) and (not (~nan).any() or np.abs(own[~nan] - ref[~nan]).max() <= BOUND)
    if n > 1:                               # the band form holds the same cells
        counts, r2 = ld_twin.ld_band(snps, n - 1, v_alt=1, v_het=2, min_n=1)
        for d in range(1, n):
            assert same_bits(r2[:n - d, d - 1], twin[np.arange(n - d), np.arange(d, n)])
            assert np.isnan(r2[n - d:, d - 1]).all() and not counts[n - d:, d - 1].any()
        assert (counts[:, :, 0][counts[:, :, 0] != 0] == snps.shape[1]).all()      # complete panels: every column is common


def test_the_planted_rows_are_in_the_goldens(golden_dir):
    snps, ref = golden(golden_dir, "ld_a130_r200")
    assert (snps[0] == 0).all() and (snps[1] == 1).all() and np.isnan(ref[0]).all() and np.isnan(ref[:, 1]).all()
    assert (snps[2] == 1).sum() == 1 and np.array_equal(snps[3], snps[2]) and np.array_equal(snps[4], 1 - snps[2])
    twin = ld_twin.dense(snps, [2, 3, 4], None, 1, 2, 1)
    assert (twin == 1.0).all() and np.abs(ref[2:5, 2:5] - 1.0).max() <= BOUND       # duplicate and complement: r2 = 1, exactly in integers


def test_twin_counts_against_a_brute_force_loop_and_ld_from_counts_bit_for_bit():
    rng = np.random.default_rng(41)
    for n_rows, n_acc, band, cols, rows in ((9, 5, 3, None, None), (12, 37, 12, [30, 2, 9, 17, 36, 0], None), (10, 33, 4, None, [7, 7, 0, 9, 3, 3, 8]),
                                            (1, 4, 2, None, None), (6, 1, 7, None, None)):
        snps = mixed_panel(rng, n_rows, n_acc)
        counts = ld_twin.band_counts(snps, band, cols, rows)
        assert counts.dtype == np.int32 and np.array_equal(counts, ld_twin.brute_counts(snps, band, cols, rows))
        for v_alt, v_het, min_n in ((2, 1, 2), (1, 2, 1), (3, 0, 4), (0, 3, 1), (2, 2, 2)):
            want = ld_twin.r2_from_counts(counts, v_alt, v_het, min_n)
            assert same_bits(snp_genotype.ld_from_counts(counts, v_alt, v_het, min_n), want)
            assert (want[~np.isnan(want)] <= 1.0).all()
    with pytest.raises(AssertionError, match="repeated column"):
        ld_twin.band_counts(snps, 2, [0, 0])
    # hand-made: rows 0 and 1 equal where both are known, row 2 constant among the common columns of (0, 2)
    snps = np.array([[1, 0, 2, -1, 0], [1, 0, 2, 1, 3], [0, 0, 0, 1, 1]], dtype=np.int8)
    counts, r2 = ld_twin.ld_band(snps, 2)
    assert counts[0, 0].tolist() == [3, 1, 1, 1, 1, 1, 0, 0, 1] and r2[0, 0] == 1.0
    assert counts[0, 1].tolist() == [4, 1, 1, 1, 0, 0, 0, 0, 0] and counts[1, 0].tolist() == [4, 2, 1, 1, 0, 1, 0, 0, 0]
    assert np.isnan(r2[1, 1]) and np.isnan(r2[2]).all() and not counts[2].any()
    assert np.isnan(ld_twin.r2_from_counts(counts, min_n=5)).all()
    for bad in ({"v_alt": 4}, {"v_het": -1}, {"min_n": 0}):
        with pytest.raises(ValueError):
            snp_genotype.ld_from_counts(counts, **bad)


# ------------------------------------------------------------------------------------------------ the prune
def test_prune_through_the_library_against_the_greedy_loop():
    rng = np.random.default_rng(42)
    for n, band in ((0, 3), (1, 1), (1, 5), (2, 1), (40, 1), (75, 6), (300, 64), (30, 100)):
        r2 = rng.integers(0, 11, size=(n, band)) / 10.0
        r2[rng.random((n, band)) < 0.2] = np.nan
        for eligible in (None, rng.random(n) < 0.7):
            for threshold in (0.2, 0.5, 1.0, -1.0):        # 0.2 and 0.5 equal cells: ``>`` is strict
                got = engine.ld_prune(r2, eligible, threshold)
                assert got.dtype == bool and np.array_equal(got, ld_twin.prune(r2, eligible, threshold).astype(bool)), (n, band, threshold)
    r2 = np.array([[0.5, np.nan], [0.9, 0.1], [np.nan, np.nan]])
    assert engine.ld_prune(r2, None, 0.5).tolist() == [True, True, False]       # 0.5 does not exceed 0.5; 0.9 does
    assert engine.ld_prune(r2, None, 0.4).tolist() == [True, False, True]       # row 1 pruned: it prunes nothing itself; nan never prunes
    assert engine.ld_prune(r2, [False, True, True], 0.4).tolist() == [False, True, False]
    assert engine.ld_prune(np.full((5, 3), np.nan)).all()
    with pytest.raises(ValueError, match="n_rows, band"):
        engine.ld_prune(np.zeros(4))
    with pytest.raises(ValueError, match="one entry per row"):
        engine.ld_prune(np.zeros((4, 2)), [True])
    lib = _lib.load()
    k = np.zeros(1, dtype=np.uint8)
    assert lib.snpm_ld_prune(-1, 1, None, None, 0.2, _lib.ptr(k)) == _lib.SNPM_ERR_BADARG
    assert lib.snpm_ld_prune(1, 0, _lib.ptr(np.zeros(1)), None, 0.2, _lib.ptr(k)) == _lib.SNPM_ERR_BADARG
    assert lib.snpm_ld_prune(1, 1, None, None, 0.2, _lib.ptr(k)) == _lib.SNPM_ERR_BADARG
    assert lib.snpm_ld_prune(0, 1, None, None, 0.2, None) == _lib.SNPM_OK


def test_prune_under_asan_and_ubsan_as_a_stand_alone_program(tmp_path):
    exe = str(tmp_path / "ld_prune_asan_driver")
    csrc = os.path.join(ROOT, "snpmatch_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(ROOT, "tests", "ld_prune_asan_driver.cpp"),
                           os.path.join(csrc, "snpm_host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "done fails=0" and len(lines) == 6 * 5 * 4 + 2 and all(ln.endswith(" ok") for ln in lines[:-1])
    assert any("rows=257 band=300" in ln for ln in lines) and any("rows=0 " in ln for ln in lines)


# ------------------------------------------------------------------------------------------------ the library's validation
def test_refusals_that_need_no_device():
    lib = _lib.load()
    counts, r2, cols = np.zeros((5, 3, 9), dtype=np.int32), np.zeros((5, 3)), np.zeros(4, dtype=np.int32)

    def call(ncols=4, n_rows=5, band=3, v_alt=2, v_het=1, min_n=2, counts=counts, r2=r2):
        rc = lib.snpm_panel_ld_band(None, _lib.ptr(cols), ncols, None, 0, n_rows, band, v_alt, v_het, min_n, _lib.ptr(counts), _lib.ptr(r2))
        return rc, lib.snpm_last_error(None).decode()
    assert call(ncols=-1) == (_lib.SNPM_ERR_BADARG, "negative size")
    assert call(n_rows=-1) == (_lib.SNPM_ERR_BADARG, "negative size")
    for band in (0, -3, engine.LD_MAX_BAND + 1):
        assert call(band=band) == (_lib.SNPM_ERR_BADARG, "band must be 1 .. SNPM_LD_MAX_BAND")
    for bad in ({"v_alt": 4}, {"v_alt": -1}, {"v_het": 4}, {"v_het": -1}):
        assert call(**bad) == (_lib.SNPM_ERR_BADARG, "v_alt and v_het must be 0 .. 3")
    assert call(min_n=0) == (_lib.SNPM_ERR_BADARG, "min_n must be at least 1")
    assert call(counts=None, r2=None) == (_lib.SNPM_ERR_BADARG, "counts and r2 are both NULL")
    # sound arguments: only the panel is missing (one output is enough; none is needed where there is no row; the limits are inclusive)
    assert call() == (_lib.SNPM_ERR_BADARG, "panel is NULL")
    assert call(counts=None) == call(r2=None) == (_lib.SNPM_ERR_BADARG, "panel is NULL")
    assert call(n_rows=0, counts=None, r2=None) == (_lib.SNPM_ERR_BADARG, "panel is NULL")
    assert call(band=engine.LD_MAX_BAND, v_alt=3, v_het=0, min_n=1, counts=None) == (_lib.SNPM_ERR_BADARG, "panel is NULL")
    assert not counts.any() and not r2.any()
    header = open(os.path.join(ROOT, "include", "snpmatch_hip.h")).read()
    assert "#define SNPM_LD_MAX_BAND 4096" in header and engine.LD_MAX_BAND == 4096 >= 1024
    kernel = open(os.path.join(ROOT, "snpmatch_amd", "csrc", "snpm_k_ld.hpp")).read()
    assert "#define SNPM_LD_MAX_BAND 4096" in kernel
    assert (64 * 3 * 24 + 127 * (3 * 24 + 1)) * 4 <= 65536           # rows k + rows j of a tile's column chunk: the static LDS of a block
    assert "snpm_panel_ld_band" in _lib.SYMBOLS and "snpm_ld_prune" in _lib.SYMBOLS


def test_group_and_streamed_panels_are_refused_with_the_reason_and_the_python_checks():
    for cls, why in ((engine.GroupPanel, "spread over several GPUs"), (engine.StreamedPanel, "not a resident panel")):
        with pytest.raises(TypeError, match="every accession column on one device") as err:
            engine.ld_band(cls.__new__(cls), 5)
        assert why in str(err.value)
    for cls, why in ((engine.GroupPanel, "spread over several GPUs by accession"), (engine.StreamedPanel, "streamed through the device")):
        with pytest.raises(TypeError, match="every accession column of the DB on one device") as err:
            snp_genotype.Genotype.ld_band(_Holder(cls.__new__(cls)), 5)
        assert why in str(err.value)
    panel = engine.Panel.__new__(engine.Panel)
    panel.h, panel.n_snp, panel.n_acc = None, 60, 40
    with pytest.raises(AssertionError, match="band must be 1 .. 4096"):
        engine.ld_band(panel, 0)
    with pytest.raises(TypeError, match="band must be an integer"):
        engine.ld_band(panel, 2.5)
    with pytest.raises(TypeError, match="must be integers"):
        engine.ld_band(panel, 2, np.array([0.5]))
    with pytest.raises(ValueError, match="neither counts nor r2"):
        engine.ld_band(panel, 2, counts=False, r2=False)
    with pytest.raises(ValueError, match="step 1"):
        engine.ld_band(panel, 2, None, range(0, 10, 2))


class _Holder(object):
    """stands in for a Genotype whose DB went to the given kind of panel"""

    def __init__(self, panel):
        self._panel = panel

    def panel(self):
        return self._panel


# ------------------------------------------------------------------------------------------------ Genotype and the command
@pytest.fixture
def toy(monkeypatch):
    """a DB of 12 accessions x 900 rows on two chromosomes, in blocks of correlated rows; the device calls are the twins"""
    rng = np.random.default_rng(79)
    base = rng.choice(np.array([0, 1], dtype=np.int8), size=(90, 12))
    snps = np.repeat(base, 10, axis=0)                               # ten copies of every founder row ...
    noise = rng.random(snps.shape)
    snps[noise < 0.08] = -1                                          # ... with missing calls, hets and flips
    snps[(noise > 0.08) & (noise < 0.12)] = 2
    flip = (noise > 0.9) & (snps >= 0) & (snps <= 1)
    snps[flip] = 1 - snps[flip]
    snps[10] = 0                            # monomorphic
    snps[11] = -1                           # no informative accession
    names = ["acc%02d" % i for i in range(12)]
    positions = np.concatenate([np.arange(10, 10 + 10 * 500, 10), np.arange(5, 5 + 10 * 400, 10)])
    g = snp_genotype.Genotype.from_arrays(snps, names, positions, ["Chr1", "Chr2"], [[0, 500], [500, 900]])
    calls = []

    def twin(panel, band, cols=None, rows=None, v_alt=2, v_het=1, min_n=2, counts=True, r2=True):
        calls.append((band, cols, rows))
        c, r = ld_twin.ld_band(snps, band, cols, rows, v_alt, v_het, min_n)
        return (c if counts else None), (r if r2 else None)
    stub = engine.Panel.__new__(engine.Panel)
    stub.h = None
    monkeypatch.setattr(snp_genotype.Genotype, "panel", lambda self, ctx=None, packed=None: stub)
    monkeypatch.setattr(engine, "ld_band", twin)
    import sitestats_twin
    monkeypatch.setattr(engine, "site_counts", lambda panel, groups=None, rows=None: sitestats_twin.site_counts(snps, groups, rows))
    return g, snps, names, calls


def test_genotype_methods_with_the_twin_as_device(toy):
    g, snps, names, calls = toy
    counts, r2 = g.ld_band(4, None, np.arange(20, 60))
    assert calls[-1] == (4, None, range(20, 60)) and same_bits(r2, ld_twin.ld_band(snps, 4, None, range(20, 60))[1]) and counts.shape == (40, 4, 9)
    rows, accs = np.array([700, 3, 3, 250, 899, 12, 10, 11]), np.array([6, 9, 2, 0, 11])
    got = g.calculate_ld(rows, accs)
    assert calls[-1][0] == 7 and isinstance(calls[-1][2], np.ndarray)
    assert got.shape == (8, 8) and same_bits(got, ld_twin.dense(snps, rows, accs)) and np.array_equal(np.isnan(got), np.isnan(got.T))
    assert np.isnan(got[6]).all() and np.isnan(got[7, 7])           # monomorphic; no call
    full = g.calculate_ld(rows, None, 1, 2, 4)
    assert same_bits(full, ld_twin.dense(snps, rows, None, 1, 2, 4)) and full[1, 2] == 1.0 and full[0, 0] == 1.0     # a repeated row; the diagonal
    n_calls = len(calls)
    one = g.calculate_ld([5])
    assert one.shape == (1, 1) and one[0, 0] == 1.0 and len(calls) == n_calls    # one row: no band call
    assert g.calculate_ld([]).shape == (0, 0)
    with pytest.raises(ValueError, match="at most 4097 rows"):
        g.calculate_ld(np.zeros(4098, dtype=np.int64))


def test_command_line_writes_its_files(toy, tmp_path, monkeypatch):
    g, snps, names, calls = toy
    monkeypatch.setattr(snp_genotype, "Genotype", lambda hdf5_file, hdf5_acc_file: g)
    monkeypatch.setattr(engine, "ld_prune", lambda r2, eligible=None, threshold=0.2: ld_twin.prune(r2, eligible, threshold).astype(bool))
    db = tmp_path / "db.npz"
    db.write_bytes(b"")
    out = str(tmp_path / "out")
    pos = np.asarray(g.g.positions)
    # the whole DB, chromosome by chromosome: two calls, no pair across the chromosome edge
    assert cli.main(["ld", "-d", str(db), "--band", "12", "--r2", "0.5", "--keep_r2", "-o", out]) == 0
    assert [(c[0], c[2]) for c in calls[-2:]] == [(12, range(0, 500)), (12, range(500, 900))]
    parts = [ld_twin.ld_band(snps, 12, None, range(0, 500))[1], ld_twin.ld_band(snps, 12, None, range(500, 900))[1]]
    keep = np.concatenate([ld_twin.prune(p, None, 0.5) for p in parts]).astype(bool)
    z = np.load(out + ".ld.npz")
    assert same_bits(z["r2"], np.concatenate(parts)) and np.array_equal(z["keep"], keep) and z["chr"].tolist() == ["Chr1"] * 500 + ["Chr2"] * 400
    assert np.isnan(z["r2"][499]).all() and np.array_equal(z["pos"], pos)
    lines = open(out + ".pruned.tsv").read().splitlines()
    assert lines[0] == "chr\tpos" and [ln.split("\t") for ln in lines[1:]] == [[c, str(p)] for c, p in zip(z["chr"][keep], pos[keep])]
    assert 90 <= keep.sum() < 450                                    # blocks of ten near-copies: most of a block goes
    stats = json.load(open(out + ".ld.json"))
    both = np.concatenate(parts)
    assert stats["rows"] == 900 and stats["rows_kept"] == int(keep.sum()) and stats["pairs_defined"] == int((~np.isnan(both)).sum())
    assert len(stats["mean_r2_by_offset"]) == 12 and stats["mean_r2_by_offset"][0] == pytest.approx(float(np.nanmean(np.concatenate([p[:, 0] for p in parts]))), rel=1e-12)       # (900 terms, another order of summation)
    assert stats["mean_r2_by_offset"][0] > stats["mean_r2_by_offset"][11]       # the decay curve decays
    # a region, an accession list, a window in bp: pairs further apart are undefined before anything else is done with them
    acc_file = tmp_path / "accs.txt"
    acc_file.write_text("acc09\nacc06\nacc01\nacc02\nacc11\nacc04\n")
    assert cli.main(["ld", "-d", str(db), "-a", str(acc_file), "--bed", "Chr2,100,2000", "--band", "7", "--window_bp", "30", "--min_n", "3", "--keep_r2", "-o", out]) == 0
    assert calls[-1][0] == 7 and calls[-1][1].tolist() == [9, 6, 1, 2, 11, 4] and calls[-1][2] == range(510, 700)
    want = ld_twin.ld_band(snps, 7, [9, 6, 1, 2, 11, 4], range(510, 700), min_n=3)[1]
    assert not np.isnan(want[:100, 3:]).all()
    want[:, 3:] = np.nan                                            # rows lie 10 bp apart: offsets 4 .. 7 are beyond 30 bp
    z = np.load(out + ".ld.npz")
    assert same_bits(z["r2"], want) and np.array_equal(z["keep"], ld_twin.prune(want, None, 0.2).astype(bool))
    assert json.load(open(out + ".ld.json"))["mean_r2_by_offset"][3:] == [None] * 4 and not os.path.exists(out + ".nothing")
    # a site list in the format of sitestats, over both chromosomes, not sorted: the rows are taken in DB order per chromosome
    picked = np.array([640, 3, 520, 7, 8, 15, 16, 17, 899, 500, 499])
    sites = tmp_path / "x.sites.tsv"
    sites.write_text("chr\tpos\tmaf_all\tmissing_all\n" + "".join("%s\t%d\t0.25\t0.0\n" % ("Chr1" if r < 500 else "Chr2", pos[r]) for r in picked))
    os.remove(out + ".ld.npz")
    assert cli.main(["ld", "-d", str(db), "--sites", str(sites), "--band", "3", "--r2", "0.3", "-o", out]) == 0
    assert [c[2].tolist() for c in calls[-2:]] == [[3, 7, 8, 15, 16, 17, 499], [500, 520, 640, 899]] and not os.path.exists(out + ".ld.npz")
    keep = np.concatenate([ld_twin.prune(ld_twin.ld_band(snps, 3, None, np.array(r))[1], None, 0.3) for r in ([3, 7, 8, 15, 16, 17, 499], [500, 520, 640, 899])]).astype(bool)
    lines = open(out + ".pruned.tsv").read().splitlines()[1:]
    assert [int(ln.split("\t")[1]) for ln in lines] == pos[np.sort(picked)][keep].tolist() and json.load(open(out + ".ld.json"))["rows"] == 11


def test_command_line_refusals(toy, tmp_path, monkeypatch, caplog):
    g, snps, names, calls = toy
    monkeypatch.setattr(snp_genotype, "Genotype", lambda hdf5_file, hdf5_acc_file: g)
    db = tmp_path / "db.npz"
    db.write_bytes(b"")
    out = str(tmp_path / "out")
    sites = tmp_path / "x.sites.tsv"
    sites.write_text("chr\tpos\nChr1\t11\n")
    assert cli.main(["ld", "-d", str(db), "--sites", str(sites), "-o", out]) == 2 and "sites not in the database: Chr1:11" in caplog.text
    assert cli.main(["ld", "-d", str(db), "--sites", str(sites), "--bed", "Chr1,1,100", "-o", out]) == 2 and "not both" in caplog.text
    sites.write_text("chrom\tposition\nChr1\t10\n")
    assert cli.main(["ld", "-d", str(db), "--sites", str(sites), "-o", out]) == 2 and "must name the columns chr and pos" in caplog.text
    sites.write_text("chr\tpos\nChr9\t10\n")
    assert cli.main(["ld", "-d", str(db), "--sites", str(sites), "-o", out]) == 2 and "chromosome Chr9 of the site list" in caplog.text
    assert cli.main(["ld", "-d", str(db), "--band", "0", "-o", out]) == 2 and "--band must be 1 .. 4096" in caplog.text
    acc_file = tmp_path / "accs.txt"
    acc_file.write_text("acc01\nacc01\n")
    assert cli.main(["ld", "-d", str(db), "-a", str(acc_file), "-o", out]) == 2 and "names an accession twice" in caplog.text
    assert not os.path.exists(out + ".pruned.tsv")
    r2 = np.array([[0.5, 0.6, 0.7], [0.1, 0.2, 0.3], [0.4, 0.4, 0.4], [0.9, 0.9, 0.9]])
    masked = ld.mask_window(r2.copy(), np.array([10, 20, 45, 50]), 25)
    assert np.isnan(masked[0, 1:]).all() and masked[0, 0] == 0.5 and masked[1, 0] == 0.1 and np.isnan(masked[1, 1]) and masked[2, 0] == 0.4
    assert same_bits(masked[2:, 1:], r2[2:, 1:]) and same_bits(masked[3], r2[3])       # cells past the end are left as they are


# ------------------------------------------------------------------------------------------------ the kernels, on the host
def test_kernel_source_on_the_host_under_asan_and_ubsan(tmp_path):
    """every block of k_ld_planes (256 threads) and k_ld_band (1024 threads) run by real threads with a barrier, exact-size heap
    buffers, arbitrary pad bytes, stale workspaces: 1 / 2 / 31 / 32 / 33 / 63 / 64 / 65 / 130 / 1135 accessions x 0 / 1 / 2 / band /
    band + 1 / 63 / 64 / 65 rows with bands 1 / 2 / 63 / 64 / 65 in the three layouts, every band in every layout at 1135 accessions,
    rows of a pitch that takes the byte loads, 800 and 1601 accessions (more than one column chunk of 768) and 16 384, a column
    subset, a row list that is unsorted with a repeat, other genotype values, counts only / r2 only / both, two and three slabs with
    the halo across each edge and a last slab shorter than the band.  The slab plan of every case is the library's, and
    engine.ld_slab_rows agrees with it."""
    cases = host_kernel_util.run_driver("ld_host_driver", tmp_path)
    assert len(cases) == 80 + 15 + 6 + 4 + 4 + 1
    field = lambda ln, key: int(ln.split(key + "=")[1].split()[0])      # noqa: E731
    runs = [ln for ln in cases if not ln.startswith("case plan")]
    assert {field(ln, "acc") for ln in runs} >= {1, 2, 31, 32, 33, 63, 64, 65, 130, 1135, 800, 1601, 16384}
    assert {field(ln, "band") for ln in runs} >= {1, 2, 63, 64, 65} and {field(ln, "rows") for ln in runs} >= {0, 1, 2, 3, 63, 64, 65, 66}
    assert {(field(ln, "layout"), field(ln, "band")) for ln in runs if ln.startswith("case 1135 ")} == {(l, b) for l in (0, 1, 2) for b in (1, 2, 63, 64, 65)}
    assert sum(field(ln, "slabs") == 2 for ln in runs) == 2 and sum(field(ln, "slabs") == 3 for ln in runs) == 2
    assert sum(field(ln, "wide") == 0 for ln in runs) >= 5 and sum(field(ln, "list") for ln in runs) >= 5 and sum(field(ln, "subset") for ln in runs) >= 20
    assert {field(ln, "outs") for ln in runs} == {1, 2, 3}
    for ln in runs:                         # the Python form of the plan: 256 MiB, or a budget of one byte
        if field(ln, "rows"):
            ws = 1 if field(ln, "slabs") > 1 else 256 << 20
            assert engine.ld_slab_rows(ws, field(ln, "acc"), field(ln, "band"), field(ln, "rows")) == field(ln, "slab_rows"), ln
    plan = [int(v) for v in [ln for ln in cases if ln.startswith("case plan")][0].split()[2:6]]
    assert plan == [engine.ld_slab_rows(1 << 20, 16384, 65, 200), engine.ld_slab_rows(256 << 20, 1135, 50, 11000000),
                    engine.ld_slab_rows(1 << 20, 1135, 4096, 200), engine.ld_slab_rows(1, 1, 1, 10)] == [64, 101952, 64, 10]
