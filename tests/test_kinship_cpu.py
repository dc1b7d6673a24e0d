"""Panel kinship without a GPU: the numpy twin (tests/kinship_twin.py) and ``snp_genotype.calc_kinship_mat`` against the reference's
goldens (counts equal, kinship equal as fp64 bits, ``nan`` where the reference has ``nan``); every refusal of
``snpm_panel_kinship_counts`` that needs no device; the ``kinship`` subcommand with the twin in the place of the device call; and the
kernel source itself, compiled for the host and run by 256 real threads per block under AddressSanitizer + UBSan
(tests/kin_host_driver.cpp on tests/host_kernel/, a child process)."""
import glob
import os

import numpy as np
import pytest

import host_kernel_util
import kinship_twin
from snpmatch_amd import _lib, cli, engine
from snpmatch_amd.core import kinship, snp_genotype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["kinship_a%d_r%d" % (a, r) for a in (1, 2, 7) for r in (1, 999, 1000, 1001, 2500)]


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(b)
    return (a.dtype == np.float64 and a.shape == b.shape and np.array_equal(np.isnan(a), nan) and
            np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64)))


def test_every_golden_is_listed(golden_dir):
    assert sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(golden_dir, "kinship_*.npz"))) == sorted(CASES)


@pytest.mark.parametrize("name", CASES)
def test_twin_and_calc_kinship_mat_reproduce_the_reference(name, golden_dir):
    case = np.load(os.path.join(golden_dir, name + ".npz"))
    snps = case["snps"]
    assert set(np.unique(snps).tolist()) <= {-1, 0, 1, 2}
    ninfo, same, diff = kinship_twin.kinship_counts(snps)
    assert ninfo.dtype == np.int32 and np.array_equal(ninfo, case["num_snps"])
    assert np.array_equal(same.astype(np.int64) - diff, case["k_mat"])
    assert same_bits(kinship_twin.kinship(ninfo, same, diff), case["kinship"])
    assert same_bits(snp_genotype.kinship_from_counts(ninfo, same, diff), case["kinship"])
    # the method's result: the listed accessions (a shuffle with one repeat), all rows, summed over 1000-row chunks there
    listed = kinship_twin.kinship_counts(snps, cols=case["acc_ix"])
    assert same_bits(kinship_twin.kinship(*listed), case["method_kinship"])
    # the host function
    k_mat, num_snps = snp_genotype.calc_kinship_mat(snps, return_counts=True)
    assert type(k_mat) is np.ndarray and k_mat.dtype == np.float64 and np.array_equal(k_mat, case["k_mat"]) and np.array_equal(num_snps, case["num_snps"])
    assert not np.signbit(k_mat[k_mat == 0]).any()
    assert same_bits(snp_genotype.calc_kinship_mat(snps), case["kinship"])
    assert same_bits(snp_genotype.calc_kinship_mat(snps[:, case["acc_ix"]]), case["method_kinship"])


def test_the_planted_columns_are_in_the_goldens(golden_dir):
    case = np.load(os.path.join(golden_dir, "kinship_a7_r2500.npz"))
    kin, n = case["kinship"], case["num_snps"]
    assert np.isnan(kin[2]).all() and np.isnan(kin[:, 2]).all()                 # an accession without a call
    assert np.array_equal(case["snps"][:, 3], case["snps"][:, 4]) and kin[3, 4] == kin[3, 3] == kin[4, 4]
    assert n[5, 6] == 0 and np.isnan(kin[5, 6]) and n[5, 5] > 0 and n[6, 6] > 0     # no shared informative row
    assert (case["snps"] == 2).any() and not np.isnan(kin[0, 1])


def test_twin_on_a_hand_made_matrix():
    snps = np.array([[0, 0, -1, 3], [1, 0, 1, 3], [2, 1, 1, -1], [1, 1, 0, 0]], dtype=np.int8)
    ninfo, same, diff = kinship_twin.kinship_counts(snps)
    assert ninfo.tolist() == [[4, 4, 3, 3], [4, 4, 3, 3], [3, 3, 3, 2], [3, 3, 2, 3]]
    assert same.tolist() == [[3, 2, 1, 0], [2, 4, 1, 0], [1, 1, 3, 1], [0, 0, 1, 1]]
    assert diff.tolist() == [[0, 1, 1, 1], [1, 0, 2, 1], [1, 2, 0, 0], [1, 1, 0, 0]]
    sub = kinship_twin.kinship_counts(snps, cols=[2, 0, 2], rows=[3, 3, 1])       # repeats count as listed
    assert sub[0].tolist() == [[3, 3, 3], [3, 3, 3], [3, 3, 3]] and sub[1].tolist() == [[3, 1, 3], [1, 3, 1], [3, 1, 3]]
    assert sub[2].tolist() == [[0, 2, 0], [2, 0, 2], [0, 2, 0]]


# ------------------------------------------------------------------------------------------------ the library's validation
def test_refusals_that_need_no_device():
    lib = _lib.load()
    out = np.zeros((3, 2, 2), dtype=np.int32)
    cols = np.zeros(2, dtype=np.int32)

    def call(ncols, n_rows, outs=(0, 1, 2), cols=cols, row0=0):
        ptrs = [_lib.ptr(out[k]) if k is not None else None for k in outs]
        rc = lib.snpm_panel_kinship_counts(None, _lib.ptr(cols), ncols, None, row0, n_rows, *ptrs)
        return rc, lib.snpm_last_error(None).decode()
    assert call(-1, 5) == (_lib.SNPM_ERR_BADARG, "negative size")
    assert call(2, -1) == (_lib.SNPM_ERR_BADARG, "negative size")
    rc, msg = call(11553, 5)
    assert rc == _lib.SNPM_ERR_BADARG and "too many accessions" in msg and "SNPM_KIN_MAX_ACCESSIONS" in msg
    rc, msg = call(2, 2 ** 31)
    assert rc == _lib.SNPM_ERR_BADARG and "2^31 rows" in msg
    for outs in ((None, 1, 2), (0, None, 2), (0, 1, None)):
        assert call(2, 5, outs) == (_lib.SNPM_ERR_BADARG, "ninfo / same / diff is NULL")
    assert call(2, 5) == (_lib.SNPM_ERR_BADARG, "panel is NULL")                  # sound arguments: only the panel is missing
    assert call(0, 5, (None, None, None)) == (_lib.SNPM_ERR_BADARG, "panel is NULL")
    assert call(11552, 2 ** 31 - 1, cols=None) == (_lib.SNPM_ERR_BADARG, "panel is NULL")     # both limits are inclusive
    header = open(os.path.join(ROOT, "include", "snpmatch_hip.h")).read()
    assert "#define SNPM_KIN_MAX_ACCESSIONS 11552" in header and engine.KIN_MAX_ACCESSIONS == 11552
    assert 11552 ** 2 < 2 ** 27 and (11552 // 32) * (11552 // 32 + 1) // 2 < 2 ** 16
    assert "snpm_panel_kinship_counts" in _lib.SYMBOLS


def test_group_and_streamed_panels_are_refused_with_the_reason():
    for cls, why in ((engine.GroupPanel, "spread over several GPUs"), (engine.StreamedPanel, "not a resident panel")):
        with pytest.raises(TypeError, match="every accession column on one device") as err:
            engine.kinship_counts(cls.__new__(cls))
        assert why in str(err.value)
    for cls, why in ((engine.GroupPanel, "spread over several GPUs by accession"), (engine.StreamedPanel, "streamed through the device")):
        with pytest.raises(TypeError, match="every accession column of the DB on one device") as err:
            snp_genotype.Genotype.kinship_counts(_Holder(cls.__new__(cls)), None, None)
        assert why in str(err.value)


class _Holder(object):
    """stands in for a Genotype whose DB went to the given kind of panel"""

    def __init__(self, panel):
        self._panel = panel

    def panel(self):
        return self._panel


# ------------------------------------------------------------------------------------------------ Genotype and the command
@pytest.fixture
def toy(monkeypatch):
    """a DB of 12 accessions x 900 rows on two chromosomes with planted near-identical pairs; the device call is the twin"""
    rng = np.random.default_rng(77)
    snps = rng.choice(np.array([-1, 0, 1, 2], dtype=np.int8), size=(900, 12), p=[0.1, 0.5, 0.35, 0.05])
    snps[:, 4] = snps[:, 1]                                     # identical
    snps[:, 9] = snps[:, 6]
    flip = rng.choice(np.flatnonzero((snps[:, 6] == 0) | (snps[:, 6] == 1)), size=5, replace=False)
    snps[flip, 9] = 1 - snps[flip, 6]                           # five differences among ~760 homozygous rows: above 0.99
    snps[:, 11] = snps[:, 0]
    snps[60:, 11] = -1                                          # identical, but on 60 rows only (fewer homozygous ones): below min_sites
    names = ["acc%02d" % i for i in range(12)]
    positions = np.concatenate([np.arange(10, 10 + 10 * 500, 10), np.arange(5, 5 + 10 * 400, 10)])
    g = snp_genotype.Genotype.from_arrays(snps, names, positions, ["Chr1", "Chr2"], [[0, 500], [500, 900]])
    calls = []

    def twin(panel, cols, rows):
        calls.append((cols, rows))
        return kinship_twin.kinship_counts(snps, cols, None if rows is None else np.asarray(rows))
    stub = engine.Panel.__new__(engine.Panel)
    stub.h = None
    monkeypatch.setattr(snp_genotype.Genotype, "panel", lambda self, ctx=None, packed=None: stub)
    monkeypatch.setattr(engine, "kinship_counts", twin)
    return g, snps, names, calls


def test_genotype_methods_on_listed_accessions_and_rows(toy):
    g, snps, names, calls = toy
    kin = g.kinship_given_snps()
    assert type(kin) is np.ndarray and same_bits(kin, snp_genotype.calc_kinship_mat(snps)) and calls[-1] == (None, None)
    acc = np.array([6, 9, 2, 6])
    rows = np.array([700, 3, 3, 250, 899])
    assert same_bits(g.kinship_given_snps(acc, rows), snp_genotype.calc_kinship_mat(snps[rows][:, acc]))
    assert isinstance(calls[-1][1], np.ndarray)
    # a run of rows travels as a dense range; the region of a bed triple is such a run
    region = g.determine_snp_ix_given_bed("Chr2,100,2000")
    assert region.tolist() == list(range(510, 700)) and g.determine_snp_ix_given_bed(["chr1", 1, 10 ** 9]).tolist() == list(range(500))
    assert same_bits(g.kinship_given_snps(filter_snp_ix=region), snp_genotype.calc_kinship_mat(snps[510:700]))
    assert calls[-1][1] == range(510, 700)
    assert g.get_chr_ind("Chr2") == 1 and g.get_chr_ind("7") is None
    with pytest.raises(AssertionError, match="not in the database"):
        g.determine_snp_ix_given_bed("Chr7,1,2")


def test_command_line_writes_both_files(toy, tmp_path, monkeypatch):
    g, snps, names, calls = toy
    monkeypatch.setattr(snp_genotype, "Genotype", lambda hdf5_file, hdf5_acc_file: g)
    db = tmp_path / "db.npz"
    db.write_bytes(b"")
    out = str(tmp_path / "out")
    assert cli.main(["kinship", "-d", str(db), "-o", out]) == 0
    z = np.load(out + ".kinship.npz")
    assert z["accessions"].tolist() == names
    want = kinship_twin.kinship_counts(snps)
    assert all(np.array_equal(z[k], w) and z[k].dtype == np.int32 for k, w in zip(("ninfo", "same", "diff"), want))
    assert same_bits(z["kinship"], snp_genotype.calc_kinship_mat(snps))
    lines = open(out + ".duplicates.tsv").read().splitlines()
    assert lines[0].split("\t") == ["acc_1", "acc_2", "same", "diff", "ninfo", "identity", "kinship"]
    rows = [ln.split("\t") for ln in lines[1:]]
    assert [(r[0], r[1]) for r in rows] == [("acc01", "acc04"), ("acc06", "acc09")]          # exactly the planted pairs, by identity
    ninfo, same, diff = want
    assert rows[0][2:6] == [str(same[1, 4]), "0", str(ninfo[1, 4]), "1.0"]
    assert rows[1][3] == "5" and rows[1][5] == repr(int(same[6, 9]) / float(int(same[6, 9]) + 5)) and float(rows[1][5]) >= 0.99
    assert rows[1][6] == repr(float(z["kinship"][6, 9]))
    # thresholds are the user's: fewer sites let the short pair in, a lower identity nothing else at this size
    assert cli.main(["kinship", "-d", str(db), "-o", out, "--min_sites", "20"]) == 0
    pairs = [tuple(ln.split("\t")[:2]) for ln in open(out + ".duplicates.tsv").read().splitlines()[1:]]
    assert pairs == [("acc00", "acc11"), ("acc01", "acc04"), ("acc06", "acc09")]
    # an accession list (file order, a name may repeat) and a region
    acc_file = tmp_path / "accs.txt"
    acc_file.write_text("# curated\nacc09\nacc06 extra text\n\nacc02\n")
    assert cli.main(["kinship", "-d", str(db), "-a", str(acc_file), "--bed", "Chr1,1,3000", "-o", out]) == 0
    z = np.load(out + ".kinship.npz")
    assert z["accessions"].tolist() == ["acc09", "acc06", "acc02"]
    region = kinship_twin.kinship_counts(snps, cols=[9, 6, 2], rows=slice(0, 299))
    assert np.array_equal(z["ninfo"], region[0]) and np.array_equal(z["diff"], region[2])
    assert calls[-1][1] == range(0, 299)
    acc_file.write_text("acc09\nnobody\n")
    assert cli.main(["kinship", "-d", str(db), "-a", str(acc_file), "-o", out]) == 2


def test_duplicate_pairs_needs_sites_and_sorts_ties_by_name():
    names = ["b", "a", "c"]
    same = np.array([[9, 5, 5], [5, 9, 5], [5, 5, 9]])
    diff = np.zeros((3, 3), dtype=int)
    rows = kinship.duplicate_pairs(names, same, same, diff, min_identity=1.0, min_sites=5)
    assert [r[:2] for r in rows] == [("a", "c"), ("b", "a"), ("b", "c")]
    assert kinship.duplicate_pairs(names, same, same, diff, min_sites=6) == []
    assert kinship.duplicate_pairs(names, diff, diff, diff, min_identity=0.0, min_sites=0) == []      # 0 / 0 is no identity


# ------------------------------------------------------------------------------------------------ the kernels, on the host
def test_kernel_source_on_the_host_under_asan_and_ubsan(tmp_path):
    """every block of k_kin_planes / k_kin_count run by 256 real threads with a barrier, exact-size heap buffers, stale planes:
    1 / 2 / 31 / 32 / 33 / 65 / 130 accessions x 0 / 1 / 63 / 64 / 65 rows in the three layouts, a chunk - 1 / exact / + 1, two
    slabs (whole chunks and single LDS steps), column and row lists (one over three slabs), the split layout at 1135 accessions;
    and the slab plan alone at the grid.y cap and below one step"""
    cases = host_kernel_util.run_driver("kin_host_driver", tmp_path)
    assert len(cases) == 46 and sum(ln.startswith("case plan-") for ln in cases) == 2
    assert sum("slabs=2" in ln for ln in cases) == 2 and sum("slabs=3" in ln for ln in cases) == 1
