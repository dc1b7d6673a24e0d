"""Site statistics without a GPU: the numpy twin (tests/sitestats_twin.py), ``snp_genotype.calculate_af_snp_mat`` / ``_polarize_snps``
/ ``af_from_counts`` and the ``Genotype`` methods against the reference's goldens (counts equal, frequencies equal as fp64 bits,
``nan`` where the reference has ``nan``); every refusal of ``snpm_panel_site_counts`` that needs no device; the layering of repeated
columns in ``engine.site_counts`` and the ``sitestats`` subcommand with the twin in the place of the device call; and the kernel
source itself, compiled for the host and run by 512 real threads per block under AddressSanitizer + UBSan
(tests/site_host_driver.cpp on tests/host_kernel/, a child process)."""
import glob
import json
import os

import numpy as np
import pytest

import host_kernel_util
import sitestats_twin
from snpmatch_amd import _lib, cli, engine
from snpmatch_amd.core import sitestats, snp_genotype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["sitestats_a%d_r%d" % (a, r) for a in (1, 2, 7) for r in (1, 999, 1000, 1001, 2500)]
CALC_VARIANTS = [(pg, maf, mi) for pg in (0, 1, 2) for maf in (True, False) for mi in (0, 2)]      # the rows of ``calc_af``
# method calls of the generator: name -> (accession filter, row filter, no_accs_missing_info, polarize_geno, return_maf)
CALLS = {"all": (None, False, 0, 1, True), "listed": ("listed", False, 1, 1, False), "pops": ("pops", False, 0, 1, True),
         "listed_rows": ("listed", True, 0, 0, True), "pops_rows": ("pops", True, 2, 1, False), "all_rows": (None, True, 0, 2, False)}


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(b)
    return (a.dtype == np.float64 and a.shape == b.shape and np.array_equal(np.isnan(a), nan) and
            np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64)))


def method_calls(case):
    """(name, accession filter, row filter, min, polarize_geno, return_maf, {population or None: reference [2, n]}) per call kept"""
    pops = {"north": case["pop_north"], "south": case["pop_south"]}
    for name, (acc, rows, mi, pg, maf) in CALLS.items():
        acc_ix = None if acc is None else (case["acc_ix"] if acc == "listed" else pops)
        want = {pop: case["m_%s_%s" % (name, pop)] for pop in pops} if acc == "pops" and "m_%s_north" % name in case else None
        if acc != "pops" and "m_" + name in case:
            want = {None: case["m_" + name]}
        if want is not None:
            yield name, acc_ix, case["row_ix"] if rows else None, mi, pg, maf, want


def test_every_golden_is_listed(golden_dir):
    assert sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(golden_dir, "sitestats_*.npz"))) == sorted(CASES)


@pytest.mark.parametrize("name", CASES)
def test_twin_and_host_functions_reproduce_the_reference(name, golden_dir):
    case = np.load(os.path.join(golden_dir, name + ".npz"))
    snps = case["snps"]
    assert snps.dtype == np.int8 and set(np.unique(snps).tolist()) <= {-1, 0, 1, 2, 3}
    head = snps[:case["calc_af"].shape[1]]
    counts = sitestats_twin.site_counts(head)
    assert counts.dtype == np.int32 and counts.shape == (1, len(head), 4)
    for k, (pg, maf, mi) in enumerate(CALC_VARIANTS):
        got, num = snp_genotype.calculate_af_snp_mat(head, min_informative=mi, polarize_geno=pg, return_maf=maf)
        assert num.dtype == np.int64 and np.array_equal(num, case["calc_num_alleles"]) and same_bits(got, case["calc_af"][k])
        assert same_bits(snp_genotype.af_from_counts(counts[0], mi, pg, maf), case["calc_af"][k])
        assert same_bits(sitestats_twin.frequency(counts[0], mi, pg, maf), case["calc_af"][k])
    got, num = snp_genotype.calculate_af_snp_mat(head)              # the defaults: alt allele, folded, no minimum
    assert same_bits(got, case["calc_af"][CALC_VARIANTS.index((1, True, 0))])
    for pg in (0, 1):
        pol = snp_genotype._polarize_snps(head, polarize_geno=pg)
        assert pol.dtype == np.int8 and np.array_equal(pol, case["polarized"][pg]) and pol is not head
        flipped = (case["polarized"][pg] != head).any(axis=1)
        assert not (flipped & ~(counts[0, :, pg] > head.shape[1] / 2.0)).any()
    seen = 0
    for call, acc_ix, rows, mi, pg, maf, want in method_calls(case):
        groups = None if acc_ix is None else (list(acc_ix.values()) if isinstance(acc_ix, dict) else [acc_ix])
        twin = sitestats_twin.site_counts(snps, groups, rows)
        for k, ref in enumerate(want.values()):
            assert np.array_equal(twin[k, :, 3], ref[1]), call
            assert same_bits(snp_genotype.af_from_counts(twin[k], mi, pg, maf), ref[0]), call
            seen += 1
    assert seen == (4 if name.endswith("r2500") else 8)


def test_the_planted_rows_are_in_the_goldens(golden_dir):
    case = np.load(os.path.join(golden_dir, "sitestats_a7_r2500.npz"))
    snps, listed = case["snps"], case["acc_ix"]
    assert len(listed) == 8 and len(np.unique(listed)) == 7                       # one repeat
    assert (snps[0] == -1).all() and np.isnan(case["m_all"][0, 0]) and case["m_all"][1, 0] == 0
    assert (snps[1] == 3).all() and case["m_all"][0, 1] == 0.0 and case["m_all"][1, 1] == 7      # "other": informative, no allele
    assert (snps[2] == 1).all() and (case["polarized"][1, 2] == 0).all()          # all alt: flipped
    assert (snps[3, listed] == 1).sum() == 4 and np.array_equal(case["polarized"][1, 3], snps[3])     # exactly half: not flipped
    assert len(np.unique(case["row_ix"])) < len(case["row_ix"]) and (np.diff(case["row_ix"]) < 0).any()
    assert len(np.intersect1d(case["pop_north"], case["pop_south"])) and len(np.unique(case["pop_south"])) < len(case["pop_south"])


def test_af_from_counts_on_hand_made_counts():
    counts = np.array([[3, 1, 0, 4], [0, 0, 0, 0], [0, 2, 2, 5], [1, 0, 0, 1]], dtype=np.int32)
    af = snp_genotype.af_from_counts(counts, 0, 1, False)
    assert af[0] == 0.25 and np.isnan(af[1]) and af[2] == 0.6 and af[3] == 0.0
    assert snp_genotype.af_from_counts(counts, 0, 1, True)[2] == 1 - 0.6
    assert np.isnan(snp_genotype.af_from_counts(counts, 1, 1, True)[3])          # ninfo <= min_informative
    assert snp_genotype.af_from_counts(counts, 0, 0, False).tolist()[0] == 0.75
    assert snp_genotype.af_from_counts(counts, 0, 2, False)[2] == 0.6            # a het three times over 2 * 5
    assert snp_genotype.af_from_counts(counts.reshape(2, 2, 4)).shape == (2, 2)
    for bad in (3, -1, 1.5):
        with pytest.raises(ValueError, match="polarize_geno must be 0, 1 or 2"):
            snp_genotype.af_from_counts(counts, 0, bad, True)


def test_twin_on_a_hand_made_matrix():
    snps = np.array([[0, 0, -1, 3], [1, 0, 1, 3], [2, 1, 1, -1], [1, 1, 0, 0]], dtype=np.int8)
    assert sitestats_twin.site_counts(snps)[0].tolist() == [[2, 0, 0, 3], [1, 2, 0, 4], [0, 2, 1, 3], [2, 2, 0, 4]]
    sub = sitestats_twin.site_counts(snps, [[2, 0, 2], []], rows=[3, 3, 1])           # repeats count as listed
    assert sub[0].tolist() == [[2, 1, 0, 3], [2, 1, 0, 3], [0, 3, 0, 3]] and not sub[1].any()


# ------------------------------------------------------------------------------------------------ the library's validation
def test_refusals_that_need_no_device():
    lib = _lib.load()
    out = np.zeros((2, 5, 4), dtype=np.int32)
    cols = np.zeros(4, dtype=np.int32)

    def call(off, n_groups, n_rows, counts=out, cols=cols):
        off = None if off is None else np.asarray(off, dtype=np.int64)
        rc = lib.snpm_panel_site_counts(None, _lib.ptr(cols), _lib.ptr(off), n_groups, None, 0, n_rows, _lib.ptr(counts))
        return rc, lib.snpm_last_error(None).decode()
    assert call([0, 2, 4], -1, 5) == (_lib.SNPM_ERR_BADARG, "negative size")
    assert call([0, 2, 4], 2, -1) == (_lib.SNPM_ERR_BADARG, "negative size")
    rc, msg = call(list(range(34)), 33, 5)
    assert rc == _lib.SNPM_ERR_BADARG and "too many groups" in msg and "SNPM_SITE_MAX_GROUPS" in msg
    assert call([1, 2, 4], 2, 5) == (_lib.SNPM_ERR_BADARG, "grp_off must start at 0")
    assert call([0, 3, 2], 2, 5) == (_lib.SNPM_ERR_BADARG, "grp_off must not decrease")
    assert call(None, 2, 5) == (_lib.SNPM_ERR_BADARG, "grp_off is NULL with a column list")
    assert call([0, 2, 4], 2, 5, cols=None) == (_lib.SNPM_ERR_BADARG, "cols is NULL but grp_off lists columns")
    assert call(None, 2, 5, cols=None) == (_lib.SNPM_ERR_BADARG, "cols is NULL (all accessions): n_groups must be 1")
    assert call([0, 2, 4], 2, 5, counts=None) == (_lib.SNPM_ERR_BADARG, "counts is NULL")
    # sound arguments: only the panel is missing (no output is needed where there is no work; the group limit is inclusive)
    assert call([0, 2, 4], 2, 5) == (_lib.SNPM_ERR_BADARG, "panel is NULL")
    assert call([0, 2, 4], 2, 0, counts=None) == (_lib.SNPM_ERR_BADARG, "panel is NULL")
    assert call([0], 0, 5, counts=None) == (_lib.SNPM_ERR_BADARG, "panel is NULL")
    assert call(None, 1, 5, cols=None) == (_lib.SNPM_ERR_BADARG, "panel is NULL")
    assert call([0] * 33, 32, 5, counts=np.zeros((32, 5, 4), dtype=np.int32)) == (_lib.SNPM_ERR_BADARG, "panel is NULL")
    assert (out == 0).all()
    header = open(os.path.join(ROOT, "include", "snpmatch_hip.h")).read()
    assert "#define SNPM_SITE_MAX_GROUPS 32" in header and engine.SITE_MAX_GROUPS == 32
    kernel = open(os.path.join(ROOT, "snpmatch_amd", "csrc", "snpm_k_site.hpp")).read()
    assert "#define SNPM_SITE_MAX_GROUPS 32" in kernel
    assert 32 * 8 * 64 * 4 == 65536                                 # groups x words per lane x lanes x 4 B: the static LDS of a block
    assert "snpm_panel_site_counts" in _lib.SYMBOLS


def test_group_and_streamed_panels_are_refused_with_the_reason():
    for cls, why in ((engine.GroupPanel, "spread over several GPUs"), (engine.StreamedPanel, "not a resident panel")):
        with pytest.raises(TypeError, match="every accession column on one device") as err:
            engine.site_counts(cls.__new__(cls))
        assert why in str(err.value)
    for cls, why in ((engine.GroupPanel, "spread over several GPUs by accession"), (engine.StreamedPanel, "streamed through the device")):
        with pytest.raises(TypeError, match="every accession column of the DB on one device") as err:
            snp_genotype.Genotype.site_counts(_Holder(cls.__new__(cls)), None, None)
        assert why in str(err.value)


class _Holder(object):
    """stands in for a Genotype whose DB went to the given kind of panel"""

    def __init__(self, panel):
        self._panel = panel

    def panel(self):
        return self._panel


# ------------------------------------------------------------------------------------------------ layers of repeated columns
@pytest.fixture
def device_twin(monkeypatch):
    """``engine._site_counts_call`` answered by the twin on a panel of 40 accessions x 60 rows; it refuses what the library refuses"""
    rng = np.random.default_rng(5)
    snps = rng.choice(np.array([-1, 0, 1, 2, 3], dtype=np.int8), size=(60, 40), p=[0.15, 0.4, 0.3, 0.1, 0.05])
    calls = []

    def call(panel, col_lists, row_idx, row0, n_rows):
        calls.append(None if col_lists is None else [c.tolist() for c in col_lists])
        rows = row_idx if row_idx is not None else range(row0, row0 + n_rows)
        if col_lists is None:
            return sitestats_twin.site_counts(snps, None, rows)
        assert len(col_lists) <= engine.SITE_MAX_GROUPS
        assert all(c.dtype == np.int32 and len(np.unique(c)) == len(c) for c in col_lists), "a column twice in one group"
        return sitestats_twin.site_counts(snps, list(col_lists), rows)
    monkeypatch.setattr(engine, "_site_counts_call", call)
    panel = engine.Panel.__new__(engine.Panel)
    panel.h, panel.n_snp, panel.n_acc = None, 60, 40
    return panel, snps, calls


def test_repeats_travel_as_layers_of_distinct_columns(device_twin):
    panel, snps, calls = device_twin
    assert [l.tolist() for l in engine._site_layers([5, 3, 5, 9, 5, 3])] == [[3, 5, 9], [3, 5], [5]]
    assert [l.tolist() for l in engine._site_layers([])] == [[]] and [l.tolist() for l in engine._site_layers([7, 2])] == [[2, 7]]
    groups = [np.array([5, 3, 5, 9, 5, 3]), np.array([], dtype=np.int64), np.array([1, 2, 3]), np.array([0, 0])]
    got = engine.site_counts(panel, groups)
    assert got.dtype == np.int32 and got.shape == (4, 60, 4) and np.array_equal(got, sitestats_twin.site_counts(snps, groups))
    assert calls == [[[3, 5, 9], [3, 5], [5], [], [1, 2, 3], [0], [0]]]          # one call, seven layers
    assert not got[1].any() and np.array_equal(got[3], 2 * sitestats_twin.site_counts(snps, [[0]])[0])
    # None, one array, a plain list of indices; rows as a range, a slice, a list
    del calls[:]
    assert np.array_equal(engine.site_counts(panel), sitestats_twin.site_counts(snps)) and calls == [None]
    assert np.array_equal(engine.site_counts(panel, np.array([4, 4, 1]), range(5, 9)), sitestats_twin.site_counts(snps, [[4, 4, 1]], range(5, 9)))
    assert np.array_equal(engine.site_counts(panel, [4, 1], slice(50, None)), sitestats_twin.site_counts(snps, [[4, 1]], range(50, 60)))
    rows = np.array([7, 7, 59, 0])
    assert np.array_equal(engine.site_counts(panel, [[4, 1], [2]], rows), sitestats_twin.site_counts(snps, [[4, 1], [2]], rows))
    assert engine.site_counts(panel, [], rows).shape == (0, 4, 4) and engine.site_counts(panel, None, range(3, 3)).shape == (1, 0, 4)
    with pytest.raises(ValueError, match="step 1"):
        engine.site_counts(panel, None, range(0, 10, 2))
    with pytest.raises(TypeError, match="must be integers"):
        engine.site_counts(panel, [np.array([0.5, 1.0])])


def test_more_layers_than_one_call_holds_take_several_calls(device_twin):
    panel, snps, calls = device_twin
    rng = np.random.default_rng(6)
    groups = [rng.permutation(40)[:1 + k % 7] for k in range(engine.SITE_MAX_GROUPS + 1)]
    groups[31] = np.array([8, 8, 8, 2])                             # its three layers straddle the two calls
    got = engine.site_counts(panel, groups, range(10, 40))
    assert np.array_equal(got, sitestats_twin.site_counts(snps, groups, range(10, 40)))
    assert [len(c) for c in calls] == [32, 3] and calls[0][31] == [2, 8] and calls[1][:2] == [[8], [8]]


# ------------------------------------------------------------------------------------------------ Genotype and the command
@pytest.fixture
def toy(monkeypatch):
    """a DB of 12 accessions x 900 rows on two chromosomes; the device call is the twin"""
    rng = np.random.default_rng(78)
    snps = rng.choice(np.array([-1, 0, 1, 2], dtype=np.int8), size=(900, 12), p=[0.1, 0.5, 0.35, 0.05])
    snps[10] = 0                            # monomorphic everywhere
    snps[11] = -1                           # no informative accession
    snps[12] = 1                            # alt everywhere: polarised
    snps[13, :6], snps[13, 6:] = 1, 0       # common in the first six accessions, absent from the others
    snps[14, :6], snps[14, 6:] = [0, 0, 0, 1, 1, 1], [-1, -1, -1, -1, 0, 1]     # maf 0.5 in both halves, 4 of 6 missing in the second
    names = ["acc%02d" % i for i in range(12)]
    positions = np.concatenate([np.arange(10, 10 + 10 * 500, 10), np.arange(5, 5 + 10 * 400, 10)])
    g = snp_genotype.Genotype.from_arrays(snps, names, positions, ["Chr1", "Chr2"], [[0, 500], [500, 900]])
    calls = []

    def twin(panel, groups=None, rows=None):
        calls.append((groups, rows))
        return sitestats_twin.site_counts(snps, groups, rows)
    stub = engine.Panel.__new__(engine.Panel)
    stub.h = None
    monkeypatch.setattr(snp_genotype.Genotype, "panel", lambda self, ctx=None, packed=None: stub)
    monkeypatch.setattr(engine, "site_counts", twin)
    return g, snps, names, calls


def test_genotype_methods_against_the_host_functions(toy):
    g, snps, names, calls = toy
    maf, nind = g.get_af_snps(0, return_nind=True)
    want, num = snp_genotype.calculate_af_snp_mat(snps)
    assert same_bits(maf, want) and nind.dtype == np.int64 and np.array_equal(nind, num) and calls[-1] == (None, None)
    acc, rows = np.array([6, 9, 2, 6]), np.array([700, 3, 3, 250, 899, 12])
    got = g.get_af_snps(1, filter_snps_ix=rows, filter_acc_ix=acc, polarize_geno=0, return_maf=False)
    assert type(got) is np.ndarray and same_bits(got, snp_genotype.calculate_af_snp_mat(snps[rows][:, acc], 1, 0, False)[0])
    assert isinstance(calls[-1][1], np.ndarray)
    region = g.determine_snp_ix_given_bed("Chr2,100,2000")           # a run of rows travels as a dense range
    pops = {"a": np.array([0, 1, 2, 3, 4, 5]), "b": np.array([5, 6, 7, 7])}
    maf, nind = g.get_af_snps(2, True, region, pops)
    assert calls[-1][1] == range(510, 700) and list(maf) == list(nind) == ["a", "b"]
    for pop, ix in pops.items():
        want, num = snp_genotype.calculate_af_snp_mat(snps[510:700][:, ix], 2)
        assert same_bits(maf[pop], want) and nind[pop].dtype == np.float64 and np.array_equal(nind[pop], num)
    with pytest.raises(AssertionError, match="numpy arrays in a dictionary"):
        g.get_af_snps(0, filter_acc_ix={"a": [0, 1]})
    assert g.site_counts(pops, region).shape == (2, 190, 4)
    # the rows the reference's polarisation would flip
    for pg in (0, 1):
        mask = g.polarize_mask(polarize_geno=pg)
        assert mask.dtype == bool and np.array_equal(mask, (snp_genotype._polarize_snps(snps, pg) != snps).any(axis=1) | ((snps == pg).sum(axis=1) == 12))
        sub = g.polarize_mask(acc, rows, pg)
        assert np.array_equal(sub, (snps[rows][:, acc] == pg).sum(axis=1) > 2.0)
    assert g.polarize_mask()[12] and not g.polarize_mask()[13]      # all alt; exactly half alt
    with pytest.raises(ValueError, match="polarize_geno must be 0, 1 or 2"):
        g.polarize_mask(polarize_geno=3)
    with pytest.raises(TypeError, match="not a dict"):
        g.polarize_mask(pops)


def test_genotype_methods_reproduce_the_goldens_with_the_twin_as_device(golden_dir, monkeypatch):
    case = np.load(os.path.join(golden_dir, "sitestats_a7_r1001.npz"))
    snps = case["snps"]
    g = snp_genotype.Genotype.from_arrays(snps, ["A%d" % i for i in range(7)], np.arange(1, 1002), ["Chr1"], [[0, 1001]])
    stub = engine.Panel.__new__(engine.Panel)
    monkeypatch.setattr(snp_genotype.Genotype, "panel", lambda self, ctx=None, packed=None: stub)
    monkeypatch.setattr(engine, "site_counts", lambda panel, groups=None, rows=None: sitestats_twin.site_counts(snps, groups, rows))
    n = 0
    for call, acc_ix, rows, mi, pg, maf, want in method_calls(case):
        got, nind = g.get_af_snps(mi, True, rows, acc_ix, pg, maf)
        for pop, ref in want.items():
            assert same_bits(got if pop is None else got[pop], ref[0]) and np.array_equal(nind if pop is None else nind[pop], ref[1]), call
            n += 1
    assert n == 8


def test_command_line_writes_the_three_files(toy, tmp_path, monkeypatch):
    g, snps, names, calls = toy
    monkeypatch.setattr(snp_genotype, "Genotype", lambda hdf5_file, hdf5_acc_file: g)
    db = tmp_path / "db.npz"
    db.write_bytes(b"")
    out = str(tmp_path / "out")
    # the whole panel as one population: two files, no site list without a threshold
    assert cli.main(["sitestats", "-d", str(db), "-o", out]) == 0
    z = np.load(out + ".sitestats.npz")
    want = sitestats_twin.site_counts(snps)
    assert z["populations"].tolist() == ["all"] and z["n_listed"].tolist() == [12]
    assert z["counts"].dtype == np.int32 and np.array_equal(z["counts"], want) and np.array_equal(z["nind"], want[:, :, 3]) and z["nind"].dtype == np.int64
    assert same_bits(z["maf"][0], snp_genotype.calculate_af_snp_mat(snps)[0]) and same_bits(z["af"][0], snp_genotype.calculate_af_snp_mat(snps, return_maf=False)[0])
    assert z["chr"].tolist() == ["Chr1"] * 500 + ["Chr2"] * 400 and np.array_equal(z["pos"], g.g.positions)
    assert not os.path.exists(out + ".sites.tsv")
    stats = json.load(open(out + ".sitestats.json"))["stats"]["all"]
    c = want[0].astype(np.int64)
    assert stats["rows"] == 900 and stats["accessions"] == 12 and stats["no_informative"] == int((c[:, 3] == 0).sum()) >= 1
    assert stats["monomorphic"] == int(((c[:, 3] > 0) & (c[:, :3].max(axis=1) == c[:, 3])).sum()) >= 2
    assert stats["polarised"] == int((c[:, 1] > 6).sum()) >= 1
    assert sum(stats["maf_histogram"]) == 900 - stats["no_informative"] and len(stats["maf_histogram"]) == 10
    # two populations, a region, both thresholds: a row passes only when it passes in EVERY population
    pop_file = tmp_path / "pops.tsv"
    pop_file.write_text("# accession population\n" + "".join("acc%02d\t%s\n" % (i, "west" if i < 6 else "east") for i in range(12)) + "\n")
    assert cli.main(["sitestats", "-d", str(db), "--pops", str(pop_file), "--bed", "Chr1,1,100000", "--min_maf", "0.2", "--max_missing", "0.5", "-o", out]) == 0
    z = np.load(out + ".sitestats.npz")
    assert z["populations"].tolist() == ["west", "east"] and z["counts"].shape == (2, 500, 4) and calls[-1][1] == range(0, 500)
    groups = [np.arange(6), np.arange(6, 12)]
    assert np.array_equal(z["counts"], sitestats_twin.site_counts(snps, groups, range(0, 500)))
    maf = np.array([snp_genotype.calculate_af_snp_mat(snps[:500][:, ix])[0] for ix in groups])
    missing = 1 - z["counts"][:, :, 3] / 6.0
    with np.errstate(invalid="ignore"):
        keep = ((maf >= 0.2) & (missing <= 0.5)).all(axis=0)
    lines = open(out + ".sites.tsv").read().splitlines()
    assert lines[0].split("\t") == ["chr", "pos", "maf_west", "missing_west", "maf_east", "missing_east"]
    assert [int(ln.split("\t")[1]) for ln in lines[1:]] == g.g.positions[:500][keep].tolist() and 0 < keep.sum() < 500
    passed = set(int(ln.split("\t")[1]) for ln in lines[1:])
    assert g.g.positions[13] not in passed                          # maf 0.5 in the west, 0 in the east
    assert g.g.positions[14] not in passed                          # maf passes in both, four of six missing in the east
    row = dict((int(ln.split("\t")[1]), ln.split("\t")) for ln in lines[1:])[int(g.g.positions[:500][keep][0])]
    k = int(np.flatnonzero(keep)[0])
    assert row[2] == repr(float(maf[0, k])) and row[5] == repr(float(missing[1, k]))
    assert set(json.load(open(out + ".sitestats.json"))["stats"]) == {"west", "east"}
    # only one threshold: the other does not filter
    assert cli.main(["sitestats", "-d", str(db), "--pops", str(pop_file), "--bed", "Chr1,1,100000", "--max_missing", "0.5", "-o", out]) == 0
    assert len(open(out + ".sites.tsv").read().splitlines()) - 1 == int((missing <= 0.5).all(axis=0).sum())
    # an accession list is one population, in file order, a repeat as listed
    acc_file = tmp_path / "accs.txt"
    acc_file.write_text("acc09\nacc06\nacc09\n")
    assert cli.main(["sitestats", "-d", str(db), "-a", str(acc_file), "-o", out]) == 0
    z = np.load(out + ".sitestats.npz")
    assert z["populations"].tolist() == ["listed"] and z["n_listed"].tolist() == [3] and np.array_equal(z["counts"], sitestats_twin.site_counts(snps, [[9, 6, 9]]))


def test_command_line_refuses_bad_population_files(toy, tmp_path, monkeypatch, caplog):
    g, snps, names, calls = toy
    monkeypatch.setattr(snp_genotype, "Genotype", lambda hdf5_file, hdf5_acc_file: g)
    db = tmp_path / "db.npz"
    db.write_bytes(b"")
    out = str(tmp_path / "out")
    pop_file = tmp_path / "pops.tsv"
    pop_file.write_text("acc01 west\nnobody east\n")
    assert cli.main(["sitestats", "-d", str(db), "--pops", str(pop_file), "-o", out]) == 2
    assert "accessions not in the database: nobody" in caplog.text
    pop_file.write_text("acc01 west\nacc02\n")
    assert cli.main(["sitestats", "-d", str(db), "--pops", str(pop_file), "-o", out]) == 2
    assert "line 2: expected an accession and a population" in caplog.text
    pop_file.write_text("# nothing\n")
    assert cli.main(["sitestats", "-d", str(db), "--pops", str(pop_file), "-o", out]) == 2
    assert "names no accession" in caplog.text
    acc_file = tmp_path / "accs.txt"
    acc_file.write_text("acc01\n")
    pop_file.write_text("acc01 west\n")
    assert cli.main(["sitestats", "-d", str(db), "--pops", str(pop_file), "-a", str(acc_file), "-o", out]) == 2
    assert "not both" in caplog.text
    assert not os.path.exists(out + ".sitestats.npz")
    with pytest.raises(ValueError, match="names no accession"):
        sitestats.populations_of(g, {"popFile": None, "accFile": _empty(tmp_path)})


def _empty(tmp_path):
    path = tmp_path / "empty.txt"
    path.write_text("\n")
    return str(path)


# ------------------------------------------------------------------------------------------------ the kernel, on the host
def test_kernel_source_on_the_host_under_asan_and_ubsan(tmp_path):
    """every block of k_site_counts run by 512 real threads with a barrier, exact-size heap buffers, arbitrary pad bytes, a stale
    workspace: 1 / 2 / 31 / 32 / 33 / 63 / 64 / 65 / 130 / 1135 accessions x 0 / 1 / 63 / 64 / 65 rows in the three layouts (the
    split layout at 1135 accessions included), 1 / 2 / 3 / SNPM_SITE_MAX_GROUPS groups with an empty, a one-column and overlapping
    groups, rows of a pitch that takes the byte loads, a whole wave per row, a row list with repeats, two slabs"""
    cases = host_kernel_util.run_driver("site_host_driver", tmp_path)
    assert len(cases) == 62
    assert sum("slabs=2" in ln for ln in cases) == 2 and sum("wide=0" in ln for ln in cases) >= 5
    assert {1, 8, 32, 64} <= set(int(ln.split("lanes=")[1].split()[0]) for ln in cases)       # lanes per row: a row per lane .. a whole wave
    assert sum("groups=32 " in ln for ln in cases) >= 10 and any("layout=2 acc=1135" in ln for ln in cases)
