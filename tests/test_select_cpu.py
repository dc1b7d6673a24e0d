"""
The selection layer under the panel commands, without a device: what the ten resident-panel scans of ``engine`` hand to the C entry
points for every form of ``rows`` and ``cols`` (a recording stub stands in for the library), what ``Genotype`` hands to the scans,
and the accession / row selection of the commands (``core/_select.py``) with its refusals, word for word.
"""
import ctypes as C
import os

import numpy as np
import pytest

from snpmatch_amd import engine
from snpmatch_amd.core import (_select, admixture, f1search, ibd, kinship, ld, markers, mosaic, parentsearch, pca, power, sitestats,
                               snp_genotype, windows)

N_SNP, N_ACC = 50, 9


# ------------------------------------------------------------------------------------------------ (a) the scans and the C entry points
class _RecordingLib(object):
    """every ``snpm_*`` entry point records its name and arguments and reports success"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


def _stub_panel():
    lib = _RecordingLib()
    ctx = object.__new__(engine.Context)
    ctx.lib, ctx.h = lib, None                  # (h None: Context.__del__ has nothing to close)
    panel = object.__new__(engine.Panel)
    panel.ctx, panel.h, panel.n_snp, panel.n_acc = ctx, None, N_SNP, N_ACC
    return panel, lib


def _array_at(pointer, n, ctype):
    return None if pointer is None else np.array((ctype * n).from_address(pointer.value))


# scan -> (the call with every other argument valid for n_rows rows and ncols columns, the limit's name or None)
SCANS = {
    "kinship_counts": (lambda p, c, r, nr, nc: engine.kinship_counts(p, c, r), "KIN"),
    "f1_counts": (lambda p, c, r, nr, nc: engine.f1_counts(p, np.zeros(nr, np.uint8), c, r), "F1X"),
    "parent_counts": (lambda p, c, r, nr, nc: engine.parent_counts(p, np.zeros(nr, np.uint8), [0, nr], 1, c, r), "F1X"),
    "ibd_counts": (lambda p, c, r, nr, nc: engine.ibd_counts(p, [0, nr], cols=c, rows=r), "F1X"),
    "gram": (lambda p, c, r, nr, nc: engine.gram(p, np.zeros((nr, 4)), c, r), "PCA"),
    "loadings": (lambda p, c, r, nr, nc: engine.loadings(p, np.zeros((nr, 4)), np.zeros((nc, 2)), c, r), None),
    "admix": (lambda p, c, r, nr, nc: engine.admix(p, np.full((nc, 2), 0.5), np.full((nr, 2), 0.5), 1, c, r), None),
    "marker_select": (lambda p, c, r, nr, nc: engine.marker_select(p, cols=c, rows=r), "MK"),
    "sim_counts": (lambda p, c, r, nr, nc: engine.sim_counts(p, [0, nr], 0.01, 1, c, r), "SIM"),
    "mosaic": (lambda p, c, r, nr, nc: engine.mosaic(p, np.zeros((1, nr), np.uint8), [0, nr], np.zeros((3, 4), dtype=np.int64), 5, c, r), "MOS"),
}
ROW_LIST = np.array([7, 3, 3, 49, 0])
# rows -> the library's (row_idx, row0, n_rows)
ROW_FORMS = [(None, (None, 0, N_SNP)), (slice(3, 40), (None, 3, 37)), (range(3, 40), (None, 3, 37)), (ROW_LIST, (ROW_LIST, 0, 5))]
COL_FORMS = [(None, (None, N_ACC)), ([4, 0, 4, 8], ([4, 0, 4, 8], 4))]


@pytest.mark.parametrize("scan", sorted(SCANS))
def test_rows_and_cols_reach_the_c_entry_point(scan):
    call, _ = SCANS[scan]
    for rows, (want_idx, want_row0, want_n) in ROW_FORMS:
        for cols, (want_cols, want_ncols) in COL_FORMS:
            panel, lib = _stub_panel()
            seen = []

            def entry(h, p_cols, ncols, p_rows, row0, n_rows, *rest):      # the common head of the ten entry points
                seen.append((_array_at(p_cols, ncols, C.c_int32), ncols, _array_at(p_rows, n_rows, C.c_int64), row0, n_rows))
                return 0
            lib.__dict__["snpm_panel_" + scan] = entry
            call(panel, cols, rows, want_n, want_ncols)
            assert len(seen) >= 1 and not lib.calls, "one entry point, the scan's own"
            for got_cols, ncols, got_idx, row0, n_rows in seen:
                assert (ncols, row0, n_rows) == (want_ncols, want_row0, want_n)
                assert got_cols is None if want_cols is None else (got_cols.dtype == np.int32 and got_cols.tolist() == want_cols)
                assert got_idx is None if want_idx is None else (got_idx.dtype == np.int64 and got_idx.tolist() == want_idx.tolist())


@pytest.mark.parametrize("scan", sorted(s for s in SCANS if SCANS[s][1]))
def test_too_many_columns_are_refused_before_the_library(scan, monkeypatch):
    call, limit_name = SCANS[scan]
    limit = getattr(engine, limit_name + "_MAX_ACCESSIONS")
    panel, lib = _stub_panel()
    with pytest.raises(AssertionError) as err:
        call(panel, np.zeros(limit + 1, dtype=np.int32), slice(0, 4), 4, limit + 1)
    assert str(err.value) == "too many accessions for one call: %d, at most %d (SNPM_%s_MAX_ACCESSIONS)" % (limit + 1, limit, limit_name)
    assert not lib.calls
    monkeypatch.setattr(engine, limit_name + "_MAX_ACCESSIONS", 6)         # (the limit itself passes: shown at a size that costs nothing)
    with pytest.raises(AssertionError, match="7, at most 6"):
        call(panel, np.zeros(7, dtype=np.int32), slice(0, 4), 4, 7)
    assert not lib.calls
    call(panel, np.zeros(6, dtype=np.int32), slice(0, 4), 4, 6)
    assert len(lib.calls) >= 1


def test_scans_refuse_what_is_not_a_resident_panel():
    for scan, (call, _) in SCANS.items():
        with pytest.raises(TypeError) as err:
            call(object(), None, None, N_SNP, N_ACC)
        assert str(err.value) == ("%s needs every accession column on one device: a object is not a resident panel, load the DB as one resident "
                                  "panel (int8 or packed) on one GPU" % scan)


# ------------------------------------------------------------------------------------------------ (b) Genotype -> scan
def test_rows_or_range():
    rr = snp_genotype._rows_or_range
    assert rr([5, 6, 7, 8]) == range(5, 9) and rr(range(5, 9)) == range(5, 9) and isinstance(rr(range(5, 9)), range)
    got = rr([5, 7])
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.tolist() == [5, 7]
    assert rr(None) is None


# method -> the call with the row filter last in the lambda, and the engine function it must reach
PASS_THROUGHS = {
    "kinship_counts": lambda g, r: g.kinship_counts(None, r),
    "f1_counts": lambda g, r: g.f1_counts(np.zeros(4, np.uint8), None, r),
    "parent_counts": lambda g, r: g.parent_counts(np.zeros(4, np.uint8), [0, 4], 1, None, r),
    "ibd_counts": lambda g, r: g.ibd_counts([0, 4], filter_snp_ix=r),
    "marker_select": lambda g, r: g.marker_select(filter_snp_ix=r),
    "gram": lambda g, r: g.gram(np.zeros((4, 4)), None, r),
    "loadings": lambda g, r: g.loadings(np.zeros((4, 4)), np.zeros((N_ACC, 1)), None, r),
    "admix": lambda g, r: g.admix(np.zeros((N_ACC, 2)), np.zeros((4, 2)), 1, None, r),
    "sim_counts": lambda g, r: g.sim_counts([0, 4], 0.0, 1, None, r),
    "mosaic": lambda g, r: g.mosaic(np.zeros((1, 4), np.uint8), [0, 4], np.zeros((3, 4), dtype=np.int64), 5, None, r),
    "site_counts": lambda g, r: g.site_counts(None, r),
    "ld_band": lambda g, r: g.ld_band(2, None, r),
    "window_counts": lambda g, r: g.window_counts([0, 4], None, None, r),
}


@pytest.mark.parametrize("method", sorted(PASS_THROUGHS))
def test_genotype_hands_a_range_on_as_a_range(method, monkeypatch):
    g = snp_genotype.Genotype.from_arrays(np.zeros((N_SNP, N_ACC), dtype=np.int8), ["a%d" % i for i in range(N_ACC)], np.arange(N_SNP), ["1"], [[0, N_SNP]])
    panel, _ = _stub_panel()
    monkeypatch.setattr(snp_genotype.Genotype, "panel", lambda self, ctx=None, packed=None: panel)
    seen = []

    def scan(*args, **kwargs):
        seen.append(args)
        return "result"
    monkeypatch.setattr(engine, method, scan)           # looked up when the method runs
    for rows in (range(5, 9), [5, 6, 7, 8]):
        assert PASS_THROUGHS[method](g, rows) == "result"
        got = [a for a in seen[-1] if isinstance(a, range)]
        assert seen[-1][0] is panel and got == [range(5, 9)]


# ------------------------------------------------------------------------------------------------ (c) the commands' selection
@pytest.fixture(scope="module")
def toy(golden_dir):
    z = np.load(os.path.join(golden_dir, "toy_db.npz"))
    return snp_genotype.Genotype.from_arrays(z["snps"], z["accs"], z["positions"], z["chrs"], z["regions"])


class _Reached(Exception):
    """the selection was accepted: the command went on to its scan"""


def _raise_reached(*args, **kwargs):
    raise _Reached(args)


# command -> (entry point, what it reaches after the selection as (owner, attribute), the position of the accession indices among
# the arguments of that, the "twice" refusal or None)
LIST_TWICE = "the accession list %s names an accession twice"
LISTED_TWICE = "an accession is listed twice (%s)"
COMMANDS = {
    "kinship": (kinship.potatoKinship, (snp_genotype.Genotype, "kinship_counts"), 1, None),
    "sitestats": (sitestats.potatoSiteStats, (snp_genotype.Genotype, "site_counts"), 1, None),
    "ld": (ld.potatoLD, (snp_genotype.Genotype, "ld_band"), 2, LIST_TWICE),
    "windows": (windows.potatoWindows, (snp_genotype.Genotype, "genome_window_counts"), 3, None),
    "f1search": (f1search.potatoF1Search, (f1search, "F1Search"), 5, None),
    "parentsearch": (parentsearch.potatoParentSearch, (parentsearch, "ParentSearch"), 8, None),
    "power": (power.potatoPower, (power, "Power"), 6, None),
    "mosaic": (mosaic.potatoMosaic, (mosaic, "Mosaic"), 10, None),
    "ibd": (ibd.potatoIBD, (ibd, "genome_ibd"), 6, None),
    "markers": (markers.potatoMarkers, (snp_genotype.Genotype, "marker_select"), 6, LIST_TWICE),
    "pca": (pca.potatoPCA, (snp_genotype.Genotype, "site_counts"), 1, LISTED_TWICE),
    "admixture": (admixture.potatoAdmixture, (snp_genotype.Genotype, "site_counts"), 1, LISTED_TWICE),
}


def _args(tmp_path, **more):
    args = {"hdf5File": "db", "hdf5accFile": None, "outFile": str(tmp_path / "out"), "inFile": "sample.bed", "levels": "10,20", "K": 2, "components": 2}
    args.update(more)
    return args


@pytest.fixture
def command(request, toy, monkeypatch):
    entry, (owner, attribute), at, twice = COMMANDS[request.param]
    monkeypatch.setattr(snp_genotype, "Genotype", lambda hdf5_file, hdf5_acc_file: toy)
    monkeypatch.setattr(f1search.snpmatch, "parse_inputs_once", lambda path, log_debug=False: None)
    monkeypatch.setattr(mosaic, "read_samples", lambda path, log_debug=False: (["s"], None, None, None))
    monkeypatch.setattr(owner, attribute, _raise_reached)
    return request.param, entry, at, twice


def _selected(reached, name, at):
    got = reached.value.args[0][at]
    return got["listed"] if name == "sitestats" else got


@pytest.mark.parametrize("command", sorted(COMMANDS), indirect=True)
def test_accession_list_of_every_command(command, toy, tmp_path):
    name, entry, at, twice = command
    acc_file = tmp_path / "accs.txt"
    names = [str(a) for a in toy.accessions]
    # the list in its order
    acc_file.write_text("# picked\n%s\n%s extra\n\n%s\n" % (names[7], names[2], names[30]))
    with pytest.raises(_Reached) as reached:
        entry(_args(tmp_path, accFile=str(acc_file)))
    got = _selected(reached, name, at)
    assert got.dtype == np.int64 and got.tolist() == [7, 2, 30]
    # no list: every accession
    with pytest.raises(_Reached) as reached:
        entry(_args(tmp_path))
    got = reached.value.args[0][at]
    assert got is None
    # an empty list
    acc_file.write_text("# nobody\n\n")
    with pytest.raises(ValueError) as err:
        entry(_args(tmp_path, accFile=str(acc_file)))
    assert str(err.value) == "the accession list %s names no accession" % acc_file
    # unknown names: the first ten
    unknown = ["x%d" % i for i in range(12)]
    acc_file.write_text("\n".join([names[0]] + unknown) + "\n")
    with pytest.raises(ValueError) as err:
        entry(_args(tmp_path, accFile=str(acc_file)))
    assert str(err.value) == "accessions not in the database: " + ", ".join(unknown[:10])
    # a name twice: refused where the columns must differ, a column twice elsewhere
    acc_file.write_text("%s\n%s\n%s\n" % (names[3], names[5], names[3]))
    if twice is not None:
        with pytest.raises(ValueError) as err:
            entry(_args(tmp_path, accFile=str(acc_file)))
        assert str(err.value) == twice % acc_file
    else:
        with pytest.raises(_Reached) as reached:
            entry(_args(tmp_path, accFile=str(acc_file)))
        assert _selected(reached, name, at).tolist() == [3, 5, 3]


@pytest.mark.parametrize("command", ["ld", "markers", "pca", "admixture", "power"], indirect=True)
def test_bed_and_sites_exclude_each_other(command, tmp_path):
    _, entry, _, _ = command
    with pytest.raises(ValueError) as err:
        entry(_args(tmp_path, bed="1,1,100000", sitesFile=str(tmp_path / "no_such_file.tsv")))
    assert str(err.value) == "give either --bed or --sites, not both"


def _rows_as_the_commands_chose_them(g, args):
    """the block that ld, markers, pca and admixture each carried before ``_select.rows_of``"""
    if args.get('sitesFile'):
        return ld.rows_of_sites(g, *ld.read_sites(args['sitesFile']))
    if args.get('bed'):
        return np.asarray(g.determine_snp_ix_given_bed(args['bed']), dtype=np.int64)
    return np.arange(len(g.g.positions), dtype=np.int64)


def test_rows_of(toy, tmp_path):
    positions = np.asarray(toy.g.positions)
    sites = tmp_path / "picked.sites.tsv"
    picked = [2500, 17, 9999, 17, 4000]                      # any order, a site twice, chromosome ends
    chrs = _select.row_chromosomes(toy, np.array(picked))
    sites.write_text("chr\tpos\tmaf_all\n" + "".join("%s\t%d\t0.1\n" % (c, positions[r]) for c, r in zip(chrs, picked)) + "\n")
    for args in ({"sitesFile": str(sites)}, {"bed": "2,1,400000"}, {"bed": "Chr5,1,2"}, {}):
        got, want = _select.rows_of(toy, args), _rows_as_the_commands_chose_them(toy, args)
        assert got.dtype == np.int64 and got.dtype == want.dtype and np.array_equal(got, want)
    assert _select.rows_of(toy, {"sitesFile": str(sites)}).tolist() == [17, 2500, 4000, 9999]
    assert len(_select.rows_of(toy, {"bed": "2,1,400000"})) > 0 and len(_select.rows_of(toy, {})) == len(positions)
    with pytest.raises(ValueError) as err:
        _select.rows_of(toy, {"bed": "2,1,400000", "sitesFile": str(sites)})
    assert str(err.value) == "give either --bed or --sites, not both"


def test_old_names_stay_importable():
    assert kinship.read_accession_list is _select.read_accession_list and sitestats.read_populations is _select.read_populations
    assert ld.read_sites is _select.read_sites and ld.rows_of_sites is _select.rows_of_sites
    assert sitestats.row_chromosomes is _select.row_chromosomes and f1search.hard_classes is _select.hard_classes
    assert mosaic.read_samples is _select.read_samples
