"""markers without a GPU: the numpy twin (tests/markers_twin.py) against a brute-force loop over rows and pairs on a few hundred small
seeded cases, with the invariants of the greedy loop checked on every one; a hand-made matrix whose picks are worked out by hand;
every refusal of ``snpm_panel_marker_select`` that needs no device and the refusal of group and streamed panels; the ``markers``
subcommand with the twin in the place of the device on a planted panel; and the kernel source itself, compiled for the host and
run by real threads under AddressSanitizer + UBSan (tests/mk_host_driver.cpp on tests/host_kernel/, a stand-alone child process)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import host_kernel_util
import markers_twin as twin
from snpmatch_amd import _lib, cli, engine
from snpmatch_amd.core import markers, snp_genotype


# ------------------------------------------------------------------------------------------------ the twin
def _case(seed):
    """a small seeded case: <= 12 accessions, <= 40 rows; depth 1 .. 3 and 255, masks, min_dist, duplicate rows and columns,
    all-missing and all-het panels"""
    rng = np.random.default_rng(seed)
    n_acc, n_rows = int(rng.integers(1, 13)), int(rng.integers(0, 41))
    snps = rng.choice(np.array([-1, 0, 1, 2, 3], dtype=np.int8), size=(n_rows, n_acc), p=[0.1, 0.45, 0.35, 0.07, 0.03])
    kind = seed % 10
    if kind == 7:
        snps[:] = -1                                                        # all missing
    if kind == 8:
        snps[:] = 2                                                         # all het
    kw = {"depth": (1, 2, 3, 255)[seed % 4]}
    if seed % 3 == 0:
        kw["max_markers"] = int(rng.integers(0, 8))
    if seed % 2:
        kw["coord"], kw["min_dist"] = rng.integers(-10, 10, size=n_rows), int(rng.integers(0, 6))
    if kind in (1, 4):
        kw["eligible"] = (rng.random(n_rows) < 0.7).astype(np.uint8) * int(rng.integers(1, 256))
    if kind in (2, 5) and n_rows:
        kw["rows"] = rng.integers(0, n_rows, size=int(rng.integers(1, 41)))       # a row list with duplicate rows
    if kind in (3, 5):
        kw["cols"] = rng.integers(0, n_acc, size=int(rng.integers(1, 13)))        # ... with duplicate columns
    if "rows" in kw:
        for k in ("coord", "eligible"):
            if k in kw:
                kw[k] = np.resize(kw[k], len(kw["rows"])) if len(kw[k]) else np.zeros(len(kw["rows"]), dtype=np.int64)
    return snps, kw


def _invariants(snps, kw, got):
    h0, h1 = twin.planes(snps, kw.get("cols"), kw.get("rows"))
    n_rows, ncols = h0.shape
    depth, need = kw["depth"], got["need"]
    initial = depth * (ncols * (ncols - 1) // 2)
    upper = np.triu(np.ones((ncols, ncols), dtype=bool), 1)
    assert got["remaining"] == int(need[upper].astype(np.int64).sum()) and np.array_equal(need, need.T) and not np.diag(need).any()
    assert int(got["gain_at"].astype(np.int64).sum()) == initial - got["remaining"]
    assert got["n_chosen"] == len(got["chosen"]) == len(got["gain_at"]) == len(set(got["chosen"].tolist()))
    if depth == 1:
        assert (np.diff(got["gain_at"]) <= 0).all()                         # gains never grow while a pair is needed once
    assert np.array_equal(twin.replay(snps, got["chosen"], depth, kw.get("cols"), kw.get("rows")), need)
    max_markers = twin.NO_LIMIT if kw.get("max_markers") is None else kw["max_markers"]
    assert got["n_chosen"] <= min(max_markers, n_rows)
    if got["stop_reason"] == twin.STOP_RESOLVED:
        assert got["remaining"] == 0
    elif got["stop_reason"] == twin.STOP_MAX_MARKERS:
        assert got["n_chosen"] == max_markers and got["remaining"] > 0
    else:
        # no row that is still eligible separates a pair in need
        elig = np.ones(n_rows, dtype=bool) if kw.get("eligible") is None else np.asarray(kw["eligible"]) != 0
        for r in got["chosen"].tolist():
            elig[r] = False
            if kw.get("coord") is not None:
                elig &= np.abs(np.asarray(kw["coord"], dtype=np.int64) - int(kw["coord"][r])) >= kw["min_dist"]
        assert got["remaining"] > 0 and not (twin.gains(h0, h1, need > 0)[elig] > 0).any()
    if got["n_chosen"] and got["first_gain"] is not None:
        assert got["first_gain"][got["chosen"][0]] == got["gain_at"][0]


@pytest.mark.parametrize("block", range(6))
def test_twin_against_brute_force_and_the_invariants(block):
    reasons = set()
    for seed in range(60 * block, 60 * block + 60):
        snps, kw = _case(seed)
        got, want = twin.marker_select(snps, **kw), twin.brute_force(snps, **kw)
        assert twin.same(got, want), (seed, got, want)
        _invariants(snps, kw, got)
        reasons.add(got["stop_reason"])
    assert reasons == {0, 1, 2}


#        A   B   C   D      separates                 first_gain
HAND = [[0,  0,  1,  1],    # AC AD BC BD             4
        [0,  1,  0,  1],    # AB AD BC CD             4
        [1,  0,  0,  2],    # AB AC      (D is a het) 2
        [0,  1,  1,  0],    # AB AC BD CD             4
        [-1, 0,  1,  3]]    # BC  (A missing, D "other") 1


def test_twin_on_a_hand_made_matrix():
    """Six pairs.  depth 1: round 0 has the gains 4 4 2 4 1 -- rows 0, 1 and 3 tie, the smallest position wins: row 0; AB and CD are
    left.  Round 1: row 1 separates AB and CD (2), row 2 AB (1), row 3 AB and CD (2), row 4 nothing in need -- rows 1 and 3 tie: row
    1; nothing is left: chosen 0, 1 with gains 4, 2, stop reason 0.
    depth 2: row 0 (4) leaves AB and CD at 2, the other four at 1; round 1: row 1 = AB AD BC CD = 4, row 3 = AB AC BD CD = 4, the
    tie goes to row 1, which leaves AB AC BD CD at 1; round 2: row 3 separates exactly those: chosen 0, 1, 3, gains 4, 4, 4.
    Row 0 masked, depth 1: rows 1 and 3 tie at 4: row 1, leaving AC and BD; row 2 = AC (1), row 3 = AC BD (2): chosen 1, 3.
    Rows 2 and 4 only: position 0 (AB AC, 2), then position 1 (BC, 1), then no row is left: reason 2 with AD, BD, CD in need.
    Coordinates 10 12 30 11 50, min_dist 3: the pick of row 0 excludes rows 1 and 3 (|12 - 10|, |11 - 10| < 3); row 2 separates AB
    (1); row 4 separates nothing in need: reason 2 with CD left."""
    snps = np.array(HAND, dtype=np.int8)
    got = twin.marker_select(snps)
    assert got["first_gain"].tolist() == [4, 4, 2, 4, 1] and got["first_gain"].dtype == np.int32
    assert (got["chosen"].tolist(), got["gain_at"].tolist(), got["remaining"], got["stop_reason"]) == ([0, 1], [4, 2], 0, 0)
    assert not got["need"].any() and got["need"].dtype == np.uint8 and got["chosen"].dtype == np.int64
    got = twin.marker_select(snps, depth=2)
    assert (got["chosen"].tolist(), got["gain_at"].tolist(), got["remaining"], got["stop_reason"]) == ([0, 1, 3], [4, 4, 4], 0, 0)
    got = twin.marker_select(snps, eligible=[0, 1, 1, 1, 1])
    assert (got["chosen"].tolist(), got["gain_at"].tolist(), got["stop_reason"]) == ([1, 3], [4, 2], 0) and got["first_gain"][0] == 4
    got = twin.marker_select(snps, max_markers=1)
    assert (got["chosen"].tolist(), got["remaining"], got["stop_reason"]) == ([0], 2, 1) and got["need"][0, 1] == got["need"][3, 2] == 1
    got = twin.marker_select(snps, rows=[2, 4])
    assert (got["chosen"].tolist(), got["gain_at"].tolist(), got["remaining"], got["stop_reason"]) == ([0, 1], [2, 1], 3, 2)
    assert np.argwhere(np.triu(got["need"])).tolist() == [[0, 3], [1, 3], [2, 3]]
    got = twin.marker_select(snps, coord=[10, 12, 30, 11, 50], min_dist=3)
    assert (got["chosen"].tolist(), got["gain_at"].tolist(), got["remaining"], got["stop_reason"]) == ([0, 2], [4, 1], 1, 2) and got["need"][2, 3] == 1
    # min_dist 2 keeps row 1 (|12 - 10| = 2 is not < 2): the picks of the plain call
    assert twin.marker_select(snps, coord=[10, 12, 30, 11, 50], min_dist=2)["chosen"].tolist() == [0, 1]
    # a repeated column is a pair nothing separates: A A B -- row 1 separates both A-B pairs, the A-A pair stays
    got = twin.marker_select(snps, cols=[0, 0, 1])
    assert (got["chosen"].tolist(), got["gain_at"].tolist(), got["remaining"], got["stop_reason"]) == ([1], [2], 1, 2) and got["need"][0, 1] == 1
    # depth 255: need never reaches 0, every row with a gain is picked once, largest first
    got = twin.marker_select(snps, depth=255)
    assert (got["chosen"].tolist(), got["gain_at"].tolist(), got["stop_reason"]) == ([0, 1, 3, 2, 4], [4, 4, 4, 2, 1], 2) and got["remaining"] == 6 * 255 - 15
    # calls that launch nothing: the initial state, first_gain zeros
    got = twin.marker_select(snps, max_markers=0)
    assert (got["n_chosen"], got["remaining"], got["stop_reason"]) == (0, 6, 1) and not got["first_gain"].any() and got["need"].sum() == 12
    got = twin.marker_select(snps, cols=[2])
    assert (got["n_chosen"], got["remaining"], got["stop_reason"]) == (0, 0, 0) and got["need"].tolist() == [[0]]
    got = twin.marker_select(snps, rows=range(2, 2))
    assert (got["n_chosen"], got["remaining"], got["stop_reason"]) == (0, 6, 2) and got["first_gain"].shape == (0,)


# ------------------------------------------------------------------------------------------------ the library's validation
def test_refusals_that_need_no_device():
    lib = _lib.load()
    cols = np.zeros(3, dtype=np.int32)
    coord = np.zeros(5, dtype=np.int64)
    chosen, gain_at = np.zeros(5, dtype=np.int64), np.zeros(5, dtype=np.int32)
    need = np.zeros((3, 3), dtype=np.uint8)
    first = np.zeros(5, dtype=np.int32)

    def call(ncols=3, n_rows=5, depth=1, max_markers=5, min_dist=0, coord=None, cols=cols, outs=(True, True, True), need=need, chosen=chosen, gain_at=gain_at,
             first=first):
        scal = [C.c_int64(0), C.c_int64(0), C.c_int32(0)]
        refs = [C.byref(s) if on else None for s, on in zip(scal, outs)]
        rc = lib.snpm_panel_marker_select(None, _lib.ptr(cols), ncols, None, 0, n_rows, _lib.ptr(coord), min_dist, None, depth, max_markers, _lib.ptr(chosen),
                                          _lib.ptr(gain_at), refs[0], refs[1], refs[2], _lib.ptr(need), _lib.ptr(first))
        return rc, lib.snpm_last_error(None).decode()
    bad = _lib.SNPM_ERR_BADARG
    assert call(ncols=-1) == (bad, "negative size") and call(n_rows=-1) == (bad, "negative size") and call(max_markers=-1) == (bad, "negative size")
    for depth in (0, 256, -1, 2 ** 31 - 1):
        assert call(depth=depth) == (bad, "depth must lie in 1 .. 255")
    assert call(min_dist=-1, coord=coord) == (bad, "min_dist must not be negative")
    assert call(min_dist=1) == (bad, "min_dist needs coord: without coordinates it must be 0")
    rc, msg = call(ncols=4097)
    assert rc == bad and "too many accessions" in msg and "SNPM_MK_MAX_ACCESSIONS" in msg
    rc, msg = call(n_rows=2 ** 31)
    assert rc == bad and "2^31 rows" in msg
    for k in range(3):
        assert call(outs=tuple(j != k for j in range(3))) == (bad, "n_chosen / remaining / stop_reason is NULL")
    assert call(need=None) == (bad, "need is NULL")
    assert call(chosen=None) == (bad, "chosen / gain_at is NULL") and call(gain_at=None) == (bad, "chosen / gain_at is NULL")
    # sound arguments: only the panel is missing -- the extremes of the parameters, no first_gain, no chosen where no pick is possible
    for kw in ({}, {"depth": 255}, {"first": None}, {"min_dist": 2 ** 62, "coord": coord}, {"min_dist": 0, "coord": coord}, {"ncols": 4096, "cols": None},
               {"max_markers": 0, "chosen": None, "gain_at": None}, {"n_rows": 0, "chosen": None, "gain_at": None}, {"ncols": 0, "need": None},
               {"max_markers": 2 ** 62}):
        assert call(**kw) == (bad, "panel is NULL"), kw
    assert "snpm_panel_marker_select" in _lib.SYMBOLS and engine.MK_MAX_ACCESSIONS == 4096


def test_header_constants_are_the_python_ones():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "snpmatch_hip.h")).read()
    assert int(re.search(r"#define SNPM_MK_MAX_ACCESSIONS (\d+)", text).group(1)) == engine.MK_MAX_ACCESSIONS
    kernels = open(os.path.join(root, "snpmatch_amd", "csrc", "snpm_k_mk.hpp")).read()
    assert int(re.search(r"constexpr int MK_MAX_WC = (\d+);", kernels).group(1)) * 64 == engine.MK_MAX_ACCESSIONS
    assert (twin.STOP_RESOLVED, twin.STOP_MAX_MARKERS, twin.STOP_NO_GAIN) == (0, 1, 2) and len(engine.MK_STOP_REASONS) == len(markers.STOP_REASONS) == 3


class _Holder(object):
    """stands in for a Genotype whose DB went to the given kind of panel"""

    def __init__(self, panel):
        self._panel = panel

    def panel(self):
        return self._panel


def test_group_and_streamed_panels_are_refused_with_the_reason():
    for cls, why in ((engine.GroupPanel, "spread over several GPUs"), (engine.StreamedPanel, "not a resident panel")):
        with pytest.raises(TypeError, match="marker_select needs every accession column on one device") as err:
            engine.marker_select(cls.__new__(cls))
        assert why in str(err.value)
    for cls, why in ((engine.GroupPanel, "spread over several GPUs by accession"), (engine.StreamedPanel, "streamed through the device")):
        with pytest.raises(TypeError, match="the marker selection needs every accession column of the DB on one device") as err:
            snp_genotype.Genotype.marker_select(_Holder(cls.__new__(cls)))
        assert why in str(err.value)


def test_coordinates_keep_chromosomes_apart():
    class G(object):
        pass
    g = _Holder(None)
    g.g = G()
    g.g.chr_regions = np.array([[0, 3], [3, 3], [3, 6]])                  # the second chromosome has no row
    g.g.positions = np.array([5, 70, 900, 1, 2, 950])
    rows = np.array([0, 2, 3, 5, 1])
    for min_dist in (0, 1, 100, 10 ** 6):
        coord = markers.coordinates(g, rows, min_dist)
        assert coord.dtype == np.int64 and coord.tolist() == [5, 900, 1 + 900 + 2 * min_dist, 950 + 900 + 2 * min_dist, 70]
        assert coord[2] - coord[1] >= min_dist                              # the first row of a chromosome against the last of the one before
    assert markers.coordinates(g, np.zeros(0, dtype=np.int64), 5).shape == (0,)


# ------------------------------------------------------------------------------------------------ the command
@pytest.fixture
def planted(monkeypatch, tmp_path):
    """the planted DB as an .npz; the device call is the twin"""
    case = twin.planted_case()
    snps = case["snps"]
    db = str(tmp_path / "db.npz")
    np.savez(db, snps=snps, accessions=case["names"], positions=case["positions"], chrs=case["chrs"], chr_regions=case["chr_regions"])
    calls = []
    stub = engine.Panel.__new__(engine.Panel)
    stub.h = None

    def device(panel, depth=1, max_markers=None, coord=None, min_dist=0, eligible=None, cols=None, rows=None, first_gain=True):
        calls.append({"depth": depth, "max_markers": max_markers, "coord": coord, "min_dist": min_dist, "eligible": eligible, "cols": cols, "rows": rows})
        return twin.marker_select(snps, depth, max_markers, coord, min_dist, eligible, cols, rows, first_gain)
    monkeypatch.setattr(snp_genotype.Genotype, "panel", lambda self, ctx=None, packed=None: stub)
    monkeypatch.setattr(engine, "marker_select", device)
    return case, db, calls


def _tsv(path):
    return [ln.split("\t") for ln in open(path).read().splitlines()]


def write_sites(case, path, leave_out):
    """every row of the planted DB but the listed ones, as a site list"""
    chr_of = np.repeat(case["chrs"], np.diff(case["chr_regions"], axis=1).reshape(-1))
    with open(path, "w") as out:
        out.write("chr\tpos\tmaf\n")
        for r in range(len(case["positions"])):
            if r not in leave_out:
                out.write("%s\t%d\t0.3\n" % (chr_of[r], case["positions"][r]))
    return chr_of


def separations_from_tsv(case, lines):
    """int [n_acc, n_acc]: by how many of the markers of a markers.tsv (looked up by chr and pos in the DB) each pair is separated"""
    chr_of = np.repeat(case["chrs"], np.diff(case["chr_regions"], axis=1).reshape(-1))
    where = {(str(c), int(p)): r for r, (c, p) in enumerate(zip(chr_of, case["positions"]))}
    rows = [where[(ln[1], int(ln[2]))] for ln in lines[1:]]
    h0, h1 = twin.planes(case["snps"], rows=np.array(rows, dtype=np.int64))
    s = h0.astype(np.int64).T @ h1.astype(np.int64)
    return rows, s + s.T


def check_planted_outputs(case, out, depth):
    """what both command tests (the twin here, the device in test_gpu_markers.py) ask of the three files"""
    names = case["names"].tolist()
    lines = _tsv(out + ".markers.tsv")
    assert lines[0] == ["order", "chr", "pos", "gain", "remaining"] and [ln[0] for ln in lines[1:]] == [str(k + 1) for k in range(len(lines) - 1)]
    rows, sep = separations_from_tsv(case, lines)
    assert not set(rows) & set(twin.PLANTED_HIDDEN_ROWS) and len(set(rows)) == len(rows)
    stats = json.load(open(out + ".markers.json"))
    # the unresolved pairs are exactly the identical pair and the pair that differs only at rows the site list leaves out
    want = sorted([twin.PLANTED_TWINS, twin.PLANTED_HIDDEN])
    assert [(u["acc_1"], u["acc_2"], u["need"]) for u in stats["unresolved"]] == [(names[a], names[b], depth) for a, b in want]
    assert stats["unresolved_pairs"] == 2 and stats["stop_reason"] == 2 and stats["remaining"] == 2 * depth and stats["stop_reason_text"] == "no candidate with gain"
    assert (stats["accessions"], stats["pairs"], stats["depth"], stats["candidates"], stats["markers"]) == (40, 780, depth, 597, len(rows))
    # every other pair is separated depth times by the listed markers: from the tsv alone
    other = np.triu(np.ones((40, 40), dtype=bool), 1)
    for a, b in want:
        other[a, b] = False
        assert sep[a, b] == 0
    assert (sep[other] >= depth).all()
    # gain and remaining of the tsv are consistent: remaining falls by the gain, from depth * pairs to the json's figure
    gain, left = np.array([int(ln[3]) for ln in lines[1:]]), np.array([int(ln[4]) for ln in lines[1:]])
    assert np.array_equal(left, depth * 780 - np.cumsum(gain)) and left[-1] == stats["remaining"] and (gain > 0).all()
    z = np.load(out + ".markers.npz")
    assert z["rows"][z["chosen"]].tolist() == rows and np.array_equal(z["gain_at"], gain) and z["need"].dtype == np.uint8 and z["need"].shape == (40, 40)
    assert z["pos"][z["chosen"]].tolist() == [int(ln[2]) for ln in lines[1:]] and z["chr"][z["chosen"]].tolist() == [ln[1] for ln in lines[1:]]
    assert np.argwhere(np.triu(z["need"])).tolist() == [list(p) for p in want] and z["accessions"].tolist() == names
    h0, h1 = twin.planes(case["snps"], rows=z["rows"])
    assert np.array_equal(z["first_gain"], twin.gains(h0, h1, ~np.eye(40, dtype=bool)).astype(np.int32)) and len(z["rows"]) == 597
    return stats, z


def test_command_separates_every_pair_but_the_planted_two(planted, tmp_path):
    case, db, calls = planted
    snps = case["snps"]
    assert snps.shape == (600, 40) and twin.PLANTED_SEED == 41
    a, b = twin.PLANTED_HIDDEN
    differ = np.flatnonzero(snps[:, a] != snps[:, b])
    assert differ.tolist() == list(twin.PLANTED_HIDDEN_ROWS) and np.array_equal(snps[:, twin.PLANTED_TWINS[0]], snps[:, twin.PLANTED_TWINS[1]])
    sites = str(tmp_path / "x.sites.tsv")
    write_sites(case, sites, set(twin.PLANTED_HIDDEN_ROWS))
    out = str(tmp_path / "out")
    assert cli.main(["markers", "-d", db, "--sites", sites, "--depth", "2", "-o", out]) == 0
    keep = np.array([r for r in range(600) if r not in twin.PLANTED_HIDDEN_ROWS])
    assert len(calls) == 1 and calls[0]["depth"] == 2 and calls[0]["max_markers"] is None and calls[0]["coord"] is None and calls[0]["min_dist"] == 0
    assert calls[0]["cols"] is None and calls[0]["eligible"] is None and np.array_equal(calls[0]["rows"], keep)
    stats, z = check_planted_outputs(case, out, 2)
    want = twin.marker_select(snps, 2, rows=keep)
    assert np.array_equal(z["chosen"], want["chosen"]) and np.array_equal(z["need"], want["need"]) and stats["markers"] == want["n_chosen"]
    # with every row a candidate the hidden pair is resolved too: only the identical pair is left; the rows are a dense range
    assert cli.main(["markers", "-d", db, "-o", out]) == 0 and calls[-1]["rows"] == range(0, 600)
    stats = json.load(open(out + ".markers.json"))
    assert [(u["acc_1"], u["acc_2"]) for u in stats["unresolved"]] == [("acc07", "acc29")] and stats["candidates"] == 600 and stats["max_markers"] is None
    # the markers.tsv is a site list: as candidates it gives the same set back, in the same order
    first = _tsv(out + ".markers.tsv")
    assert cli.main(["markers", "-d", db, "--sites", out + ".markers.tsv", "-o", out + "2"]) == 0
    again = _tsv(out + "2.markers.tsv")
    assert sorted(ln[1:3] for ln in again[1:]) == sorted(ln[1:3] for ln in first[1:]) and json.load(open(out + "2.markers.json"))["remaining"] == 1
    # --max_markers: stop reason 1; --bed: the rows of a region
    assert cli.main(["markers", "-d", db, "--max_markers", "3", "--bed", "Chr2,1,100000", "-o", out]) == 0
    stats = json.load(open(out + ".markers.json"))
    assert calls[-1]["max_markers"] == 3 and calls[-1]["rows"] == range(350, 450) and (stats["markers"], stats["stop_reason"], stats["candidates"]) == (3, 1, 100)
    assert all(ln[1] == "Chr2" for ln in _tsv(out + ".markers.tsv")[1:])
    # --min_dist_bp: coordinates travel, the chromosomes are kept apart, chosen markers of a chromosome are that far apart
    assert cli.main(["markers", "-d", db, "--min_dist_bp", "5000", "-o", out]) == 0
    coord = calls[-1]["coord"]
    assert calls[-1]["min_dist"] == 5000 and coord.dtype == np.int64 and coord[:350].tolist() == case["positions"][:350].tolist()
    assert coord[350] - coord[349] >= 5000 and (np.diff(coord) > 0).all()
    picked = _tsv(out + ".markers.tsv")[1:]
    for name in ("Chr1", "Chr2"):
        pos = np.sort([int(ln[2]) for ln in picked if ln[1] == name])
        assert len(pos) > 1 and (np.diff(pos) >= 5000).all()
    # an accession list in another order: the pairs are named by the list's order
    acc_file = tmp_path / "accs.txt"
    acc_file.write_text("acc29\nacc03\nacc07\n")
    assert cli.main(["markers", "-d", db, "-a", str(acc_file), "-o", out]) == 0 and calls[-1]["cols"].tolist() == [29, 3, 7]
    stats = json.load(open(out + ".markers.json"))
    assert stats["unresolved"] == [{"acc_1": "acc29", "acc_2": "acc07", "need": 1}] and (stats["accessions"], stats["pairs"]) == (3, 3)
    # bad arguments: exit code 2, the device is not asked
    asked = len(calls)
    for bad in (["--depth", "0"], ["--depth", "256"], ["--min_dist_bp", "-1"], ["--max_markers", "0"], ["--bed", "Chr1,1,1000", "--sites", sites]):
        assert cli.main(["markers", "-d", db, "-o", out] + bad) == 2
    acc_file.write_text("acc29\nacc29\n")
    assert cli.main(["markers", "-d", db, "-a", str(acc_file), "-o", out]) == 2
    assert cli.main(["power", "-d", db, "-n", "10", "--bed", "Chr1,1,1000", "--sites", sites, "-o", out]) == 2      # power reads a site list too, not both
    assert len(calls) == asked and markers.potatoMarkers.__doc__


# ------------------------------------------------------------------------------------------------ the kernels, on the host
def test_kernel_source_on_the_host_under_asan_and_ubsan(tmp_path):
    """every block of k_mk_rowplanes / k_mk_gain / k_mk_pick / k_mk_update run by 256 real threads with a barrier, the round loop
    enqueued in the library's batches, exact-size heap buffers, arbitrary pad bytes, stale workspaces: 1 / 2 / 63 / 64 / 65 / 130
    accessions x 1 / 7 / 8 / 9 / 63 / 64 / 65 rows (8: the row group of a gain block) over the three layouts and the four depths;
    row and column lists with repeats; eligibility masks, one that forbids the best row, one that forbids all; max_markers 1, a
    whole batch of rounds and one more; min_dist larger than the coordinate range, 1 with every coordinate twice, 5, 0; duplicated
    rows at depth 1 and 2; depth 255; all-missing, all-het and one-allele panels; the split layout at 1135 accessions"""
    cases = host_kernel_util.run_driver("mk_host_driver", tmp_path)
    assert len(cases) == 64
    field = lambda ln, k: next(f.split("=")[1] for f in ln.split() if f.startswith(k + "="))      # noqa: E731
    group = int(re.search(r"constexpr int MK_GAIN_ROWS = (\d+);", open(os.path.join(host_kernel_util.ROOT, "snpmatch_amd", "csrc", "snpm_k_mk.hpp")).read()).group(1))
    grid = [ln for ln in cases if ln.split()[1] == "grid"]
    assert {(int(field(ln, "acc")), int(field(ln, "rows"))) for ln in grid} == {(a, r) for a in (1, 2, 63, 64, 65, 130) for r in (1, group - 1, group, group + 1, 63, 64, 65)}
    assert {field(ln, "layout") for ln in grid} == {"0", "1", "2"} and {field(ln, "depth") for ln in grid} == {"1", "2", "3", "255"}
    assert {field(ln, "layout") for ln in cases if ln.split()[1] == "lists"} == {"0", "1", "2"}
    assert {field(ln, "reason") for ln in cases} == {"0", "1", "2"}
    by_name = {ln.split()[1]: ln for ln in cases}
    assert field(by_name["max-1"], "picks") == "1" and field(by_name["max-batch"], "batches") == "1" and field(by_name["max-batch-plus-1"], "batches") == "2"
    assert field(by_name["dist-all"], "picks") == "1" and field(by_name["nothing-eligible"], "picks") == "0"
    assert all(field(by_name[k], "picks") == "0" and field(by_name[k], "reason") == "2" for k in ("all-missing", "all-het", "one-allele"))
    assert int(field(by_name["duplicated-depth-2"], "picks")) > int(field(by_name["duplicated-depth-1"], "picks"))
    assert field(by_name["depth-255-more-allowed"], "reason") == "2" and field(by_name["split-wide"], "acc") == "1135"
    assert field(by_name["resolved-in-batch-2"], "batches") == "2" and field(by_name["resolved-in-batch-2"], "reason") == "0"      # an end found by the second read of the state
