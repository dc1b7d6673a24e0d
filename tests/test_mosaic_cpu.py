"""mosaic without a GPU: the numpy twin (tests/mosaic_twin.py) against a brute-force full-transition DP over seeded random cases
(the brute cost is the twin's cost and the cost of the twin's path on EVERY case); a planted sample copied from four accessions of
a 40-accession panel that holds a near-duplicate of one source, whose plan the twin recovers to within PLANTED_TOL sites of every
breakpoint; every refusal of ``snpm_panel_mosaic`` that needs no device; the ``mosaic`` subcommand, its arguments and its three
files with the twin in the place of the device; the segment writer on a hand-made state."""
import json

import numpy as np
import pytest

import mosaic_twin as twin
from snpmatch_amd import _lib, cli, engine
from snpmatch_amd.core import mosaic, snp_genotype

NONE = 0xFF


# ------------------------------------------------------------------------------------------------ twin against brute force
def _random_case(rng, n_rows, ncols, S, zero_table=False, blank_cols=False, no_classes=False, dup=False):
    snps = rng.choice(np.array([-1, 0, 1, 2, 3], dtype=np.int8), size=(n_rows, ncols), p=[.1, .4, .35, .1, .05])
    if blank_cols:
        snps[:, rng.integers(0, ncols)] = -1
        if ncols > 2:
            snps[:, :] = np.where(rng.random(ncols) < 0.5, -1, snps)
    cols = None
    if dup:
        cols = rng.integers(0, ncols, size=ncols + 2)
        cols[-1] = cols[0]
    src = rng.integers(0, ncols)
    cls = np.zeros(n_rows, dtype=np.uint8)
    for k in range(n_rows):
        if rng.random() < 0.08:
            src = rng.integers(0, ncols)
        v = snps[k, src]
        cls[k] = v if 0 <= v <= 2 and rng.random() > 0.1 else rng.integers(0, 3)
    cls[rng.random(n_rows) < 0.05] = NONE
    if no_classes:
        cls[:] = NONE
    cost = np.zeros((3, 4), dtype=np.uint8) if zero_table else rng.integers(0, 16, size=(3, 4)).astype(np.uint8)
    cuts = np.sort(rng.integers(0, n_rows + 1, size=rng.integers(0, 4)))
    chain_off = np.concatenate([[0], cuts, [n_rows]]).astype(np.int64)
    return snps, cols, cls, cost, chain_off, S


def _check(case):
    snps, cols, cls, cost, chain_off, S = case
    state, chain_cost, col_cost = twin.mosaic(snps, cls, chain_off, cost, S, cols)
    e = twin.emissions(twin.select(snps, cols), cls, cost)
    want = twin.brute(e, chain_off, S)
    assert np.array_equal(chain_cost[0], want), (chain_cost[0], want)
    assert np.array_equal(twin.path_cost(e, chain_off, S, state[0]), want)
    assert state.dtype == np.int32 and state.min() >= 0 and state.max() < e.shape[1]
    for c in range(len(chain_off) - 1):
        assert np.array_equal(col_cost[0, c], e[chain_off[c]:chain_off[c + 1]].sum(axis=0))
    return state, chain_cost, col_cost


def test_twin_is_the_full_transition_dp_on_random_cases():
    rng = np.random.default_rng(2026)
    n = 0
    for S in (1, 2, 3, 7, 40, 1 << 20):
        for _ in range(20):
            _check(_random_case(rng, int(rng.integers(1, 90)), int(rng.integers(1, 9)), S, dup=bool(rng.integers(0, 2))))
            n += 1
    for S in (1, 7, 1 << 20):
        for kind in ("zero_table", "blank_cols", "no_classes", "dup"):
            for _ in range(5):
                _check(_random_case(rng, int(rng.integers(1, 90)), int(rng.integers(1, 9)), S, **{kind: True}))
                n += 1
    assert n == 180


def test_twin_edges_written_out():
    # a zero table and a sample without classes: every path is free, the lowest column wins every tie, nothing switches
    rng = np.random.default_rng(3)
    for kind in ("zero_table", "no_classes"):
        state, chain_cost, col_cost = _check(_random_case(rng, 70, 5, 1, **{kind: True}))
        assert not state.any() and not chain_cost.any() and not col_cost.any()
    # S at its maximum on short chains: the path never switches, the chain cost is the best column's
    for _ in range(10):
        case = _random_case(rng, 80, 6, 1 << 20)
        state, chain_cost, col_cost = _check(case)
        off = case[4]
        for c in range(len(off) - 1):
            if off[c + 1] > off[c]:
                assert chain_cost[0, c] == col_cost[0, c].min() and len(set(state[0, off[c]:off[c + 1]].tolist())) == 1
                assert state[0, off[c]] == int(np.argmin(col_cost[0, c]))
    # two equal columns: the tie goes to the lower position, whichever column it names
    snps = np.array([[0, 0], [1, 1], [0, 0]], dtype=np.int8)
    state, _, _ = twin.mosaic(snps, np.array([0, 1, 0], dtype=np.uint8), [0, 3], mosaic.cost_table(), 1, cols=[1, 1, 0])
    assert state.tolist() == [[0, 0, 0]]
    # a hand-made switch: column 0 fits the first three rows, column 1 the last three; S = 1 switches where the costs tie (strict >)
    snps = np.array([[0, 1], [0, 1], [0, 1], [1, 0], [1, 0], [1, 0]], dtype=np.int8)
    state, chain_cost, col_cost = twin.mosaic(snps, np.zeros(6, dtype=np.uint8), [0, 6], mosaic.cost_table(2, 1), 1)
    assert state.tolist() == [[0, 0, 0, 1, 1, 1]] and chain_cost.tolist() == [[1]] and col_cost.tolist() == [[[6, 6]]]
    # the int8 "other" code is not missing: it costs column 3 of the table; a packed panel reads it as missing
    cost = np.array([[0, 2, 1, 7], [2, 0, 1, 7], [1, 1, 0, 7]], dtype=np.uint8)
    snps = np.array([[3], [3], [-1]], dtype=np.int8)
    assert twin.mosaic(snps, np.array([0, 2, 1], dtype=np.uint8), [0, 3], cost, 5)[1].tolist() == [[14]]
    assert twin.mosaic(snps, np.array([0, 2, 1], dtype=np.uint8), [0, 3], cost, 5, packed=True)[1].tolist() == [[0]]


# ------------------------------------------------------------------------------------------------ the planted case
def test_twin_recovers_the_planted_plan():
    p = twin.planted()
    cost = mosaic.cost_table(twin.PLANTED_MISMATCH, twin.PLANTED_HET)
    state, chain_cost, col_cost = twin.mosaic(p["snps"], p["classes"], p["chain_off"], cost, twin.PLANTED_S, rows=p["rows"])
    segs = mosaic.segments_of(state[0], p["chain_off"])
    assert twin.plan_recovered(segs), segs.tolist()
    assert twin.PLANTED_NEAR not in segs[:, 3] and set(segs[:, 3].tolist()) == set(twin.PLANTED_SOURCES)
    # the mosaic explains the sample far better than any single accession
    assert chain_cost[0].sum() * 4 < col_cost[0].sum(axis=0).min()
    e = twin.emissions(twin.select(p["snps"], rows=p["rows"]), p["classes"], cost)
    assert np.array_equal(twin.brute(e, p["chain_off"], twin.PLANTED_S), chain_cost[0])


# ------------------------------------------------------------------------------------------------ the library's validation
def test_refusals_that_need_no_device():
    lib = _lib.load()
    cols = np.zeros(2, dtype=np.int32)
    good = np.array([[0, 1, 2, NONE, 0], [NONE, NONE, 1, 1, 2]], dtype=np.uint8)
    off5 = np.array([0, 2, 2, 5], dtype=np.int64)
    table = np.array([[0, 2, 1, 2], [2, 0, 1, 2], [1, 1, 0, 15]], dtype=np.uint8)
    state, ccost, colc = np.zeros((2, 5), dtype=np.int32), np.zeros((2, 3), dtype=np.int32), np.zeros((2, 3, 2), dtype=np.int32)

    def call(ncols, n_rows, cols=cols, off=off5, n_chain=3, cls=good, n_samples=2, cost=table, S=40, outs=(state, ccost, colc)):
        rc = lib.snpm_panel_mosaic(None, _lib.ptr(cols), ncols, None, 0, n_rows, _lib.ptr(off), n_chain, _lib.ptr(cls), n_samples, _lib.ptr(cost), S,
                                   *[_lib.ptr(o) for o in outs])
        return rc, lib.snpm_last_error(None).decode()
    bad = _lib.SNPM_ERR_BADARG
    assert call(-1, 5) == (bad, "negative size") and call(2, -1) == (bad, "negative size")
    assert call(2, 5, n_chain=-1) == (bad, "negative size") and call(2, 5, n_samples=-1) == (bad, "negative size")
    rc, msg = call(engine.MOS_MAX_ACCESSIONS + 1, 5)
    assert rc == bad and "too many accessions" in msg and "SNPM_MOS_MAX_ACCESSIONS" in msg and engine.MOS_MAX_ACCESSIONS >= 11552
    rc, msg = call(2, 2 ** 31)
    assert rc == bad and "2^31 rows" in msg
    rc, msg = call(2, 5, n_chain=(1 << 20) + 1)
    assert rc == bad and "too many chains" in msg
    assert call(2, 5, off=None) == (bad, "chain_off is NULL")
    assert call(2, 5, off=np.array([1, 2, 2, 5], dtype=np.int64)) == (bad, "chain_off must start at 0")
    assert call(2, 5, off=np.array([0, 3, 2, 5], dtype=np.int64)) == (bad, "chain_off must not decrease")
    assert call(2, 5, off=np.array([0, 2, 2, 4], dtype=np.int64)) == (bad, "chain_off must end at n")
    assert call(2, 5, n_chain=0) == (bad, "chain_off must end at n")              # no chain, but rows
    assert call(2, 5, n_samples=0) == (bad, "n_samples must be at least 1")
    assert call(2, 5, cost=None) == (bad, "cost is NULL")
    for at in (0, 5, 11):
        t = table.copy()
        t.reshape(-1)[at] = 16
        assert call(2, 5, cost=t) == (bad, "cost holds an entry above 15")
    for S in (0, -1, (1 << 20) + 1, -2 ** 31):
        assert call(2, 5, S=S) == (bad, "switch_cost must be 1 .. 2^20")
    long_off = np.array([0, (2 ** 31 - 1) // 15 + 1], dtype=np.int64)            # 15 * chain + 1 just reaches 2^31
    assert call(2, int(long_off[1]), off=long_off, n_chain=1, S=1)[1] == "15 * (longest chain) + switch_cost must stay below 2^31"
    assert call(2, 5, cls=None) == (bad, "sample_class is NULL")
    for byte in (3, 4, 0x7F, 0xFE):
        cls = good.copy()
        cls[1, 3] = byte
        assert call(2, 5, cls=cls) == (bad, "sample_class holds a byte other than 0, 1, 2 or 0xFF")
    assert call(2, 5, outs=(None, ccost, colc)) == (bad, "state is NULL")
    assert call(2, 5, outs=(state, None, colc)) == (bad, "chain_cost is NULL")
    assert call(2, 5) == (bad, "panel is NULL")                                   # sound arguments: only the panel is missing
    assert call(2, 5, outs=(state, ccost, None)) == (bad, "panel is NULL")        # col_cost is optional
    assert call(2, 5, S=1) == (bad, "panel is NULL") and call(2, 5, S=1 << 20) == (bad, "panel is NULL")
    assert call(0, 5, outs=(None, None, None)) == (bad, "panel is NULL")
    assert call(2, 0, cls=None, off=np.zeros(1, dtype=np.int64), n_chain=0, outs=(None, None, None)) == (bad, "panel is NULL")
    assert call(2, 0, cls=None, off=np.zeros(3, dtype=np.int64), n_chain=2, n_samples=0, outs=(None, None, None)) == (bad, "panel is NULL")
    assert call(engine.MOS_MAX_ACCESSIONS, 5, cols=None) == (bad, "panel is NULL")      # the limit is inclusive
    assert "snpm_panel_mosaic" in _lib.SYMBOLS


class _Holder(object):
    """stands in for a Genotype whose DB went to the given kind of panel"""

    def __init__(self, panel):
        self._panel = panel

    def panel(self):
        return self._panel


def test_group_and_streamed_panels_are_refused_with_the_reason():
    cls8, off = np.zeros((1, 3), dtype=np.uint8), np.array([0, 3])
    for cls, why in ((engine.GroupPanel, "spread over several GPUs"), (engine.StreamedPanel, "not a resident panel")):
        with pytest.raises(TypeError, match="mosaic needs every accession column on one device") as err:
            engine.mosaic(cls.__new__(cls), cls8, off, mosaic.cost_table(), 40)
        assert why in str(err.value)
        with pytest.raises(TypeError, match="the mosaic needs every accession column of the DB on one device"):
            snp_genotype.Genotype.mosaic(_Holder(cls.__new__(cls)), cls8, off, mosaic.cost_table(), 40)


# ------------------------------------------------------------------------------------------------ the command
def test_cost_table_of_the_flags():
    assert mosaic.cost_table().tolist() == [[0, 2, 1, 2], [2, 0, 1, 2], [1, 1, 0, 2]]
    assert mosaic.cost_table(15, 0).tolist() == [[0, 15, 0, 15], [15, 0, 0, 15], [0, 0, 0, 15]]
    for m, h in ((16, 1), (-1, 1), (2, 16), (2, -1)):
        with pytest.raises(ValueError):
            mosaic.cost_table(m, h)
    for S in (0, (1 << 20) + 1):
        with pytest.raises(ValueError):
            mosaic.check_switch_cost(S)


def test_cli_arguments():
    args = cli.get_options("d", "v").parse_args(["mosaic", "-i", "s.vcf.gz", "-d", "db.snpm", "-o", "out"])
    got = vars(args)
    assert (got["switch_cost"], got["mismatch"], got["het_cost"], got["min_seg_sites"]) == (40, 2, 1, 20)
    assert got["accFile"] is None and got["hdf5accFile"] is None and got["func"] is cli.snpmatch_mosaic
    got = vars(cli.get_options("d", "v").parse_args(["mosaic", "-i", "s.bed", "-d", "db.snpm", "-e", "acc.hdf5", "-a", "founders.txt", "--switch_cost", "7",
                                                     "--mismatch", "3", "--het_cost", "0", "--min_seg_sites", "5", "-o", "o"]))
    assert (got["switch_cost"], got["mismatch"], got["het_cost"], got["min_seg_sites"], got["accFile"], got["hdf5accFile"]) == (7, 3, 0, 5, "founders.txt", "acc.hdf5")
    for missing in (["-d", "db", "-o", "o"], ["-i", "s", "-o", "o"], ["-i", "s", "-d", "db"]):
        with pytest.raises(SystemExit):
            cli.get_options("d", "v").parse_args(["mosaic"] + missing)


def test_segments_of_a_hand_made_state_and_their_table(tmp_path):
    state = np.array([3, 3, 1, 1, 1, 0, 0, 0, 2, 0], dtype=np.int32)
    chain_off = np.array([0, 0, 5, 5, 8, 10, 10])                  # empty chains first, in the middle, last; a switch at a chain boundary is none
    segs = mosaic.segments_of(state, chain_off)
    assert segs.tolist() == [[1, 0, 1, 3], [1, 2, 4, 1], [3, 5, 7, 0], [4, 8, 8, 2], [4, 9, 9, 0]]
    assert mosaic.segments_of(np.zeros(0, dtype=np.int32), [0, 0]).shape == (0, 4)
    assert mosaic.segments_of(np.array([4]), [0, 1]).tolist() == [[0, 0, 0, 4]]
    path = str(tmp_path / "seg.tsv")
    mosaic.write_segments(path, ["s1"], [segs], [[0, 4, 1, 0, 2]], ["c0", "c1", "c2", "c3", "c4", "c5"], np.arange(10) * 10 + 5,
                          ["A", "B", "C", "D"], min_seg_sites=2)
    lines = [ln.split("\t") for ln in open(path).read().splitlines()]
    assert lines[0] == ["sample", "chr", "first_pos", "last_pos", "accession", "sites", "cost", "short"]
    assert lines[1:] == [["s1", "c1", "5", "15", "D", "2", "0", "0"], ["s1", "c1", "25", "45", "B", "3", "4", "0"], ["s1", "c3", "55", "75", "A", "3", "1", "0"],
                         ["s1", "c4", "85", "85", "C", "1", "0", "1"], ["s1", "c4", "95", "95", "A", "1", "2", "1"]]
    assert mosaic.chains_of([0, 3, 4, 9], [[0, 4], [4, 4], [4, 10]]).tolist() == [0, 2, 2, 4]


@pytest.fixture
def planted_command(tmp_path, monkeypatch):
    p = twin.planted()
    db = str(tmp_path / "db.npz")
    np.savez(db, snps=p["snps"], accessions=p["accessions"], positions=p["positions"], chrs=p["chrs"], chr_regions=p["chr_regions"])
    bed = str(tmp_path / "sample.bed")
    with open(bed, "w") as fh:
        for c, pos, t in zip(p["s_chr"], p["s_pos"], p["s_gt"]):
            fh.write("%s\t%d\t%s\n" % (c, pos, t))
    calls = []
    stub = engine.Panel.__new__(engine.Panel)
    stub.h = None

    def device(panel, classes, chain_off, cost, switch_cost, cols=None, rows=None, want_col_cost=False):
        calls.append((cols, rows, np.asarray(chain_off).copy(), np.asarray(cost).copy(), switch_cost))
        rows = np.arange(rows.start, rows.stop) if isinstance(rows, range) else rows
        out = twin.mosaic(p["snps"], classes, chain_off, cost, switch_cost, cols, rows)
        return out if want_col_cost else out[:2] + (None,)
    monkeypatch.setattr(snp_genotype.Genotype, "panel", lambda self, ctx=None, packed=None: stub)
    monkeypatch.setattr(engine, "mosaic", device)
    return p, db, bed, calls


def test_command_recovers_the_planted_plan(planted_command, tmp_path):
    p, db, bed, calls = planted_command
    out = str(tmp_path / "out")
    assert cli.main(["mosaic", "-i", bed, "-d", db, "-o", out]) == 0
    assert calls[0][0] is None and np.array_equal(calls[0][1], p["rows"]) and np.array_equal(calls[0][2], p["chain_off"])
    assert calls[0][3].tolist() == mosaic.cost_table().tolist() and calls[0][4] == 40 and len(calls) == 2
    z = np.load(out + ".mosaic.npz")
    want = twin.mosaic(p["snps"], p["classes"], p["chain_off"], mosaic.cost_table(), 40, rows=p["rows"])
    assert np.array_equal(z["state"], want[0]) and np.array_equal(z["chain_cost"], want[1]) and np.array_equal(z["rows"], p["rows"])
    assert z["columns"].tolist() == list(range(40)) and z["samples"].tolist() == ["sample.bed"] and np.array_equal(z["chain_off"], p["chain_off"])
    lines = [ln.split("\t") for ln in open(out + ".mosaic.segments.tsv").read().splitlines()]
    segs = mosaic.segments_of(want[0][0], p["chain_off"])
    assert twin.plan_recovered(segs) and len(lines) == 1 + len(segs)
    e = twin.emissions(twin.select(p["snps"], rows=p["rows"]), p["classes"], mosaic.cost_table())
    for ln, (c, k0, k1, a) in zip(lines[1:], segs.tolist()):
        assert ln == ["sample.bed", str(c + 1), str(p["s_pos"][k0]), str(p["s_pos"][k1]), "acc%02d" % a, str(k1 - k0 + 1), str(e[k0:k1 + 1, a].sum()), "0"]
    stats = json.load(open(out + ".mosaic.json"))
    s = stats["samples"]["sample.bed"]
    assert stats["matched_rows"] == 2700 and stats["chains"] == 2 and stats["candidates"] == 40
    assert stats["parameters"] == {"switch_cost": 40, "mismatch": 2, "het_cost": 1, "min_seg_sites": 20, "cost": mosaic.cost_table().tolist()}
    assert s["switches"] == 4 and s["segments"] == 6 and s["short_segments"] == 0 and s["total_cost"] == int(want[1].sum())
    assert s["total_cost"] == sum(int(ln[6]) for ln in lines[1:]) + 40 * s["switches"]
    assert [a["accession"] for a in s["accessions"]] == ["acc17", "acc05", "acc31", "acc23"] and sum(a["sites"] for a in s["accessions"]) == 2700
    single = want[2][0].sum(axis=0)
    assert s["best_single"] == {"accession": "acc%02d" % int(np.argmin(single)), "cost": int(single.min())} and s["best_single"]["cost"] > 4 * s["total_cost"]
    # a founder list in another order: states are positions in the list, names follow it
    acc_file = tmp_path / "founders.txt"
    acc_file.write_text("acc31\nacc38\nacc05\nacc23\n")
    assert cli.main(["mosaic", "-i", bed, "-d", db, "-a", str(acc_file), "--switch_cost", "30", "--min_seg_sites", "460", "-o", out]) == 0
    z = np.load(out + ".mosaic.npz")
    assert z["columns"].tolist() == [31, 38, 5, 23] and z["accessions"].tolist() == ["acc31", "acc38", "acc05", "acc23"]
    lines = [ln.split("\t") for ln in open(out + ".mosaic.segments.tsv").read().splitlines()]
    assert [ln[4] for ln in lines[1:]] == ["acc05", "acc38", "acc31", "acc23", "acc38", "acc05"]         # the near-duplicate stands in for acc17
    assert [ln[7] for ln in lines[1:]] == ["1", "0", "1", "1", "0", "1"]
    assert cli.main(["mosaic", "-i", bed, "-d", db, "--switch_cost", "0", "-o", out]) == 2
    assert cli.main(["mosaic", "-i", bed, "-d", db, "--mismatch", "16", "-o", out]) == 2


def test_multi_sample_vcf_is_a_batch_on_its_shared_records(planted_command, tmp_path):
    """two sample columns: the planted sample, and the same without a call at every third record (class 0xFF there)"""
    p, db, _, calls = planted_command
    vcf = str(tmp_path / "two.vcf")
    with open(vcf, "w") as fh:
        fh.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tplanted\tthinned\n")
        for k, (c, pos, t) in enumerate(zip(p["s_chr"], p["s_pos"], p["s_gt"])):
            fh.write("%s\t%d\t.\tA\tT\t.\tPASS\t.\tGT\t%s\t%s\n" % (c, pos, t, "./." if k % 3 == 0 else t))
    out = str(tmp_path / "out")
    assert cli.main(["mosaic", "-i", vcf, "-d", db, "-o", out]) == 0
    classes = np.stack([p["classes"], np.where(np.arange(2700) % 3 == 0, NONE, p["classes"]).astype(np.uint8)])
    want = twin.mosaic(p["snps"], classes, p["chain_off"], mosaic.cost_table(), 40, rows=p["rows"])
    z = np.load(out + ".mosaic.npz")
    assert z["samples"].tolist() == ["planted", "thinned"] and np.array_equal(z["state"], want[0]) and np.array_equal(z["chain_cost"], want[1])
    assert len(calls) == 3                                      # one call for the batch, one per sample for the costs inside its segments
    stats = json.load(open(out + ".mosaic.json"))["samples"]
    assert stats["planted"]["classed_rows"] == 2700 and stats["thinned"]["classed_rows"] == 1800 and stats["thinned"]["switches"] == 4
    names = {ln.split("\t")[0] for ln in open(out + ".mosaic.segments.tsv").read().splitlines()[1:]}
    assert names == {"planted", "thinned"}
