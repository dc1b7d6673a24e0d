"""pairsnp on the device: ``snpm_pair_counts`` / ``k_pair_transpose`` + ``k_pair_count`` against the reference's goldens and the
numpy twin (tests/pairsnp_twin.py), whole files through ``pairwiseScore`` / ``PairCohort`` and the command line, and random ids at
the shapes where the decomposition could break: T = 32 samples per tile side (a 2 x 2 register tile of pairs per lane, the
transpose works on 64 samples), C = 4096 records per chunk (every segment padded to whole chunks, 256 records per LDS step)."""
import json

import numpy as np
import pytest

import pairsnp_twin
import pairsnp_util
from snpmatch_amd import cli, engine
from snpmatch_amd.core import pairsnp

pytestmark = pytest.mark.gpu

T = 32          # PR_TILE of csrc/snpm_k_pairs.hpp
C = 4096        # PR_CHUNK
SEGMENTS = [0, 1, 3, 4, 5, C - 1, 0, C, C + 1, 3 * C + 2]          # every length of interest, an empty segment between two others


@pytest.fixture(scope="module")
def ctx():
    return engine.default_context()


def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def _check(ctx, ids, seg_off):
    """device == twin, both matrices symmetric, both diagonals = calls per segment"""
    common, match = engine.pair_counts(ctx, ids, seg_off)
    t_common, t_match = pairsnp_twin.pair_counts(np.ascontiguousarray(ids), seg_off)
    assert common.dtype == np.int32 and match.dtype == np.int32
    assert np.array_equal(common, t_common)
    assert np.array_equal(match, t_match)
    assert np.array_equal(common, common.transpose(0, 2, 1)) and np.array_equal(match, match.transpose(0, 2, 1))
    calls = np.add.reduceat(np.concatenate([np.asarray(ids) != 0, np.zeros((1, ids.shape[1]), dtype=bool)]).astype(np.int64),
                            np.asarray(seg_off[:-1]), axis=0)
    calls[np.diff(seg_off) == 0] = 0                     # (reduceat gives a row, not zero, for an empty range)
    diag = np.arange(ids.shape[1])
    assert np.array_equal(common[:, diag, diag], calls) and np.array_equal(match[:, diag, diag], calls)
    return common, match


def _random_ids(rng, n, ns, top=5, absent=0.2):
    ids = rng.integers(1, top + 1, size=(n, ns), dtype=np.uint8)
    ids[rng.random((n, ns)) < absent] = 0
    return ids


@pytest.mark.parametrize("ns", [1, 2, T - 1, T, T + 1])
def test_every_segment_length_at_small_sample_counts(ns, ctx):
    rng = np.random.default_rng(100 + ns)
    seg_off = _offsets(SEGMENTS)
    _check(ctx, _random_ids(rng, int(seg_off[-1]), ns), seg_off)


@pytest.mark.parametrize("ns", [2 * T + 1, 257])
def test_several_tiles_of_samples(ns, ctx):
    rng = np.random.default_rng(200 + ns)
    seg_off = _offsets([3, 0, C + 1])
    _check(ctx, _random_ids(rng, int(seg_off[-1]), ns, top=2), seg_off)


def test_all_segments_empty(ctx):
    common, match = engine.pair_counts(ctx, np.zeros((0, 5), dtype=np.uint8), [0, 0, 0])
    assert common.shape == (3 - 1, 5, 5) and not common.any() and not match.any()


def test_one_pair_over_many_records_is_split_over_the_grid(ctx):
    rng = np.random.default_rng(3)
    n = 300001                                            # 74 chunks of one segment
    ids = _random_ids(rng, n, 2, top=127, absent=0.03)
    same = rng.random(n) < 0.9
    ids[same, 1] = np.where(ids[same, 1] != 0, ids[same, 0], 0)
    common, match = _check(ctx, ids, [0, n])
    assert 0 < match[0, 0, 1] < common[0, 0, 1] < n


def test_uniform_and_extreme_ids(ctx):
    seg_off = _offsets([5, C + 3])
    n = int(seg_off[-1])
    common, match = _check(ctx, np.zeros((n, T + 1), dtype=np.uint8), seg_off)
    assert not common.any() and not match.any()
    common, match = _check(ctx, np.full((n, T + 1), 77, dtype=np.uint8), seg_off)
    assert np.all(common == np.diff(seg_off)[:, None, None]) and np.array_equal(common, match)
    rng = np.random.default_rng(4)
    ids = np.where(rng.random((n, 5)) < 0.5, 1, 127).astype(np.uint8)          # 1 ^ 127 = 126: every bit but the lowest differs
    common, match = _check(ctx, ids, seg_off)
    assert np.all(common == np.diff(seg_off)[:, None, None]) and match[1, 0, 1] < common[1, 0, 1]


def test_row_strided_view_with_0xff_behind_the_rows(ctx):
    rng = np.random.default_rng(5)
    n, ns = C + 7, T + 3
    wide = np.full((n, ns + 13), 0xFF, dtype=np.uint8)
    wide[:, :ns] = _random_ids(rng, n, ns)
    view = wide[:, :ns]
    assert view.strides[0] == ns + 13
    common, match = _check(ctx, view, [0, 9, n])
    again = engine.pair_counts(ctx, np.ascontiguousarray(view), [0, 9, n])
    assert np.array_equal(common, again[0]) and np.array_equal(match, again[1])


def test_second_smaller_call_sees_nothing_of_the_first(ctx):
    rng = np.random.default_rng(6)
    seg_off = _offsets([C + 5, 2 * C])
    _check(ctx, np.full((int(seg_off[-1]), 2 * T + 1), 9, dtype=np.uint8), seg_off)
    _check(ctx, _random_ids(rng, 10, 3), [0, 4, 10])
    _check(ctx, _random_ids(rng, C + 1, T + 1), [0, 1, C + 1])


# ------------------------------------------------------------------------------------------------ the reference's goldens
def _device_step(ctx, seen):
    def step(ids, seg_off):
        out = engine.pair_counts(ctx, ids, seg_off)
        seen.append((np.array(ids), np.array(seg_off), out))
        return out
    return step


def _finish_cache_writers():
    import threading
    for t in threading.enumerate():
        if t.name == "snpmatch-parse-cache":
            t.join()


@pytest.mark.parametrize("name", pairsnp_util.CASES)
def test_goldens_through_the_device_call(name, ctx, tmp_path, monkeypatch):
    case = pairsnp_util.load(name)
    seen = []
    monkeypatch.setattr(pairsnp, "count_pairs", _device_step(ctx, seen))
    monkeypatch.chdir(tmp_path)
    names = pairsnp_util.write_inputs(case, str(tmp_path))
    db = pairsnp_util.write_db(case, str(tmp_path))
    cohort = pairsnp.PairCohort.from_files(names, db, False)
    assert np.array_equal(cohort.common, case["cohort_common"]) and np.array_equal(cohort.match, case["cohort_match"])
    t_common, t_match = pairsnp_twin.pair_counts(seen[0][0], seen[0][1])
    assert np.array_equal(cohort.common, t_common) and np.array_equal(cohort.match, t_match)
    for (a, b), text in zip(case["pairs"].tolist(), case["json"].tolist()):
        stats = pairsnp.pairwiseScore(names[a], names[b], False, "pair", db)
        ids, seg_off, (common, match) = seen[-1]
        twin = pairsnp_twin.pair_counts(ids, seg_off)
        assert np.array_equal(common, twin[0]) and np.array_equal(match, twin[1])
        assert open("pair.matches.json").read() == text
        assert pairsnp.dumps(stats) == text and pairsnp.dumps(cohort.stats(a, b)) == text
    _finish_cache_writers()


def test_command_line_on_files(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    for name, pair in (("pairsnp_f_db", (1, 3)), ("pairsnp_g_bed", (2, 0)), ("pairsnp_e_disjoint", (0, 1))):
        case = pairsnp_util.load(name)
        names = pairsnp_util.write_inputs(case, str(tmp_path))
        db = pairsnp_util.write_db(case, str(tmp_path))
        texts = dict(zip(map(tuple, case["pairs"].tolist()), case["json"].tolist()))
        with_db = ["-d", db] if db else []
        assert cli.main(["pairsnp", "-i", names[pair[0]], "-j", names[pair[1]], "-o", "x"] + with_db) == 0
        assert open("x.matches.json").read() == texts[pair]
        assert cli.main(["pairsnp-batch", "-i"] + names + ["-o", "plate"] + with_db) == 0
        z = np.load("plate.pairs.npz")
        assert np.array_equal(z["common"], case["cohort_common"]) and np.array_equal(z["match"], case["cohort_match"])
        rows = [ln.split("\t") for ln in open("plate.pairs.tsv").read().splitlines()[1:]]
        assert len(rows) == len(names) * (len(names) - 1) // 2
        for row in rows:
            ref = json.loads(texts[(names.index(row[0]), names.index(row[1]))])
            assert int(row[3]) == ref["matches"][1] and row[4] == repr(float(ref["matches"][0]))
        _finish_cache_writers()
    # one multi-sample VCF as a cohort
    case = pairsnp_util.load("pairsnp_b_phasing")
    axis = sorted(set(zip(case["chr_0"].tolist(), case["pos_0"].tolist())) | set(zip(case["chr_1"].tolist(), case["pos_1"].tolist())))
    gts = np.full((len(axis), 2), "./.", dtype="U3")
    for s in range(2):
        where = dict(zip(zip(case["chr_%d" % s].tolist(), case["pos_%d" % s].tolist()), case["gt_%d" % s].tolist()))
        for r, key in enumerate(axis):
            gts[r, s] = where.get(key, "./.")
    vcf = pairsnp_util.write_vcf("plate.vcf", ["p0", "p1"], np.array([c for c, _ in axis]), np.array([p for _, p in axis]), gts)
    assert cli.main(["pairsnp-batch", "-i", vcf, "-o", "v"]) == 0
    ref = json.loads(dict(zip(map(tuple, case["pairs"].tolist()), case["json"].tolist()))[(0, 1)])
    row = open("v.pairs.tsv").read().splitlines()[1].split("\t")
    assert row[:2] == ["p0", "p1"] and int(row[3]) == ref["matches"][1] and row[4] == repr(float(ref["matches"][0]))
