"""pairsnp without a GPU: the host layer (``core/pairsnp.py``, the two subcommands) against the reference's goldens with the numpy
twin (tests/pairsnp_twin.py) in the place of the device call, and every validation branch of ``snpm_pair_counts`` through a NULL
context (the library validates on the host before it asks for a device)."""
import json
import os

import numpy as np
import pytest

import pairsnp_twin
import pairsnp_util
from snpmatch_amd import cli, engine
from snpmatch_amd.core import pairsnp, parsers


@pytest.fixture
def twin(monkeypatch):
    calls = []

    def step(ids, seg_off):
        calls.append((np.array(ids), np.array(seg_off)))
        return pairsnp_twin.pair_counts(ids, seg_off)
    monkeypatch.setattr(pairsnp, "count_pairs", step)
    return calls


def _finish_cache_writers():
    import threading
    for t in threading.enumerate():
        if t.name == "snpmatch-parse-cache":
            t.join()


@pytest.mark.parametrize("name", pairsnp_util.CASES)
def test_goldens_through_pairwise_score_and_cohort(name, twin, tmp_path, monkeypatch):
    case = pairsnp_util.load(name)
    monkeypatch.chdir(tmp_path)
    names = pairsnp_util.write_inputs(case, str(tmp_path))
    db = pairsnp_util.write_db(case, str(tmp_path))
    from snpmatch_amd.core.snpmatch import pairwiseScore          # the reference's import path
    cohort = pairsnp.PairCohort.from_files(names, db, False)
    assert len(twin) == 1 and twin[0][0].shape[1] == len(names)             # ONE device call for the whole cohort
    for (a, b), text in zip(case["pairs"].tolist(), case["json"].tolist()):
        stats = pairwiseScore(names[a], names[b], False, "pair", db)
        assert twin[-1][0].shape[1] == 2
        assert open("pair.matches.json").read() == text
        assert pairsnp.dumps(stats) == text
        assert pairsnp.dumps(cohort.stats(a, b)) == text
        ref = json.loads(text)
        assert stats["matches"][1] == ref["matches"][1] and sorted(stats) == sorted(ref)
    _finish_cache_writers()


def test_nan_line_and_empty_pair_are_in_the_goldens():
    case = pairsnp_util.load("pairsnp_e_disjoint")
    texts = dict(zip(map(tuple, case["pairs"].tolist()), case["json"].tolist()))
    assert '"2": [\n        NaN,\n        0\n    ]' in texts[(0, 1)]                     # named by both, no shared position
    assert json.loads(texts[(0, 2)])["matches"][1] == 0 and "NaN" in texts[(0, 2)]      # nothing in common at all


def test_text_ids_number_whole_strings_and_stop_at_127():
    (a, b), texts = pairsnp.text_ids([np.array(["0/1", "1/0", "0|1", "0/1"]), np.array([["1/0"], ["2/10"]])])
    assert texts.tolist() == ["0/1", "0|1", "1/0", "2/10"]
    assert a.tolist() == [1, 3, 2, 1] and b.tolist() == [[3], [4]] and a.dtype == np.uint8
    many = np.array(["%d/%d" % (i // 16, i % 16) for i in range(128)])
    (ids,), texts = pairsnp.text_ids([many[:127]])
    assert len(texts) == 127 and ids.max() == 127 and ids.min() == 1
    assert np.array_equal(texts[ids - 1], many[:127])
    with pytest.raises(ValueError, match="128 distinct genotype texts"):
        pairsnp.text_ids([many[:100], many[64:]])
    (ids,), texts = pairsnp.text_ids([np.zeros(0, dtype="U3")])
    assert ids.shape == (0,) and len(texts) == 0


def test_call_codes_would_merge_what_pairsnp_tells_apart():
    texts = np.array(["0/1", "1/0", "1/2", "0/2"])
    assert len(set(parsers.gt_call_codes(texts).tolist())) == 2
    assert len(set(pairsnp.text_ids([texts])[0][0].tolist())) == 4


@pytest.mark.parametrize("pos, what", [([10, 20, 20, 30], "repeat or decrease"), ([10, 30, 20, 40], "repeat or decrease")],
                         ids=["duplicate", "descending"])
def test_cohort_refuses_positions_that_repeat_or_decrease(pos, what, twin):
    good = (np.repeat("Chr1", 4), np.array([10, 20, 30, 40]), np.repeat("0/0", 4))
    bad = (np.repeat("Chr1", 4), np.array(pos), np.repeat("0/0", 4))
    with pytest.raises(ValueError, match=what) as err:
        pairsnp.PairCohort(["good", "bad"], [good[0], bad[0]], [good[1], bad[1]], [good[2], bad[2]])
    assert "sample bad" in str(err.value) and "Chr1" in str(err.value)
    assert not twin
    # the same positions on two chromosomes are in order
    two = (np.array(["Chr1", "Chr1", "Chr2", "Chr2"]), np.array([10, 20, 10, 20]), np.repeat("0/0", 4))
    cohort = pairsnp.PairCohort(["good", "two"], [good[0], two[0]], [good[1], two[1]], [good[2], two[2]])
    assert cohort.seg_off.tolist() == [0, 4, 6] and cohort.common[:, 0, 1].tolist() == [2, 0]


def test_cohort_from_a_multi_sample_vcf(twin, tmp_path):
    chrs = np.array(["Chr1", "Chr1", "Chr1", "Chr2", "Chr2"])
    pos = np.array([5, 9, 12, 3, 8])
    gts = np.array([["0/0", "0/0", "./."], ["0/1", "1/0", "0/1"], ["./.", "1/1", "1/1"], ["1|1", "1/1", ".|."], ["0/2", "0/2", "0/2"]])
    vcf = pairsnp_util.write_vcf(str(tmp_path / "plate.vcf"), ["A", "B", "C"], chrs, pos, gts)
    cohort = pairsnp.PairCohort.from_vcf(vcf)
    assert cohort.samples == ["A", "B", "C"] and cohort.calls.tolist() == [4, 5, 3]        # './.' and '.|.' are no records
    assert cohort.chr_ids == ["1", "2"] and cohort.seg_off.tolist() == [0, 3, 5]
    assert cohort.common.sum(axis=0).tolist() == [[4, 4, 2], [4, 5, 3], [2, 3, 3]]
    assert cohort.match.sum(axis=0).tolist() == [[4, 2, 2], [2, 5, 2], [2, 2, 3]]
    stats = cohort.stats(0, 2)
    assert stats["1"] == [1.0, 1] and stats["2"] == [1.0, 1] and stats["matches"] == [1.0, 2]
    assert stats["unique"] == {"A": [0.5, 4], "C": [1 / 3.0, 3]}
    cohort.write(str(tmp_path / "out"))
    lines = open(str(tmp_path / "out.pairs.tsv")).read().splitlines()
    assert lines[0].split("\t") == ["sample_1", "sample_2", "matches", "common", "fraction", "unique_1", "unique_2"]
    assert lines[1:] == ["A\tB\t2\t4\t0.5\t0\t1", "A\tC\t2\t2\t1.0\t2\t1", "B\tC\t2\t3\t%r\t2\t0" % (2 / 3.0)]
    z = np.load(str(tmp_path / "out.pairs.npz"))
    assert z["samples"].tolist() == ["A", "B", "C"] and z["chrs"].tolist() == ["1", "2"] and z["calls"].tolist() == [4, 5, 3]
    assert np.array_equal(z["common"], cohort.common) and np.array_equal(z["match"], cohort.match)


def test_command_line_pairsnp_and_batch(twin, tmp_path, monkeypatch):
    case = pairsnp_util.load("pairsnp_f_db")
    monkeypatch.chdir(tmp_path)
    names = pairsnp_util.write_inputs(case, str(tmp_path))
    db = pairsnp_util.write_db(case, str(tmp_path))
    texts = dict(zip(map(tuple, case["pairs"].tolist()), case["json"].tolist()))
    assert cli.main(["pairsnp", "-i", names[2], "-j", names[0], "-d", db, "-o", "x"]) == 0
    assert open("x.matches.json").read() == texts[(2, 0)]
    assert cli.main(["pairsnp-batch", "-i"] + names + ["-d", db, "-o", "plate"]) == 0
    rows = [ln.split("\t") for ln in open("plate.pairs.tsv").read().splitlines()[1:]]
    assert len(rows) == 6
    for row in rows:
        a, b = names.index(row[0]), names.index(row[1])
        ref = json.loads(texts[(a, b)])
        assert a < b and int(row[3]) == ref["matches"][1] and row[4] == repr(ref["matches"][0])
        assert int(row[5]) == ref["unique"][names[a]][1] - int(row[3]) and int(row[6]) == ref["unique"][names[b]][1] - int(row[3])
    # defaults of the reference: -o pairsnp, no DB
    case = pairsnp_util.load("pairsnp_g_bed")
    names = pairsnp_util.write_inputs(case, str(tmp_path))
    assert cli.main(["pairsnp", "-i", names[0], "-j", names[1]]) == 0
    assert open("pairsnp.matches.json").read() == dict(zip(map(tuple, case["pairs"].tolist()), case["json"].tolist()))[(0, 1)]
    _finish_cache_writers()
    with pytest.raises(SystemExit):
        cli.main(["pairsnp", "-i", names[0], "-j", "absent.bed"])
    # one multi-sample VCF is a cohort
    vcf = pairsnp_util.write_vcf("plate.vcf", ["A", "B"], np.array(["1", "1"]), np.array([4, 6]), np.array([["0/0", "0/0"], ["0/1", "1/1"]]))
    assert cli.main(["pairsnp-batch", "-i", vcf, "-o", "v"]) == 0
    assert open("v.pairs.tsv").read().splitlines()[1] == "A\tB\t1\t2\t0.5\t0\t0"


# ------------------------------------------------------------------------------------------------ the library's validation
def _refused(ids, seg_off, message):
    with pytest.raises(AssertionError, match=message):
        engine.pair_counts(None, ids, seg_off)


def test_validation_runs_without_a_context():
    ids = np.ones((6, 3), dtype=np.uint8)
    _refused(ids, [1, 6], "seg_off must start at 0")
    _refused(ids, [0, 4, 3, 6], "seg_off must not decrease")
    _refused(ids, [0, 3, 5], "seg_off must end at n")
    _refused(ids, [0, 3, 7], "seg_off must end at n")
    _refused(ids, [0], "seg_off must end at n")                      # no segment, but records
    bad = ids.copy()
    bad[4, 2] = 128
    _refused(bad, [0, 6], "an id above 127")
    bad[4, 2] = 127
    _refused(bad, [0, 6], "ctx is NULL")                             # sound arguments: only the context is missing
    wide = np.full((6, 8), 200, dtype=np.uint8)
    wide[:, :3] = 5
    _refused(wide[:, :3], [0, 2, 6], "ctx is NULL")                  # 200 in a padding column is never looked at
    wide[3, 2] = 200
    _refused(wide[:, :3], [0, 2, 6], "an id above 127")


def test_validation_of_sizes_and_limits_through_the_c_abi():
    from snpmatch_amd import _lib
    lib = _lib.load()
    ids = np.ones((4, 4), dtype=np.uint8)
    off = np.array([0, 4], dtype=np.int64)
    out = np.zeros((2, 4, 4), dtype=np.int32)

    def call(n, ns, ld, n_seg, seg=off):
        rc = lib.snpm_pair_counts(None, _lib.ptr(ids), n, ns, ld, _lib.ptr(seg), n_seg, _lib.ptr(out[0]), _lib.ptr(out[1]))
        return rc, lib.snpm_last_error(None).decode()
    assert call(-1, 4, 4, 1) == (_lib.SNPM_ERR_BADARG, "negative size")
    assert call(4, -1, 4, 1) == (_lib.SNPM_ERR_BADARG, "negative size")
    assert call(4, 4, 4, -1) == (_lib.SNPM_ERR_BADARG, "negative size")
    assert call(4, 4, 3, 1) == (_lib.SNPM_ERR_BADARG, "ld smaller than n_samples")
    rc, msg = call(0, 4097, 4097, 0)
    assert rc == _lib.SNPM_ERR_BADARG and "too many samples" in msg and "SNPM_PAIR_MAX_SAMPLES" in msg
    zeros = np.zeros(10, dtype=np.int64)
    rc, msg = call(0, 4096, 4096, 9, zeros)                          # 9 x 4096^2 cells > 2^27
    assert rc == _lib.SNPM_ERR_BADARG and "SNPM_PAIR_MAX_CELLS" in msg
    long_seg = np.array([0, 2 ** 31], dtype=np.int64)
    rc, msg = call(2 ** 31, 0, 0, 1, long_seg)                       # (no sample: no id is read)
    assert rc == _lib.SNPM_ERR_BADARG and "2^31 records" in msg
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "snpmatch_hip.h")).read()
    assert "#define SNPM_PAIR_MAX_SAMPLES 4096" in header and "#define SNPM_PAIR_MAX_CELLS ((int64_t)1 << 27)" in header


def test_empty_shapes_return_without_a_device():
    common, match = engine.pair_counts(None, np.zeros((0, 3), dtype=np.uint8), [0, 0, 0])
    assert common.shape == (2, 3, 3) and not common.any() and not match.any()               # n == 0, n_seg > 0: zeroed outputs
    common, match = engine.pair_counts(None, np.zeros((0, 3), dtype=np.uint8), [0])
    assert common.shape == (0, 3, 3)
    common, match = engine.pair_counts(None, np.zeros((5, 0), dtype=np.uint8), [0, 5])
    assert common.shape == (1, 0, 0)


def test_twin_on_a_hand_made_matrix():
    ids = np.array([[1, 1, 0], [2, 1, 2], [0, 0, 3], [3, 3, 3]], dtype=np.uint8)
    common, match = pairsnp_twin.pair_counts(ids, [0, 2, 2, 4])
    assert common[0].tolist() == [[2, 2, 1], [2, 2, 1], [1, 1, 1]] and match[0].tolist() == [[2, 1, 1], [1, 2, 0], [1, 0, 1]]
    assert not common[1].any() and not match[1].any()
    assert common[2].tolist() == [[1, 1, 1], [1, 1, 1], [1, 1, 2]] and match[2].tolist() == common[2].tolist()
