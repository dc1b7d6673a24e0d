"""genotype_cross without a GPU: the numpy twin against the reference's goldens, the host layer (with the twin in the place of the
device call) against the reference's files byte for byte, the genotype codes and their two readers, the genetic distance, the
argument validation of the C ABI, and the refusals of the command line."""
import os

import numpy as np
import pytest

import gcross_twin
import gcross_util
from snpmatch_amd import _lib, cli, engine
from snpmatch_amd.core import _vcf, genomes, genotype_cross, parsers

needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libsnpmatch_hip.so not built (run ./build_lib.sh)")


def _twin_step(record=None):
    def step(codes, p1, p2, win_off, lr_thres):
        geno, counts, lr_next = gcross_twin.cross_calls(codes, p1, p2, win_off, lr_thres)
        if record is not None:
            record.update(geno=geno, counts=counts, win_off=np.asarray(win_off), lr_next=lr_next, codes=codes, p1=p1, p2=p2)
        return geno
    return step


def _golden_lines(case, tmp_path, monkeypatch, record=None, vcf_name="f2.vcf"):
    """the package's lines for a golden case: VCF file -> reader -> host layer, the twin where the device call would be"""
    monkeypatch.setattr(genotype_cross, "genome", genomes.Genome(gcross_util.write_genome(case, str(tmp_path / "genome.json"))))
    monkeypatch.setattr(genotype_cross, "count_and_decide", _twin_step(record))
    vcf = gcross_util.write_vcf(str(tmp_path / vcf_name), case["vcf_chr"], case["vcf_pos"], case["vcf_gt"], case["samples"])
    cross = genotype_cross.GenotypeCross(gcross_util.DuckGenotype(case), str(case["parents"]), int(case["binLen"]), None, False)
    return cross, cross.genotype_cross(vcf, float(case["lr_thres"]))


@needs_lib
@pytest.mark.parametrize("name", gcross_util.CASES)
def test_host_layer_with_twin_writes_the_reference_file(name, tmp_path, monkeypatch):
    case = gcross_util.load(name)
    seen = {}
    cross, lines = _golden_lines(case, tmp_path, monkeypatch, seen, "f2.vcf.gz" if name.endswith("phasing") else "f2.vcf")
    out = str(tmp_path / "out.csv")
    cross.write_output_genotype_cross(lines, out)
    assert open(out).read() == "".join(ln + "\n" for ln in case["lines"].tolist())
    # the twin reproduces the recorded calls and counts, and no cell of a golden sits on the threshold
    assert np.array_equal(seen["geno"], case["geno"]) and np.array_equal(seen["counts"], case["counts"])
    assert np.array_equal(seen["win_off"], case["win_off"])
    assert gcross_twin.knife_edge_cells(seen["lr_next"], float(case["lr_thres"])) == 0
    # the lines say what geno says
    text = np.array(["NA", "0", "1", "2"])
    for w, ln in enumerate(case["lines"][2:].tolist()):
        assert ln.split(",")[3:] == text[case["geno"][w].astype(int) + 1].tolist()


def test_golden_cases_cover_what_they_are_for():
    d = gcross_util.load("gcross_d_sparse")
    sizes = np.diff(d["win_off"])
    assert sizes[:4].tolist() == [0, 1, 4, 5] and "Chr3" not in d["vcf_chr"] and np.all(sizes[-3:] == 0)
    assert np.all(d["geno"][:3] == -1) and np.any(d["geno"][3] >= 0)
    e = gcross_util.load("gcross_e_extremes")
    big = np.diff(e["win_off"]) >= 5
    assert np.all(e["geno"][big, 0] == 0) and np.all(e["geno"][big, 1] == 2) and np.all(e["geno"][:, 3] == -1)
    assert np.all(e["geno"][big, 2] == 1)
    b = gcross_util.load("gcross_b_phasing")
    assert np.all(np.char.find(b["vcf_gt"][:, 0], "|") == 1)
    mixed = np.char.find(b["vcf_gt"][:, 1], "|") == 1
    assert 0.2 < mixed.mean() < 0.4
    assert "1/2" in gcross_util.load("gcross_c_multiallelic")["vcf_gt"]
    assert "recomb_rates" in str(b["genome_json"]) and "recomb_rates" not in str(e["genome_json"])
    assert float(gcross_util.load("gcross_f_thres2706")["lr_thres"]) == 2.706 and float(gcross_util.load("gcross_f_thres1")["lr_thres"]) == 1.0


def test_scalar_window_call_agrees_with_the_twin():
    rng = np.random.default_rng(5)
    tot = rng.integers(0, 40, size=300)
    m = np.stack([rng.integers(0, t + 1, size=3) for t in tot])
    m[::7] = 0
    m[3::11, 0] = tot[3::11]
    m[5::13, 1] = m[5::13, 0]                    # ties
    for thres in (1.0, 1.5, 2.706):
        geno, _ = gcross_twin.decide(m[:, None, :], tot, thres)
        for k in range(len(tot)):
            call = genotype_cross.getWindowGenotype(m[k].tolist(), int(tot[k]), thres)[0]
            assert (-1 if call == 'NA' else call) == geno[k, 0], (m[k], tot[k], thres)
    assert genotype_cross.getWindowGenotype([3, 0, 0], 4, 1.5) == ('NA', 'NA')
    assert genotype_cross.getWindowGenotype([9, 1, 0], 10, 1.5)[1].startswith("1.00,")


def test_gt_text_to_code_and_back():
    text = np.array(["0/0", "1/1", "0/1", "1/0", "./.", "1/2", "0|0", "1|1", "0|1", "1|0", ".|.", "1|2", "0|0/1", "0/0/1", "./1"])
    want = [0, 1, 2, 2, 3, 4, 8, 9, 10, 10, 11, 12, 12, 4, 4]
    assert parsers.gt_call_codes(text).tolist() == want
    assert parsers.gt_call_codes(text.reshape(3, 5)).shape == (3, 5)
    assert [parsers.gt_call_code(t) for t in ("0", "1", ".", "")] == [parsers.GT_NO_SEPARATOR] * 4
    # the codes carry what parseGT reads: under the separator of the slice's first entry they give parseGT's values, also for
    # slices that mix both separators
    rng = np.random.default_rng(11)
    for _ in range(50):
        piece = rng.choice(text, size=12)
        codes = parsers.gt_call_codes(piece)
        assert np.array_equal(parsers.call_code_values(codes, bool(codes[0] & 8)), parsers.parseGT(piece)), piece


def _odd_vcf(tmp_path, name):
    rng = np.random.default_rng(3)
    texts = np.array(["0/0", "0/1", "1/1", "./.", "0|1", "1|0", ".", "1/2", "0|0", ".|.", "2|1"])
    n, s = 700, 9
    gt = rng.choice(texts, size=(n, s))
    chrom = np.repeat(["Chr1", "chr2", "3"], [300, 250, 150])
    pos = np.concatenate([np.sort(rng.choice(90000, size=k, replace=False)) + 1 for k in (300, 250, 150)])
    return gcross_util.write_vcf(str(tmp_path / name), chrom, pos, gt, ["s%d" % i for i in range(s)], fmt="DP:GT:GQ"), chrom, pos, gt


@needs_lib
@pytest.mark.parametrize("name", ["many.vcf", "many.vcf.gz"])
def test_native_and_python_code_readers_agree(name, tmp_path, monkeypatch):
    monkeypatch.setenv("SNPM_VCF_BLOCK_KB", "4")             # many blocks from a small file
    path, chrom, pos, gt = _odd_vcf(tmp_path, name)
    assert _lib.vcf_parse_calls(path) is not None            # the native reader takes the file
    fast, slow = _vcf.read_call_codes(path, native=True), _vcf.read_call_codes(path, native=False)
    for key in ("samples", "chr", "pos", "codes"):
        assert np.array_equal(fast[key], slow[key]), key
    assert fast["codes"].dtype == np.uint8 and fast["codes"].shape == gt.shape
    assert np.array_equal(fast["codes"], parsers.gt_call_codes(np.where(gt == ".", "./.", gt)))
    assert np.array_equal(fast["pos"], pos) and fast["chr"].tolist() == chrom.tolist()
    # samples_to_load=None means every sample, as in the reference
    full = parsers.import_vcf_file(path, samples_to_load=None)
    assert full["gt"].shape == gt.shape and full["samples"].tolist() == ["s%d" % i for i in range(9)]
    assert np.array_equal(parsers.gt_call_codes(full["gt"]), fast["codes"])
    assert np.array_equal(parsers.import_vcf_calls(path)["codes"], fast["codes"])


@needs_lib
def test_native_reader_declines_ragged_records(tmp_path):
    path = str(tmp_path / "ragged.vcf")
    with open(path, "w") as fh:
        fh.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ta\tb\tc\n")
        fh.write("1\t10\t.\tA\tT\t.\t.\t.\tGT\t0/0\t0/1\t1/1\n1\t20\t.\tA\tT\t.\t.\t.\tGT\t0/1\t1|1\n")
    assert _lib.vcf_parse_calls(path) is None
    got = _vcf.read_call_codes(path)                         # ... and the generic reader serves it: a missing column is './.'
    assert got["codes"].tolist() == [[0, 2, 1], [2, 9, 3]]


@needs_lib
def test_separator_less_genotypes_are_refused(tmp_path, monkeypatch, capsys):
    case = gcross_util.load("gcross_d_sparse")
    gt = case["vcf_gt"].copy()
    gt[17, 2] = "1"
    monkeypatch.setattr(genotype_cross, "genome", genomes.Genome(gcross_util.write_genome(case, str(tmp_path / "genome.json"))))
    monkeypatch.setattr(genotype_cross, "count_and_decide", _twin_step())
    vcf = gcross_util.write_vcf(str(tmp_path / "haploid.vcf"), case["vcf_chr"], case["vcf_pos"], gt, case["samples"])
    cross = genotype_cross.GenotypeCross(gcross_util.DuckGenotype(case), str(case["parents"]), int(case["binLen"]))
    with pytest.raises(SystemExit):
        cross.genotype_cross(vcf, 1.5)
    assert "unable to parse the format of GT in vcf!" in capsys.readouterr().err


@needs_lib
def test_duplicate_positions_are_refused(tmp_path, monkeypatch):
    case = gcross_util.load("gcross_d_sparse")
    pos = case["vcf_pos"].copy()
    pos[40] = pos[39]
    monkeypatch.setattr(genotype_cross, "genome", genomes.Genome(gcross_util.write_genome(case, str(tmp_path / "genome.json"))))
    monkeypatch.setattr(genotype_cross, "count_and_decide", _twin_step())
    vcf = gcross_util.write_vcf(str(tmp_path / "dup.vcf"), case["vcf_chr"], pos, case["vcf_gt"], case["samples"])
    cross = genotype_cross.GenotypeCross(gcross_util.DuckGenotype(case), str(case["parents"]), int(case["binLen"]))
    with pytest.raises(ValueError, match="more than once"):
        cross.genotype_cross(vcf, 1.5)


def test_parents_and_whole_panel_attributes():
    case = gcross_util.load("gcross_a_f2")
    cross = genotype_cross.GenotypeCross(gcross_util.DuckGenotype(case), str(case["parents"]), 100000)
    one, two = case["panel"][:, cross.p1_ix], case["panel"][:, cross.p2_ix]
    keep = (one != two) & (one >= 0) & (two >= 0)
    assert (cross.p1_ix, cross.p2_ix, cross.window_size) == (1, 4, 100000)
    assert np.array_equal(cross.snpsP1, one[keep]) and np.array_equal(cross.snpsP2, two[keep])
    assert np.array_equal(cross.commonSNPsPOS, case["positions"][keep]) and len(cross.commonSNPsCHR) == keep.sum()
    with pytest.raises(SystemExit):
        genotype_cross.GenotypeCross(gcross_util.DuckGenotype(case), "6191xnobody", 100000)
    with pytest.raises(SystemExit):
        genotype_cross.GenotypeCross(gcross_util.DuckGenotype(case), "a.vcf", 100000, father="b.vcf")


def test_estimated_cM_distance(tmp_path):
    # golden strings: the third field of the reference's lines
    for name in ("gcross_b_phasing", "gcross_e_extremes"):
        case = gcross_util.load(name)
        g = genomes.Genome(gcross_util.write_genome(case, str(tmp_path / (name + ".json"))))
        for ln in case["lines"][2:].tolist():
            window, chrid, cm = ln.split(",")[:3]
            start, end = window.split(":")[1].split("-")
            assert "%s" % g.estimated_cM_distance("%s,%d" % (chrid, int(round(np.mean([int(start), int(end)]))))) == cm
    assert g.estimated_cM_distance("Chr2,1,300000") == 3 * 150000.5 / 1000000
    with pytest.raises(AssertionError):
        g.estimated_cM_distance("Chr2")
    import snpmatch.core.genotype_cross as alias
    assert alias is genotype_cross


@needs_lib
def test_abi_refuses_bad_arguments_before_touching_a_device():
    """the library validates on the host first: with no context at all, what is wrong with the arguments is reported"""
    codes = np.zeros((6, 3), dtype=np.uint8)
    p1, p2 = np.zeros(6, dtype=np.int8), np.ones(6, dtype=np.int8)
    ok_off = [0, 2, 2, 6]

    def refused(match, codes=codes, p1=p1, p2=p2, off=ok_off):
        with pytest.raises(AssertionError, match=match):
            engine.cross_calls(None, codes, p1, p2, off, 1.5)

    refused("start at 0", off=[1, 2, 6])
    refused("must not decrease", off=[0, 4, 3, 6])
    refused("end at n", off=[0, 2, 5])
    refused("end at n", off=[0, 2, 9])
    refused("0, 1 or 2", p1=np.array([0, 0, 3, 0, 0, 0], dtype=np.int8))
    refused("0, 1 or 2", p2=np.array([1, 1, 1, -1, 1, 1], dtype=np.int8))
    refused("must differ", p2=np.array([1, 1, 1, 1, 0, 1], dtype=np.int8))
    bad = codes.copy()
    bad[4, 1] = 0xFF
    refused("genotype code", codes=bad)
    bad[4, 1] = 5
    refused("genotype code", codes=bad)
    refused("ctx is NULL")                                   # sound arguments: only now is a context asked for
    lib = _lib.load()
    rc = lib.snpm_cross_calls(None, _lib.ptr(codes), 6, 3, 2, _lib.ptr(p1), _lib.ptr(p2), _lib.ptr(np.array(ok_off, dtype=np.int64)), 3,
                              1.5, 5, None, None)
    assert rc == _lib.SNPM_ERR_BADARG and b"ld smaller" in lib.snpm_last_error(None)
    # nothing to do: returns at once, without a context
    geno, counts = engine.cross_calls(None, np.zeros((0, 4), dtype=np.uint8), [], [], [0, 0, 0], 1.5, return_counts=True)
    assert geno.shape == (2, 4) and np.all(geno == -1) and counts.shape == (2, 4, 3) and not counts.any()
    assert engine.cross_calls(None, np.zeros((0, 4), dtype=np.uint8), [], [], [0], 1.5).shape == (0, 4)
    assert engine.cross_calls(None, np.zeros((6, 0), dtype=np.uint8), p1, p2, ok_off, 1.5).shape == (3, 0)


@pytest.mark.parametrize("extra, message", [(["--hmm"], "--hmm"), (["-q", "father.vcf"], "--father")])
def test_cli_refuses_what_is_out_of_scope(extra, message, capsys):
    argv = ["genotype_cross", "-i", "f2.vcf", "-d", "db.snpm", "-p", "6091x6191", "-b", "300000", "-o", "out.csv"] + extra
    with pytest.raises(SystemExit) as stop:
        cli.main(argv)
    assert stop.value.code == 1
    err = capsys.readouterr().err
    assert message in err and "not provided by this package" in err


def test_cli_flags_match_the_reference():
    args = vars(cli.get_options("x", "y").parse_args(["genotype_cross", "-i", "a.vcf", "-d", "d", "-e", "e", "-p", "1x2", "-b", "300000",
                                                       "--genome", "g.json", "--lr_thres", "2.706", "-o", "o.csv", "-v"]))
    assert args["lr_thres"] == 2.706 and isinstance(args["lr_thres"], float) and args["binLen"] == 300000
    assert (args["inFile"], args["hdf5File"], args["hdf5accFile"], args["parents"], args["genome"], args["outFile"]) == \
        ("a.vcf", "d", "e", "1x2", "g.json", "o.csv")
    assert args["logDebug"] is True and args["hmm"] is False and args["father"] is None
    defaults = vars(cli.get_options("x", "y").parse_args(["genotype_cross"]))
    assert (defaults["lr_thres"], defaults["binLen"], defaults["genome"], defaults["outFile"]) == (1.5, 200000, "athaliana_tair10", "genotype_cross")
