"""genotype_cross_hmm without a GPU: host layer + numpy twin against the reference's goldens (lines, states, omega bits), the
tables against the reference's probabilities, the two FORMAT-DP readers against each other, the argument validation of the C ABI,
the new subcommand's flags and the ``snpmatch.core.infer`` alias."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import ghmm_twin
import ghmm_util
from snpmatch_amd import _lib, cli, engine
from snpmatch_amd.core import _vcf, genotype_cross, infer, parsers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libsnpmatch_hip.so not built (run ./build_lib.sh)")


@needs_lib
@pytest.mark.parametrize("name", ghmm_util.CASES)
def test_host_layer_with_twin_writes_the_reference_file(name, tmp_path, monkeypatch):
    case = ghmm_util.load(name)
    seen = {}

    def step(*args):
        seen["state"], seen["omega"] = ghmm_twin.cross_hmm(*args)
        seen["args"] = args
        return seen["state"]

    lines = ghmm_util.golden_lines(case, monkeypatch, tmp_path, step, "f2.vcf.gz" if name.endswith("phasing") else "f2.vcf")
    assert lines.tolist() == case["lines"].tolist()
    assert np.array_equal(seen["state"], case["state"])
    assert np.array_equal(seen["omega"].view(np.uint64), case["omega"].view(np.uint64))
    assert np.array_equal(np.asarray(seen["args"][3]), case["chain_off"])
    assert lines[0] == "id,,," + ",".join(case["samples"][case["kept"]]) and lines[1] == "pheno,," + ",0" * len(case["kept"])


@pytest.mark.parametrize("name", ghmm_util.CASES)
def test_tables_equal_the_references_probabilities(name):
    case = ghmm_util.load(name)
    emission, logI, logE = infer.emission_tables(case["depth_levels"], 0.036)
    have = ~np.isnan(case["emission"])
    assert have.any() and np.array_equal(emission[have].view(np.uint64), case["emission"][have].view(np.uint64))
    assert not np.isnan(logI).any() and not np.isnan(logE).any() and logE.shape == (6, len(case["depth_levels"]), 4, 3)
    genome = __import__("json").loads(str(case["genome_json"]))
    rate = np.mean(np.array(genome["recomb_rates"])) if "recomb_rates" in genome else 3.5
    sizes = np.diff(case["chain_off"])
    for k, length in enumerate(genome["ref_chrlen"]):
        if sizes[k]:
            mine = infer._transition_frame(np.int64(length) / 1000000, int(sizes[k]), rate).values
            assert np.array_equal(mine.view(np.uint64), case["trans"][k].view(np.uint64))


def test_golden_cases_cover_what_they_are_for():
    assert np.diff(ghmm_util.load("ghmm_g_short_chains")["chain_off"]).tolist() == [1, 2, 3]
    d = ghmm_util.load("ghmm_d_het_parents")
    assert (~np.isnan(d["emission"][:, :, 0, 0])).any(axis=1).all()                  # all six ordered parental pairs
    e = ghmm_util.load("ghmm_e_extremes")
    assert e["kept"].tolist() == [0, 1, 2, 3, 4] and len(e["samples"]) == 6           # the low-coverage sample is dropped
    assert np.array_equal(e["omega"][:, 3, 0], e["omega"][:, 3, 2])                  # never called: AA and BB tie at every step
    assert "recomb_rates" not in str(ghmm_util.load("ghmm_f_no_rates")["genome_json"])
    b = ghmm_util.load("ghmm_b_phasing")
    assert np.any(np.char.find(b["vcf_gt"][:, 1], "|") >= 0) and np.any(np.char.find(b["vcf_gt"][:, 1], "/") >= 0)
    assert np.any(np.isin(ghmm_util.load("ghmm_c_multiallelic")["vcf_gt"], ["1/2", "0/2", "2/2", "1|2"]))
    assert set(np.unique(ghmm_util.load("ghmm_a_f2")["vcf_dp"]).tolist()) == set(range(9))


def test_model_class_mirrors_the_reference_surface():
    p1, p2 = np.array([0, 1, 2, 0], dtype=np.int8), np.array([1, 0, 0, 2], dtype=np.int8)
    m = infer.IdentifyAncestryF2individual(1.5, p1, p2, recomb_rate=3.5, base_error=0.036, sample_depth=np.array([0.5, 1.5, 2.5, 4.0]))
    assert m.params["num_markers"] == 4 and m.init_prob == [0.25, 0.5, 0.25] and m.emission_prob.shape == (3, 4, 4)
    assert list(m.transition_prob.index) == ["AA", "AB", "BB"] and np.allclose(m.transition_prob.values.sum(axis=1)[[0, 2]], 1.0)
    assert np.array_equal(m.emission_prob[:, :, 0], np.ones((3, 4)))                  # rint(0.5) = 0: the all-ones emission
    E, _, _ = infer.emission_tables([0.0, 2.0, 4.0], 0.036)
    assert np.array_equal(m.emission_prob[:, :, 1], E[2, 1]) and np.array_equal(m.emission_prob[:, :, 2], E[4, 1])   # rint(2.5) = 2
    assert np.array_equal(m.emission_prob[:, :, 3], E[1, 2])
    assert m.snp_to_observations(np.array([0, 1, 2, -1])).tolist() == [0, 2, 1, 3]
    assert infer.get_af(np.array([0, 1, 2])).tolist() == [0.0, 1.0, 0.5]
    assert infer.pair_index([0, 0, 1, 1, 2, 2], [1, 2, 0, 2, 0, 1]).tolist() == [0, 1, 2, 3, 4, 5]
    assert infer.polarize_snps(np.array([0, 1, 2, -1, 1]), np.array([0, 0, 0, 0, 2]), np.array([1, 1, 1, 1, 1])).tolist() == [0, 2, 1, 3, 2]
    vals, runs = infer.uniq_neighbor(np.array([0, 0, 1, 1, 1, 2]))
    assert vals.tolist() == [0, 1, 2] and runs.tolist() == [2, 3, 1]
    assert not hasattr(infer, "IdentifyStrechesofHeterozygosity")
    import snpmatch.core.infer as alias
    assert alias is infer


def test_a_recombination_fraction_above_one_is_refused(tmp_path, monkeypatch):
    case = dict(ghmm_util.load("ghmm_g_short_chains"))
    case["genome_json"] = np.array('{"ref_chrs": ["1", "2", "3"], "ref_chrlen": [1000000, 90000000, 300000], "recomb_rates": [3.4, 3.6, 4.25]}')
    with pytest.raises(ValueError, match="recombination fraction above 1"):
        ghmm_util.golden_lines(case, monkeypatch, tmp_path, lambda *a: pytest.fail("the device step must not be reached"))


# ------------------------------------------------------------------------------------------------ the FORMAT DP readers
VCF_HEAD = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tA\tB\tC\n"
VCF_BODY = ("Chr1\t10\t.\tA\tT\t50\tPASS\tDP=9\tGT:DP\t0/0:3\t0/1:.\t1|1:12\n"
            "Chr1\t20\t.\tA\tT\t50\tPASS\t.\tGT:AD:DP\t./.:1,2:0\t1/1:0,7\t0/0\n"          # entries that end before their DP
            "Chr1\t30\t.\tA\tT\t50\tPASS\t.\tGT\t0/0\t0/1\t1/1\n"                            # a FORMAT without DP
            "Chr2\t5\t.\tA\tT\t50\tPASS\t.\tDP:GT\t007:0/0\t-2:0|1\t+4:1/2\n")
WANT_DP = [[3, -1, 12], [0, -1, -1], [-1, -1, -1], [7, -2, 4]]


def _bgzf(text, path, member=100):
    """BGZF: independent gzip members with their size in a 'BC' extra subfield, then the empty end-of-file member"""
    import struct
    import zlib
    raw = text.encode()
    with open(path, "wb") as fh:
        for a in list(range(0, len(raw), member)) + [len(raw)]:
            chunk = raw[a:a + member] if a < len(raw) else b""
            comp = zlib.compressobj(6, zlib.DEFLATED, -15)
            body = comp.compress(chunk) + comp.flush()
            fh.write(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(body) + 25))
            fh.write(body + struct.pack("<II", zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk)))
    return path


@needs_lib
@pytest.mark.parametrize("kind", ["plain", "gzip", "bgzf"])
def test_generic_and_native_depth_readers_agree(kind, tmp_path):
    path = str(tmp_path / ("f2.vcf" if kind == "plain" else "f2.vcf.gz"))
    if kind == "plain":
        open(path, "w").write(VCF_HEAD + VCF_BODY)
    elif kind == "gzip":
        with gzip.open(path, "wt") as fh:
            fh.write(VCF_HEAD + VCF_BODY)
    else:
        _bgzf(VCF_HEAD + VCF_BODY, path)
    assert _lib.vcf_parse_calls(path, depth=True) is not None                    # the native reader takes the file
    native, generic = _vcf.read_call_codes(path, native=True, depth=True), _vcf.read_call_codes(path, native=False, depth=True)
    assert native["dp"].dtype == np.int32 and generic["dp"].dtype == np.int32
    assert native["dp"].tolist() == WANT_DP and native["dp"].tobytes() == generic["dp"].tobytes()
    assert native["codes"].tobytes() == generic["codes"].tobytes() and native["has_dp"] and generic["has_dp"]
    assert native["codes"].tobytes() == _vcf.read_call_codes(path, native=True)["codes"].tobytes()
    both = parsers.import_vcf_calls(path, depth=True)
    assert both["calldata/DP"].tolist() == WANT_DP and "calldata/DP" not in parsers.import_vcf_calls(path)


@needs_lib
def test_short_records_odd_depths_and_files_without_depth(tmp_path, capsys):
    short = str(tmp_path / "short.vcf")
    open(short, "w").write(VCF_HEAD + VCF_BODY + "Chr2\t9\t.\tA\tT\t50\tPASS\t.\tGT:DP\t0/0:5\t1/1:6\n")      # a record without its last sample column
    assert _lib.vcf_parse_calls(short, depth=True) is None                       # not the native reader's to interpret
    got = parsers.import_vcf_calls(short, depth=True)
    assert got["calldata/DP"].tolist() == WANT_DP + [[5, 6, -1]] and got["codes"][-1].tolist() == [0, 1, 3]
    odd = str(tmp_path / "odd.vcf")
    open(odd, "w").write(VCF_HEAD + "Chr1\t10\t.\tA\tT\t50\tPASS\t.\tGT:DP\t0/0:3\t0/1:1e1\t1/1:2\n")
    assert _lib.vcf_parse_calls(odd, depth=True) is None                         # '1e1': declined, the generic reader decides (-1)
    assert parsers.import_vcf_calls(odd, depth=True)["calldata/DP"].tolist() == [[3, -1, 2]]
    none = str(tmp_path / "none.vcf")
    open(none, "w").write(VCF_HEAD + "Chr1\t30\t.\tA\tT\t50\tPASS\tDP=8\tGT\t0/0\t0/1\t1/1\n")
    for native in (True, False):
        with pytest.raises(SystemExit):
            parsers.import_vcf_calls(none, native=native, depth=True)
        assert "DP" in capsys.readouterr().err
    assert parsers.import_vcf_calls(none)["codes"].tolist() == [[0, 2, 1]]       # the default mode still reads the file


def test_depth_reader_under_asan_and_ubsan(tmp_path):
    """the per-sample DP mode of csrc/snpm_vcf.cpp, compiled with its own driver under AddressSanitizer + UBSan and run directly"""
    exe = str(tmp_path / "vcf_dp_asan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "vcf_dp_asan_driver.cpp"),
                           os.path.join(ROOT, "snpmatch_amd", "csrc", "snpm_vcf.cpp"), "-lz", "-o", exe])
    good, gz, short = str(tmp_path / "good.vcf"), str(tmp_path / "good.vcf.gz"), str(tmp_path / "short.vcf")
    open(good, "w").write(VCF_HEAD + VCF_BODY * 300)
    _bgzf(VCF_HEAD + VCF_BODY * 300, gz, member=997)
    open(short, "w").write(VCF_HEAD + VCF_BODY + "Chr2\t9\t.\tA\tT\t50\tPASS\t.\tGT:DP\t0/0:5\n")
    # (a library the environment preloads may come before the ASan runtime: the driver is its own program and ASan copes)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:verify_asan_link_order=0", UBSAN_OPTIONS="print_stacktrace=1", SNPM_VCF_BLOCK_KB="4")
    r = subprocess.run([exe, good, gz, short], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = r.stdout.strip().split("\n")
    want_sum = 300 * int(np.array(WANT_DP).sum())
    assert out[0] == "good.vcf rc=0 records=1200 samples=3 flags_dp=1 sum=%d first=3,-1,12" % want_sum
    assert out[1] == "good.vcf.gz rc=0 records=1200 samples=3 flags_dp=1 sum=%d first=3,-1,12" % want_sum
    assert out[2].startswith("short.vcf rc=-4") and out[-1] == "done"


# ------------------------------------------------------------------------------------------------ the C ABI without a device
@needs_lib
def test_abi_refuses_bad_arguments_before_touching_a_device():
    codes, rank, pair, off, logT, logI, logE, _, _ = ghmm_util.random_case(3, (2, 0, 4), n_depth=2)
    codes, rank = np.ascontiguousarray(codes[:, :3]), np.ascontiguousarray(rank[:, :3])

    def refused(match, codes=codes, rank=rank, pair=pair, off=off, logT=logT, logI=logI, logE=logE):
        with pytest.raises(AssertionError, match=match):
            engine.cross_hmm(None, codes, rank, pair, off, logT, logI, logE)

    refused("start at 0", off=[1, 2, 2, 6])
    refused("must not decrease", off=[0, 4, 3, 6])
    refused("end at n", off=[0, 2, 2, 5])
    refused("end at n", off=[0, 2, 2, 9])
    refused("pair must be below 6", pair=np.array([0, 1, 6, 0, 0, 0], dtype=np.uint8))
    bad = rank.copy()
    bad[5, 2] = 2
    refused("depth_rank at or above n_depth", rank=bad)
    bad = codes.copy()
    bad[4, 1] = 0xFF
    refused("genotype code", codes=bad)
    bad[4, 1] = 5
    refused("genotype code", codes=bad)
    for name, table in (("logT", logT), ("logI", logI), ("logE", logE)):
        bad = table.copy()
        bad.flat[bad.size - 1] = np.nan
        refused("NaN or \\+inf in " + name, **{name: bad})
    with_inf = logE.copy()
    with_inf[0, 0, 0, 0] = -np.inf
    refused("ctx is NULL", logE=with_inf)                    # -inf is a legal entry; sound arguments: only now is a context asked for
    refused("ctx is NULL")
    lib, ptr = _lib.load(), _lib.ptr
    args = (ptr(codes), ptr(rank), 6, 3, 2, ptr(pair), ptr(off), 3, ptr(logT), ptr(logI), ptr(logE), 2, None, None)
    assert lib.snpm_cross_hmm(None, *args) == _lib.SNPM_ERR_BADARG and b"ld smaller" in lib.snpm_last_error(None)
    args = (ptr(codes), ptr(rank), 6, -3, 3, ptr(pair), ptr(off), 3, ptr(logT), ptr(logI), ptr(logE), 2, None, None)
    assert lib.snpm_cross_hmm(None, *args) == _lib.SNPM_ERR_BADARG and b"negative size" in lib.snpm_last_error(None)
    # nothing to do: returns at once, without a context
    empty = (np.zeros((0, 4), dtype=np.uint8), np.zeros((0, 4), dtype=np.uint16), np.zeros(0, dtype=np.uint8))
    state, omega = engine.cross_hmm(None, *empty, [0, 0, 0], np.zeros((2, 3, 3)), logI, logE, return_omega=True)
    assert state.shape == (0, 4) and omega.shape == (0, 4, 3)
    assert engine.cross_hmm(None, *empty, [0], np.zeros((0, 3, 3)), logI, logE).shape == (0, 4)
    assert engine.cross_hmm(None, codes[:, :0], rank[:, :0], pair, off, logT, logI, logE).shape == (6, 0)


# ------------------------------------------------------------------------------------------------ the command line
def test_subcommand_flags():
    args = vars(cli.get_options("x", "y").parse_args(["genotype_cross_hmm", "-i", "a.vcf", "-d", "d", "-e", "e", "-p", "1x2",
                                                       "--genome", "g.json", "-o", "o.csv", "-v"]))
    assert (args["inFile"], args["hdf5File"], args["hdf5accFile"], args["parents"], args["genome"], args["outFile"]) == \
        ("a.vcf", "d", "e", "1x2", "g.json", "o.csv")
    assert args["logDebug"] is True and args["func"] is cli.snpmatch_genotype_cross_hmm
    defaults = vars(cli.get_options("x", "y").parse_args(["genotype_cross_hmm"]))
    assert (defaults["genome"], defaults["outFile"], defaults["logDebug"]) == ("athaliana_tair10", "genotype_cross_hmm", False)
    assert "genotype_cross_hmm" in genotype_cross.HMM_REFUSED and "--hmm" in genotype_cross.HMM_REFUSED
    assert "not provided by this package" in genotype_cross.HMM_REFUSED


def test_subcommand_asks_for_its_inputs(tmp_path, capsys):
    with pytest.raises(SystemExit):
        cli.main(["genotype_cross_hmm", "-i", str(tmp_path / "missing.vcf"), "-d", "db.snpm", "-p", "1x2"])
    assert "does not exist" in capsys.readouterr().err
    vcf = str(tmp_path / "f2.vcf")
    open(vcf, "w").write(VCF_HEAD + VCF_BODY)
    with pytest.raises(SystemExit):
        cli.main(["genotype_cross_hmm", "-i", vcf, "-d", "db.snpm"])
    assert "parents not specified" in capsys.readouterr().err
