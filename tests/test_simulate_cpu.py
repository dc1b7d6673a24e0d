"""simulate (host only): ``snpmatch_amd.core.simulate`` against goldens of the unmodified reference ``simulateSNPs`` /
``simulateSNPs_F1`` run under ``np.random.seed`` (tests/golden/make_golden_simulate.py) -- the same rows and the same genotypes from the
same seed, because the mirror makes the same legacy ``np.random`` calls in the same order; the goldens regenerate byte for byte where
the reference is at hand; the written bed file goes back through ``ParseInputs``; the ``simulate`` subcommand with ``--seed``."""
import glob
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from snpmatch_amd import cli
from snpmatch_amd.core import f1search, parsers, simulate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["inbred_e0", "inbred_e05", "inbred_all", "inbred_code3", "f1_h1", "f1_h05", "f1_h0", "f1_noseg"]


def _duck(case):
    side = types.SimpleNamespace(snps=case["snps"], accessions=case["accessions"], chromosomes=case["chromosomes"], positions=case["positions"])
    return types.SimpleNamespace(g=side, g_acc=side)


def _run(case, out_file=None):
    np.random.seed(int(case["seed"]))
    if bool(case["f1"]):
        return simulate.simulateSNPs_F1(_duck(case), str(case["who"]), int(case["num"]), out_file, float(case["err_rate"]), float(case["het_frac"]))
    return simulate.simulateSNPs(_duck(case), str(case["who"]), int(case["num"]), out_file, float(case["err_rate"]))


def test_every_golden_is_listed(golden_dir):
    assert sorted(os.path.basename(p)[9:-4] for p in glob.glob(os.path.join(golden_dir, "simulate_*.npz"))) == sorted(CASES)
    assert all(os.path.getsize(os.path.join(golden_dir, "simulate_%s.npz" % c)) < 20000 for c in CASES)


def test_goldens_regenerate_byte_for_byte(golden_dir, tmp_path):
    run = subprocess.run([sys.executable, os.path.join(golden_dir, "make_golden_simulate.py"), str(tmp_path)], capture_output=True, text=True)
    if run.returncode == 3:
        pytest.skip("the reference is not on this machine: " + run.stderr.strip())
    assert run.returncode == 0, run.stderr[-2000:]
    for c in CASES:
        name = "simulate_%s.npz" % c
        assert open(str(tmp_path / name), "rb").read() == open(os.path.join(golden_dir, name), "rb").read(), name


@pytest.mark.parametrize("name", CASES)
def test_mirror_replays_the_reference(name, golden_dir):
    case = np.load(os.path.join(golden_dir, "simulate_%s.npz" % name))
    frame = _run(case)
    assert list(frame.columns) == ["chr", "pos", "snp"] and frame.shape == (int(case["num"]), 3)
    assert np.array_equal(np.array(frame["chr"], dtype="U"), case["out_chr"])
    assert np.array_equal(np.array(frame["pos"], dtype="U"), case["out_pos"])
    assert np.array_equal(np.array(frame["snp"], dtype="U"), case["out_gt"])
    assert all(type(v) is str for v in frame["snp"])                            # 0/0, where the reference's frame holds b'0/0'
    again = _run(case)
    assert again.equals(frame)
    np.random.seed(int(case["seed"]) + 1)                                       # another seed: another sample
    other = (simulate.simulateSNPs_F1(_duck(case), str(case["who"]), int(case["num"]), None, float(case["err_rate"]), float(case["het_frac"]))
             if bool(case["f1"]) else simulate.simulateSNPs(_duck(case), str(case["who"]), int(case["num"]), None, float(case["err_rate"])))
    assert name in ("inbred_all", "inbred_code3") or not other.equals(frame)    # (all rows, no error: nothing left to draw)


def test_what_the_goldens_plant(golden_dir):
    load = lambda c: np.load(os.path.join(golden_dir, "simulate_%s.npz" % c))   # noqa: E731
    e0 = load("inbred_e0")
    acc = e0["snps"][:, 0]
    assert (acc == -1).any() and (acc == 2).any() and int(float(e0["err_rate"]) * int(e0["num"])) == 0
    # err_rate 0: every drawn genotype is the accession's own call there
    at = {(c, p): k for k, (c, p) in enumerate(zip(e0["chromosomes"].tolist(), e0["positions"].tolist()))}
    rows = [at[(c, int(p))] for c, p in zip(e0["out_chr"].tolist(), e0["out_pos"].tolist())]
    assert rows == sorted(rows) and len(set(rows)) == 50
    assert np.array_equal(parsers.snp_binary_to_gt(acc[rows]).astype("U"), e0["out_gt"])
    e05 = load("inbred_e05")
    rows = [at[(c, int(p))] for c, p in zip(e05["out_chr"].tolist(), e05["out_pos"].tolist())]
    changed = (parsers.snp_binary_to_gt(acc[rows]).astype("U") != e05["out_gt"]).sum()
    assert 1 <= changed <= 5                                                    # five redrawn from 0 / 1 / 2: some keep their value
    every = load("inbred_all")
    assert int(every["num"]) == (acc >= 0).sum()
    c3 = load("inbred_code3")
    assert (c3["out_gt"] == "").sum() == (c3["snps"][:, 1] == 3).sum() > 0        # a code without a text: the reference's empty genotype
    assert (load("f1_h1")["out_gt"] == "0/1").sum() > (load("f1_h05")["out_gt"] == "0/1").sum() > 0 == (load("f1_h0")["out_gt"] == "0/1").sum()
    ns = load("f1_noseg")
    assert not ((ns["snps"][:, 2] != ns["snps"][:, 4]) & (ns["snps"][:, 4] >= 0)).any() and "0/1" not in ns["out_gt"].tolist()


@pytest.mark.parametrize("name", ["inbred_e05", "f1_h05"])
def test_bed_file_round_trip_through_parse_inputs(name, golden_dir, tmp_path):
    case = np.load(os.path.join(golden_dir, "simulate_%s.npz" % name))
    bed = str(tmp_path / (name + ".bed"))
    _run(case, bed)
    text = open(bed).read()
    assert "b'" not in text and text.splitlines()[0].split("\t") == [case["out_chr"][0], case["out_pos"][0], case["out_gt"][0]]
    inputs = parsers.ParseInputs(bed, False)
    inputs.wait_for_cache()
    assert np.array_equal(inputs.chrs, case["out_chr"]) and np.array_equal(inputs.pos, case["out_pos"].astype(np.int64))
    assert np.array_equal(inputs.gt, case["out_gt"])
    drawn = np.array([{"0/0": 0, "1/1": 1, "0/1": 2}[t] for t in case["out_gt"].tolist()], dtype=np.uint8)
    assert np.array_equal(f1search.hard_classes(inputs.gt), drawn) and len(set(drawn.tolist())) == 3
    assert np.array_equal(inputs.wei.sum(axis=1), np.ones(len(drawn)))


def test_command_with_a_seed(golden_dir, tmp_path):
    case = np.load(os.path.join(golden_dir, "simulate_inbred_e05.npz"))
    db = str(tmp_path / "db.npz")
    regions = np.array([[0, 170], [170, 300]], dtype=np.int64)
    np.savez(db, snps=case["snps"], accessions=case["accessions"], positions=case["positions"], chrs=np.array(["Chr1", "Chr2"]), chr_regions=regions)
    out = str(tmp_path / "sample.bed")
    assert cli.main(["simulate", "-d", db, "-a", "A0", "-n", "100", "-p", "0.05", "--seed", "12", "-o", out]) == 0
    lines = [ln.split("\t") for ln in open(out).read().splitlines()]
    assert [ln[0] for ln in lines] == case["out_chr"].tolist() and [ln[1] for ln in lines] == case["out_pos"].tolist()
    assert [ln[2] for ln in lines] == case["out_gt"].tolist()
    f1 = np.load(os.path.join(golden_dir, "simulate_f1_h05.npz"))
    assert cli.main(["simulate", "-d", db, "-a", "A2xA3", "-n", "120", "-p", "0.05", "--f1", "--het_frac", "0.5", "--seed", "16", "-o", out]) == 0
    lines = [ln.split("\t") for ln in open(out).read().splitlines()]
    assert [ln[1] for ln in lines] == f1["out_pos"].tolist() and [ln[2] for ln in lines] == f1["out_gt"].tolist()
    assert cli.main(["simulate", "-d", db, "-a", "nobody", "-n", "10", "-o", out]) == 2
    import snpmatch.core.simulate as drop_in
    assert drop_in is simulate and drop_in.potatoSimulate is simulate.potatoSimulate
