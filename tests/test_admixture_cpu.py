"""admixture without a GPU: the numpy twin of the device primitive (tests/admixture_twin.py) against plain loops and, in fp64, against
itself in long double within the bounds the GPU tests use; the planted panel (three Balding-Nichols populations, pure and admixed
accessions) over 20 seeds; the host layer -- row sums, flags, canonical order, the ``--pops`` file, samples, the ``admixture``
subcommand with the twin in the place of the device; every refusal of ``snpm_panel_admix`` that needs no device; and the kernel
source itself, compiled for the host and run by real threads under AddressSanitizer + UBSan (tests/adm_host_driver.cpp on
tests/host_kernel/, a stand-alone child process)."""
import itertools
import json
import os
import re

import numpy as np
import pytest

import admixture_twin as twin
import host_kernel_util
import sitestats_twin
import test_pca_cpu as pca_cpu
from snpmatch_amd import _lib, cli, engine
from snpmatch_amd.core import admixture, pca, sitestats, snp_genotype

PLANTED_ITERATIONS = 300


# ------------------------------------------------------------------------------------------------ the twin
def _edge_matrix():
    """12 rows x 7 columns: row 0 all missing, column 6 all missing, a code 3, row 1 all ref (F' reaches EPS), row 2 all alt (1 - EPS)"""
    rng = np.random.default_rng(7)
    snps = rng.choice(np.array([-1, 0, 1, 2], dtype=np.int8), size=(12, 7), p=[0.1, 0.45, 0.35, 0.1])
    snps[0] = -1
    snps[1] = 0
    snps[2] = 1
    snps[2, 3] = -1
    snps[5, 2] = 3
    snps[:, 6] = -1
    return snps


@pytest.mark.parametrize("K", [1, 3])
def test_twin_against_plain_loops(K):
    snps = _edge_matrix()
    Q, F = twin.random_start(np.random.default_rng(70 + K), 7, 12, K)
    Qn, Fn, ll = twin.step(snps, Q, F)
    Ql, Fl, lll = twin.step_loops(snps, Q, F)
    assert np.allclose(Qn, Ql, rtol=1e-12, atol=0) and np.allclose(Fn, Fl, rtol=1e-12, atol=0) and abs(ll - lll) <= 1e-12 * abs(lll)
    # an all-missing row and an all-missing column keep their bits; the clamps are reached; code 3 is no call
    assert np.array_equal(Fn[0], F[0]) and np.array_equal(Qn[6], Q[6])
    assert (Fn[1] == twin.EPS).all() and (Fn[2] == twin.ONE_MINUS_EPS).all()
    other = snps.copy()
    other[5, 2] = -1
    for a, b in zip(twin.step(other, Q, F), (Qn, Fn, ll)):
        assert np.array_equal(a, b)
    if K == 1:                              # one component: Q stays 1, F' is the allele frequency of the row
        g, called = twin.dosage(snps[3:])
        assert (Qn[:6] == 1.0).all() and np.allclose(Fn[3:, 0], (g * called).sum(axis=1) / (2.0 * called.sum(axis=1)), rtol=1e-12)
    # selections: lists with repeats and a range are the matrix indexed that way
    cols, rows = [5, 5, 0, 3], range(3, 11)
    Qs, Fs = twin.random_start(np.random.default_rng(71), 4, 8, K)
    for a, b in zip(twin.step(snps, Qs, Fs, cols, rows), twin.step(snps[3:11][:, cols], Qs, Fs)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("shape", [(42, 600, 3), (130, 2500, 8), (65, 1025, 16)])
def test_twin_in_fp64_within_the_bounds_of_the_long_double_twin(shape):
    n, R, K = shape
    rng = np.random.default_rng(100 + n)
    snps = rng.choice(np.array([-1, 0, 1, 2], dtype=np.int8), size=(R, n), p=[0.1, 0.45, 0.35, 0.1])
    Q, F = twin.random_start(rng, n, R, K)
    ratios = twin.worst_ratios(twin.step(snps, Q, F), twin.step(snps, Q, F, dtype=np.longdouble), snps)
    print("fp64 twin %r: worst error / bound F %.4f Q %.4f ll %.4f" % ((shape,) + ratios))
    assert max(ratios) <= 1.0


# ------------------------------------------------------------------------------------------------ the planted panel
def used_rows(case):
    """the rows ``pca.standardise`` keeps among the 42 panel accessions with the command's defaults"""
    counts = sitestats_twin.site_counts(case["snps"], [case["panel"]], np.arange(twin.PLANTED_ROWS))[0]
    return np.flatnonzero(pca.standardise(counts, len(case["panel"]), 0.05, 0.1)[0])


def check_planted_fit(case, Q, trace):
    """the assertions on a fit of the planted panel (Q [42, 3] in panel order): the likelihood rises at every iteration; under the
    best permutation every pure accession has its argmax on its own population with that component >= 0.5.  Returns that minimum and
    the permutation; the six admixed accessions are reported, not asserted."""
    trace = np.asarray(trace, dtype=np.float64)
    assert len(trace) == PLANTED_ITERATIONS and (np.diff(trace) > 0).all(), "smallest increment %r" % float(np.diff(trace).min())
    truth = case["truth"][case["panel"]]
    n_pure = len(case["pure"])
    perm = max(itertools.permutations(range(3)), key=lambda pm: float((Q[:n_pure][:, list(pm)] * truth[:n_pure]).sum()))
    Qp = Q[:, list(perm)]
    own = (Qp[:n_pure] * truth[:n_pure]).sum(axis=1)
    assert np.array_equal(np.argmax(Qp[:n_pure], axis=1), np.argmax(truth[:n_pure], axis=1)) and own.min() >= 0.5, float(own.min())
    print("pure minimum %.3f, smallest increment %.3g, admixed |q - truth| max %.3f" % (own.min(), np.diff(trace).min(), np.abs(Qp[n_pure:] - truth[n_pure:]).max()))
    return float(own.min()), perm


@pytest.mark.parametrize("seed", range(20))
def test_planted_populations_are_recovered(seed):
    """3 Balding-Nichols populations (Fst 0.15) of 12 inbred accessions plus 6 two-way admixed ones, K = 3, 300 iterations from the
    seeded start of the command"""
    case = twin.planted_case(seed)
    used = used_rows(case)
    Q, F = admixture.random_start(seed, len(case["panel"]), len(used), 3)
    Q, F, trace = twin.admix(case["snps"], Q, F, PLANTED_ITERATIONS, case["panel"], used)
    check_planted_fit(case, Q, trace)


# ------------------------------------------------------------------------------------------------ the host layer
def test_row_sums_flags_and_canonical_order():
    rng = np.random.default_rng(9)
    snps = rng.choice(np.array([-1, 0, 1, 2], dtype=np.int8), size=(300, 40), p=[0.1, 0.45, 0.35, 0.1])
    for K in (1, 2, 5, 16):
        Q, F = twin.random_start(rng, 40, 300, K)
        Qn, Fn, ll = twin.admix(snps, Q, F, 3)
        assert (np.abs(Qn.sum(axis=1) - 1.0) <= K * twin.U52).all() and (Fn >= twin.EPS).all() and (Fn <= twin.ONE_MINUS_EPS).all()
        assert (np.diff(ll) > 0).all() or K == 1                       # (one component: the first iteration is the fixed point)
        Qf, Ff, llf = twin.admix(snps, Q, F, 1, update_q=False)
        assert np.array_equal(Qf, Q) and np.array_equal(Ff, twin.step(snps, Q, F)[1]) and llf[0] == ll[0]
        Qq, Fq, _ = twin.admix(snps, Q, F, 1, update_f=False)
        assert np.array_equal(Fq, F) and np.array_equal(Qq, twin.step(snps, Q, F)[0])
        Q0, F0, ll0 = twin.admix(snps, Q, F, 1, update_q=False, update_f=False)
        assert np.array_equal(Q0, Q) and np.array_equal(F0, F) and ll0[0] == ll[0]
    # descending column sums, the lower index on a tie
    assert admixture.canonical_order(np.array([[0.2, 0.5, 0.3], [0.1, 0.6, 0.3]])).tolist() == [1, 2, 0]
    assert admixture.canonical_order(np.array([[0.25, 0.5, 0.25], [0.25, 0.5, 0.25]])).tolist() == [1, 0, 2]
    # run_em: blocks of 20, the stop inside a block, the evaluating call at the end
    calls = []

    def admix(Q, F, n_iter, update_q, update_f):
        calls.append((n_iter, update_q, update_f))
        return twin.admix(snps, Q, F, n_iter, None, None, update_q, update_f)
    Q, F = admixture.random_start(3, 40, 300, 2)
    Qe, Fe, trace, final, converged = admixture.run_em(admix, Q, F, max_iter=50, tol=0.0)
    assert [c[0] for c in calls] == [20, 20, 10, 1] and calls[-1][1:] == (False, False) and len(trace) == 50 and not converged
    assert final > trace[-1] and np.array_equal(Qe, twin.admix(snps, Q, F, 50)[0])
    del calls[:]
    _, _, trace, _, converged = admixture.run_em(admix, Q, F, max_iter=2000, tol=1e-4)
    assert converged and len(trace) % 20 == 0 and len(trace) < 2000 and [c[0] for c in calls[:-1]] == [20] * (len(trace) // 20)
    best = admixture.fit(admix, 40, 300, 3, seed=5, restarts=3, max_iter=40, tol=0.0)
    assert best["loglik"] == max(r["loglik"] for r in best["runs"]) and [r["seed"] for r in best["runs"]] == [5, 6, 7]
    assert (np.diff(best["Q"].sum(axis=0)) <= 0).all() and best["runs"][best["restart"]]["loglik"] == best["loglik"]


def test_sample_ancestry_recovers_a_held_out_accession():
    case = twin.planted_case(0)
    used = used_rows(case)
    Q, F = admixture.random_start(0, len(case["panel"]), len(used), 3)
    Q, F, _ = twin.admix(case["snps"], Q, F, PLANTED_ITERATIONS, case["panel"], used)
    v = case["snps"][used][:, case["held"]].T
    classes = np.where((v >= 0) & (v <= 2), v, admixture.NO_CLASS).astype(np.uint8)
    classes[:, ::2] = admixture.NO_CLASS                             # records at every second row only
    q, n_sites = admixture.sample_ancestry(np.concatenate([classes, np.full((1, len(used)), admixture.NO_CLASS, dtype=np.uint8)]), F)
    assert np.isnan(q[3]).all() and n_sites[3] == 0 and (n_sites[:3] > 0.4 * len(used)).all() and np.allclose(q[:3].sum(axis=1), 1.0)
    for s, a in enumerate(case["held"].tolist()):
        cluster = np.argmax(Q[:36][case["pop"][case["pure"]] == case["pop"][a]].mean(axis=0))
        assert np.argmax(q[s]) == cluster and q[s, cluster] >= 0.5


# ------------------------------------------------------------------------------------------------ the library's validation
def test_refusals_that_need_no_device():
    lib = _lib.load()
    bad = _lib.SNPM_ERR_BADARG
    cols = np.zeros(3, dtype=np.int32)
    Q = np.full((3, 2), 0.5)
    F = np.full((5, 2), 0.25)
    ll = np.zeros(4)

    def call(ncols=3, n_rows=5, K=2, n_iter=4, flags=3, cols=cols, Q=Q, F=F, ll=ll):
        rc = lib.snpm_panel_admix(None, _lib.ptr(cols), ncols, None, 0, n_rows, K, n_iter, flags, _lib.ptr(Q), _lib.ptr(F), _lib.ptr(ll))
        return rc, lib.snpm_last_error(None).decode()
    assert call(ncols=-1) == (bad, "negative size") and call(n_rows=-1) == (bad, "negative size")
    rc, msg = call(ncols=11553, cols=None)
    assert rc == bad and "too many accessions" in msg and "SNPM_PCA_MAX_ACCESSIONS" in msg
    rc, msg = call(n_rows=2 ** 31, F=None)
    assert rc == bad and "2^31 rows" in msg
    for K in (0, -1, 17):
        assert call(K=K) == (bad, "K outside 1 .. SNPM_ADMIX_MAX_K")
    for n_iter in (0, -1, 10001):
        assert call(n_iter=n_iter) == (bad, "n_iter outside 1 .. 10000")
    for flags in (4, 8, 7, 2 ** 31):
        rc, msg = call(flags=flags)
        assert rc == bad and "unknown flag bits" in msg
    assert call(Q=None) == (bad, "Q / loglik is NULL") and call(ll=None) == (bad, "Q / loglik is NULL") and call(F=None) == (bad, "F is NULL")
    for poison in (np.nan, np.inf, -np.inf, -1e-300):
        q = Q.copy()
        q[2, 1] = poison
        assert call(Q=q) == (bad, "Q holds an entry that is not finite or is negative")
    for delta in (2e-9, -2e-9):
        q = Q.copy()
        q[1, 0] += delta
        assert call(Q=q) == (bad, "a row of Q does not sum to 1 (within 1e-9)")
    q = Q.copy()
    q[1, 0] += 5e-10
    assert call(Q=q) == (bad, "panel is NULL")
    for poison in (np.nan, np.inf, 0.0, 1.0, 0.9e-6, 1.0 - 0.9e-6, -0.25):
        f = F.copy()
        f[4, 1] = poison
        rc, msg = call(F=f)
        assert rc == bad and msg.startswith("F holds an entry outside")
    f = F.copy()
    f[0, 0], f[4, 1] = twin.EPS, twin.ONE_MINUS_EPS
    assert call(F=f) == (bad, "panel is NULL")
    # sound arguments reach the panel check: the limits themselves, the empty cases
    assert call() == (bad, "panel is NULL") and call(flags=0) == (bad, "panel is NULL") and call(n_iter=10000, ll=np.zeros(10000)) == (bad, "panel is NULL")
    assert call(K=16, Q=np.full((3, 16), 1.0 / 16), F=np.full((5, 16), 0.5)) == (bad, "panel is NULL")
    assert call(ncols=0, cols=None, Q=None, F=None, ll=None) == (bad, "panel is NULL") and call(n_rows=0, F=None) == (bad, "panel is NULL")
    assert "snpm_panel_admix" in _lib.SYMBOLS


def test_header_constants_are_the_python_ones():
    text = open(os.path.join(host_kernel_util.ROOT, "include", "snpmatch_hip.h")).read()
    kernels = open(os.path.join(host_kernel_util.ROOT, "snpmatch_amd", "csrc", "snpm_k_adm.hpp")).read()
    for src in (text, kernels):
        assert int(re.search(r"#define SNPM_ADMIX_MAX_K (\d+)", src).group(1)) == engine.ADMIX_MAX_K == admixture.MAX_K == 16
        assert float(re.search(r"#define SNPM_ADMIX_EPS (\S+)", src).group(1)) == engine.ADMIX_EPS == admixture.EPS == twin.EPS
    assert int(re.search(r"#define SNPM_ADMIX_UPDATE_F (\d+)u", text).group(1)) == engine.ADMIX_UPDATE_F
    assert int(re.search(r"#define SNPM_ADMIX_UPDATE_Q (\d+)u", text).group(1)) == engine.ADMIX_UPDATE_Q
    assert admixture.NO_CLASS == engine.F1X_NO_CLASS and admixture.potatoAdmixture.__doc__
    assert "Hardy-Weinberg" in admixture.__doc__ and "haploid" in admixture.__doc__


def test_group_and_streamed_panels_are_refused_with_the_reason():
    for cls, why in ((engine.GroupPanel, "spread over several GPUs"), (engine.StreamedPanel, "not a resident panel")):
        with pytest.raises(TypeError, match="admix needs every accession column on one device") as err:
            engine.admix(cls.__new__(cls), np.ones((1, 1)), np.zeros((0, 1)))
        assert why in str(err.value)


# ------------------------------------------------------------------------------------------------ the command
PLANTED_COMMAND_SEED = 0


def _tsv(path):
    return [ln.split("\t") for ln in open(path).read().splitlines()]


def check_planted_outputs(case, out, with_pops=True, with_samples=True):
    """what both command tests (the twin here, the device in test_gpu_admixture.py) ask of the files of ``admixture -K 3 --max_iter
    300 --tol 0`` on the 42 panel accessions"""
    names = case["names"][case["panel"]].tolist()
    lines = _tsv(out + ".admixture.Q.tsv")
    assert lines[0] == ["accession"] + (["population"] if with_pops else []) + ["Q1", "Q2", "Q3", "cluster"] and [ln[0] for ln in lines[1:]] == names
    z = np.load(out + ".admixture.npz")
    assert set(z.files) >= {"accessions", "Q", "F", "chr", "pos", "p", "trace", "seeds"}
    Q, R = z["Q"], len(z["pos"])
    assert Q.shape == (42, 3) and z["F"].shape == (R, 3) and z["p"].shape == (R,) and z["accessions"].tolist() == names
    assert np.array_equal(np.array([[float(x) for x in ln[-4:-1]] for ln in lines[1:]]), Q) and [ln[-1] for ln in lines[1:]] == ["K%d" % (k + 1) for k in np.argmax(Q, axis=1)]
    assert (np.diff(Q.sum(axis=0)) <= 0).all() and (np.abs(Q.sum(axis=1) - 1.0) <= 3 * twin.U52).all()      # canonical order; rows sum to 1
    assert np.array_equal(case["positions"][used_rows(case)], z["pos"])
    _, perm = check_planted_fit(case, Q, z["trace"])
    # the population file is what the other commands read as --pops
    pairs = sitestats.read_populations(out + ".admixture.pops.tsv")
    assert [a for a, _ in pairs] == names and [c for _, c in pairs] == [ln[-1] for ln in lines[1:]]
    stats = json.load(open(out + ".admixture.json"))
    assert set(stats) >= {"K", "min_maf", "max_missing", "seed", "max_iter", "tol", "accessions", "rows_selected", "rows_used", "rows_dropped", "iterations", "converged",
                          "loglik", "restarts", "cluster_sizes"}
    assert stats["rows_used"] == R and stats["rows_selected"] == R + sum(stats["rows_dropped"].values()) and stats["iterations"] == PLANTED_ITERATIONS
    assert sum(stats["cluster_sizes"].values()) == 42 and stats["loglik"] > z["trace"][-1] and not stats["converged"]
    if with_pops:
        table = stats["population_by_cluster"]
        for q in range(3):                  # every pure population sits in one cluster, its own under the permutation
            assert table["pop%d" % q] == {"K%d" % (k + 1): (12 if k == perm[q] else 0) for k in range(3)}
        assert sum(table["mixed"].values()) == 6
    if with_samples:
        anc = _tsv(out + ".ancestry.tsv")
        assert anc[0] == ["sample", "n_sites", "Q1", "Q2", "Q3", "cluster"] and [ln[0] for ln in anc[1:]] == case["names"][case["held"]].tolist() + ["blank"]
        assert anc[4][1:] == ["0", "NA", "NA", "NA", "NA"]
        for ln, a in zip(anc[1:4], case["held"].tolist()):
            own = perm[int(case["pop"][a][3:])]
            assert 0.35 * R < int(ln[1]) <= 0.6 * R and ln[-1] == "K%d" % (own + 1) and float(ln[2 + own]) >= 0.5
    return stats, z


@pytest.fixture
def planted(monkeypatch, tmp_path):
    """the planted DB as an .npz; the two device calls are the twins"""
    case = twin.planted_case(PLANTED_COMMAND_SEED)
    snps = case["snps"]
    calls = []
    stub = engine.Panel.__new__(engine.Panel)
    stub.h = None

    def admix(panel, Q, F, n_iter=1, cols=None, rows=None, update_q=True, update_f=True):
        calls.append((n_iter, cols, rows, update_q, update_f))
        return twin.admix(snps, Q, F, n_iter, cols, rows, update_q, update_f)
    monkeypatch.setattr(snp_genotype.Genotype, "panel", lambda self, ctx=None, packed=None: stub)
    monkeypatch.setattr(engine, "site_counts", lambda panel, groups=None, rows=None: sitestats_twin.site_counts(snps, groups, rows))
    monkeypatch.setattr(engine, "admix", admix)
    return (case,) + pca_cpu.write_planted_inputs(case, tmp_path) + (calls,)


def test_command_on_the_planted_panel(planted, tmp_path):
    case, db, pops, accs, vcf, calls = planted
    out = str(tmp_path / "out")
    run = ["admixture", "-d", db, "-K", "3", "--seed", str(PLANTED_COMMAND_SEED), "--max_iter", str(PLANTED_ITERATIONS), "--tol", "0"]
    assert cli.main(run + ["--pops", pops, "-i", vcf, "-o", out]) == 0
    stats, z = check_planted_outputs(case, out)
    assert [c[0] for c in calls] == [20] * 15 + [1] and calls[-1][3:] == (False, False) and np.array_equal(calls[0][1], case["panel"])
    assert (stats["K"], stats["seed"], stats["populations"], stats["rows_selected"]) == (3, 0, ["pop0", "pop1", "pop2", "mixed"], 600)
    assert z["seeds"].tolist() == [0] and len(stats["restarts"]) == 1
    # the start is the documented one: the same iterations by hand give the same bits (before the canonical order)
    used = used_rows(case)
    Q, F = admixture.random_start(PLANTED_COMMAND_SEED, 42, len(used), 3)
    Qh = twin.admix(case["snps"], Q, F, PLANTED_ITERATIONS, case["panel"], used)[0]
    assert np.array_equal(z["Q"], Qh[:, admixture.canonical_order(Qh)])
    # -a, no samples, two restarts, the default stop: no population column, no ancestry file of this run
    out2 = str(tmp_path / "out2")
    assert cli.main(["admixture", "-d", db, "-K", "3", "-a", accs, "--restarts", "2", "--seed", "4", "-o", out2]) == 0
    s2 = json.load(open(out2 + ".admixture.json"))
    assert not os.path.exists(out2 + ".ancestry.tsv") and "population_by_cluster" not in s2 and [r["seed"] for r in s2["restarts"]] == [4, 5]
    assert s2["loglik"] == max(r["loglik"] for r in s2["restarts"]) and s2["converged"] and s2["iterations"] % 20 == 0 and _tsv(out2 + ".admixture.Q.tsv")[0][1] == "Q1"
    # --bed: the rows of a region; --sites: the listed rows; the written --pops file feeds the next run
    assert cli.main(["admixture", "-d", db, "-K", "2", "--pops", out + ".admixture.pops.tsv", "--bed", "Chr2,1,100000", "--max_iter", "20", "-o", out2]) == 0
    z3, s3 = np.load(out2 + ".admixture.npz"), json.load(open(out2 + ".admixture.json"))
    assert set(z3["chr"].tolist()) == {"Chr2"} and s3["rows_selected"] == 100 and z3["Q"].shape == (42, 2) and set(s3["population_by_cluster"]) == {"K1", "K2", "K3"}
    sites = str(tmp_path / "x.pruned.tsv")
    with open(sites, "w") as fh:
        fh.write("chr\tpos\n" + "".join("%s\t%d\n" % (c, p) for c, p in list(zip(z["chr"], z["pos"]))[::2]))
    assert cli.main(["admixture", "-d", db, "-K", "1", "--sites", sites, "--min_maf", "0", "--max_missing", "1", "--max_iter", "20", "-o", out2]) == 0
    z4 = np.load(out2 + ".admixture.npz")
    assert z4["pos"].tolist() == z["pos"][::2].tolist() and (z4["Q"] == 1.0).all() and len(z4["accessions"]) == 45
    # refusals: exit code 2, and the device is not asked for an iteration
    asked = len(calls)
    one = tmp_path / "one.txt"
    one.write_text("%s\n" % case["names"][0])
    two = tmp_path / "two.txt"
    two.write_text("%s\n%s\n" % (case["names"][0], case["names"][1]))
    for bad in (["-K", "3", "--bed", "Chr1,1,1000", "--sites", sites], ["-K", "0"], ["-K", "17"], ["-K", "3", "-a", str(two)], ["-K", "1", "-a", str(one)],
                ["-K", "3", "--min_maf", "0.5", "--bed", "Chr1,1,5000"], ["-K", "3", "--min_maf", "0.6"], ["-K", "3", "--pops", pops, "-a", accs],
                ["-K", "3", "--restarts", "0"]):
        assert cli.main(["admixture", "-d", db, "-o", out2] + bad) == 2, bad
    assert len(calls) == asked
    args = cli.get_options("d", "v").parse_args(["admixture", "-d", "db.snpm", "-K", "5", "-o", "out"])
    assert (args.K, args.min_maf, args.max_missing, args.seed, args.restarts, args.max_iter, args.tol, args.inFile) == (5, 0.05, 0.1, 1, 1, 2000, 1e-7, None)


# ------------------------------------------------------------------------------------------------ the kernels, on the host
def test_kernel_source_on_the_host_under_asan_and_ubsan(tmp_path):
    """every block of k_adm_rows / k_adm_cols / k_adm_fold run by its real threads with a barrier and the exchanges of a wave,
    exact-size heap buffers, arbitrary pad bytes, stale workspaces, one iteration against a plain loop in long double within the
    bounds: the widths around a wave and a column block of 256, the row counts around a wave's run, a block of 32 rows and the
    shortest split of 16, the split boundary of one and of two column blocks; every K step; each flag alone, both and none; column
    and row lists with repeats; a dense range with row0 > 0; all-missing rows and columns; code 3; F at EPS and 1 - EPS"""
    cases = host_kernel_util.run_driver("adm_host_driver", tmp_path)
    field = lambda ln, k: next(f.split("=")[1] for f in ln.split() if f.startswith(k + "="))      # noqa: E731
    grid = [ln for ln in cases if ln.split()[1] == "grid"]
    assert {int(field(ln, "acc")) for ln in grid} == {1, 2, 63, 64, 65, 129, 130, 255, 256, 257}
    assert {int(field(ln, "rows")) for ln in grid} == {1, 15, 16, 17, 63, 64, 65, 1023, 1025, 2500}
    assert {field(ln, "layout") for ln in grid} == {"0", "1", "2"} and {field(ln, "K") for ln in cases if " K=" in ln} == {"1", "2", "3", "4", "5", "8", "9", "16"}
    assert {field(ln, "flags") for ln in cases if "flags=" in ln} == {"0", "1", "2", "3"}
    edge = {int(field(ln, "rows")): int(field(ln, "splits")) for ln in cases if ln.split()[1] == "split-edge-1"}
    assert edge == {8191: 512, 8192: 512, 8193: 482}
    by_name = {ln.split()[1]: ln for ln in cases}
    assert {"lists", "lists-packed", "lists-split", "row0", "all-missing", "blank-rows-columns", "code3", "evaluate-only", "split-wide", "plan-pitch"} <= set(by_name)
    assert field(by_name["all-missing"], "cells") == "0"
    worst = {k: max(float(field(ln, k)) for ln in cases if k + "=" in ln) for k in ("worst_f", "worst_q", "worst_ll")}
    print("host kernels: worst error / bound %r" % worst)
