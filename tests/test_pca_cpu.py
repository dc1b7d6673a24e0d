"""pca without a GPU: the numpy twin of the two device primitives (tests/pca_twin.py) against plain loops; ``standardise`` against a
brute-force loop on a matrix with every edge in it; ``decompose``; the identity of ``project``; the planted panel (three
Balding-Nichols populations) over 20 seeds; the ``pca`` subcommand with the twin in the place of the device; every refusal of
``snpm_panel_gram`` / ``snpm_panel_loadings`` that needs no device; and the kernel source itself, compiled for the host and run by
real threads under AddressSanitizer + UBSan (tests/pca_host_driver.cpp on tests/host_kernel/, a stand-alone child process)."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import host_kernel_util
import pca_twin as twin
import sitestats_twin
from snpmatch_amd import _lib, cli, engine
from snpmatch_amd.core import pca, snp_genotype


# ------------------------------------------------------------------------------------------------ the twin
def test_twin_against_plain_loops():
    rng = np.random.default_rng(5)
    snps = rng.choice(np.array([-1, 0, 1, 2, 3], dtype=np.int8), size=(23, 9), p=[0.15, 0.4, 0.3, 0.1, 0.05])
    for cols, rows in ((None, None), ([8, 8, 0, 3], None), (None, [22, 0, 0, 7]), ([4, 2, 2], range(3, 20)), ([1], [5])):
        ci = list(range(9)) if cols is None else list(cols)
        ri = list(range(23)) if rows is None else list(rows)
        tab = rng.normal(size=(len(ri), 4))
        vec = rng.normal(size=(len(ci), 3))
        t = [[0.0 if snps[r, c] < 0 else float(tab[k, min(int(snps[r, c]), 3)]) for c in ci] for k, r in enumerate(ri)]
        want_g = [[math.fsum(t[s][i] * t[s][j] for s in range(len(ri))) for j in range(len(ci))] for i in range(len(ci))]
        want_l = [[math.fsum(t[s][i] * vec[i, c] for i in range(len(ci))) for c in range(3)] for s in range(len(ri))]
        assert np.array_equal(twin.values(snps, tab, cols, rows), np.array(t).reshape(len(ri), len(ci)))
        assert np.allclose(twin.gram(snps, tab, cols, rows), want_g, rtol=0, atol=1e-12)
        assert np.allclose(twin.loadings(snps, tab, vec, cols, rows), want_l, rtol=0, atol=1e-12)
        # the exactly rounded forms differ from the loops only by the rounding of each product there
        assert np.allclose(twin.gram_exact(snps, tab, cols, rows), want_g, rtol=0, atol=1e-13)
        assert np.allclose(twin.loadings_exact(snps, tab, vec, cols, rows), want_l, rtol=0, atol=1e-13)
        assert np.array_equal(twin.gram_exact(snps, tab, cols, rows, cell_rows=[0]), twin.gram_exact(snps, tab, cols, rows)[:1])
        assert (twin.gram_abs(snps, tab, cols, rows) >= np.abs(twin.gram(snps, tab, cols, rows)) - 1e-12).all()
    # integer tables: exact whatever the order, the exact form included
    tab = twin.integer_table(rng, 23)
    g = twin.gram(snps, tab)
    assert np.array_equal(g, np.rint(g)) and np.array_equal(g, twin.gram_exact(snps, tab)) and np.array_equal(g, g.T)
    vec = rng.integers(-4, 5, size=(9, 5)).astype(np.float64)
    assert np.array_equal(twin.loadings(snps, tab, vec), twin.loadings_exact(snps, tab, vec))
    # an exact product pair: the low part is what the rounded product loses
    hi, lo = twin._two_product(np.array([1.0 + 2.0 ** -30]), np.array([1.0 + 2.0 ** -30]))
    assert hi[0] == 1.0 + 2.0 ** -29 and lo[0] == 2.0 ** -60


# ------------------------------------------------------------------------------------------------ standardise / decompose / project
def _standardise_loop(snps, min_maf, max_missing):
    keep, tab, ps, dropped = [], [], [], dict.fromkeys(pca.DROP_RULES, 0)
    n_listed = snps.shape[1]
    for row in snps.tolist():
        c0, c1, c2, other = row.count(0), row.count(1), row.count(2), sum(1 for v in row if v > 2)
        n = c0 + c1 + c2
        p = (2 * c1 + c2) / (2 * n) if n else float("nan")
        minor = min(2 * c1 + c2, 2 * n - 2 * c1 - c2)
        why = None
        if other:
            why = "other_code"
        elif n == 0:
            why = "no_call"
        elif minor == 0 or minor / (2 * n) < min_maf:
            why = "maf"
        elif (n_listed - n) / n_listed > max_missing:
            why = "missing"
        ps.append(p)
        keep.append(why is None)
        if why:
            dropped[why] += 1
            tab.append([0.0] * 4)
        else:
            r = 1.0 / math.sqrt(2.0 * p * (1.0 - p))
            tab.append([(0.0 - 2.0 * p) * r, (2.0 - 2.0 * p) * r, (1.0 - 2.0 * p) * r, 0.0])
    return np.array(keep), np.array(tab), np.array(ps), dropped


def test_standardise_against_a_brute_force_loop():
    rng = np.random.default_rng(11)
    snps = rng.choice(np.array([-1, 0, 1, 2], dtype=np.int8), size=(60, 20), p=[0.06, 0.5, 0.36, 0.08])
    snps[0] = -1                                                    # all missing
    snps[1] = 0                                                     # monomorphic ...
    snps[2] = 1
    snps[2, :2] = -1                                                # ... with missing calls
    snps[3, 5] = 3                                                  # an "other" code
    snps[4] = 0
    snps[4, 0] = 1                                                  # p = 2 / 40 = 0.05 exactly: kept
    snps[5] = 1
    snps[5, 0] = 0                                                  # p = 0.95: minor frequency 0.05 exactly, kept
    snps[6] = 0
    snps[6, 0] = 2                                                  # p = 1 / 40 < 0.05
    snps[7] = [0, 1] * 10
    snps[7, :2] = -1                                                # missing 2 / 20 = 0.1 exactly: kept
    snps[8] = [0, 1] * 10
    snps[8, :3] = -1                                                # missing 0.15
    snps[9] = 2                                                     # all het: p = 0.5
    snps[10, :] = -1
    snps[10, 3] = 3                                                 # an "other" code and nothing else
    counts = sitestats_twin.site_counts(snps)[0]
    for min_maf, max_missing in ((0.05, 0.1), (0.0, 1.0), (0.3, 0.3), (0.5, 0.0)):
        keep, tab, p, dropped = pca.standardise(counts, 20, min_maf, max_missing)
        wk, wt, wp, wd = _standardise_loop(snps, min_maf, max_missing)
        assert np.array_equal(keep, wk) and dropped == wd and sum(dropped.values()) == int((~keep).sum())
        assert np.array_equal(tab, wt) and np.array_equal(p, wp, equal_nan=True) and tab.dtype == np.float64 and tab.shape == (60, 4)
    keep, tab, p, dropped = pca.standardise(counts, 20)
    assert keep[[4, 5, 7, 9]].all() and not keep[[0, 1, 2, 3, 6, 8, 10]].any() and math.isnan(p[0])
    assert dropped["other_code"] == 2 and dropped["no_call"] == 1 and p[4] == 0.05 and p[9] == 0.5
    assert np.allclose(tab[9], [-math.sqrt(2.0), math.sqrt(2.0), 0.0, 0.0], rtol=0, atol=4e-16)      # (1 / sqrt(0.5) is rounded twice)
    # a kept row has mean 0; a row of homozygous calls only (inbred lines) has twice the Hardy-Weinberg variance the divisor assumes
    t = twin.values(snps[[4]], tab[[4]])
    assert abs(t.sum()) < 1e-12 and abs((t ** 2).sum() / 20 - 2.0) < 1e-12
    # the [1, rows, 4] array of site_counts itself is taken as well
    assert np.array_equal(pca.standardise(sitestats_twin.site_counts(snps), 20)[0], keep)


def test_decompose_order_sign_and_explained_share():
    rng = np.random.default_rng(3)
    z = rng.normal(size=(50, 12))
    gram = z.T @ z
    w, v, explained, trace = pca.decompose(gram, 50, 5)
    assert w.shape == (5,) and v.shape == (12, 5) and (np.diff(w) <= 0).all() and abs(trace - np.trace(gram) / 50) < 1e-12
    assert np.allclose(np.linalg.norm(v, axis=0), 1.0) and np.allclose((gram / 50) @ v, v * w, atol=1e-10)
    for c in range(5):
        assert v[np.argmax(np.abs(v[:, c])), c] > 0
    assert np.allclose(explained, w / trace) and explained.sum() <= 1.0 + 1e-12
    w_all, _, e_all, _ = pca.decompose(gram, 50, 12)
    assert abs(e_all.sum() - 1.0) < 1e-12 and np.allclose(w_all[:5], w)
    # a tie of the largest magnitude goes to the lowest index: (1, -1) / sqrt 2 is returned with its FIRST entry positive
    w2, v2, _, _ = pca.decompose(np.array([[2.0, -1.0], [-1.0, 2.0]]), 1, 2)
    assert np.allclose(w2, [3.0, 1.0]) and v2[0, 0] > 0 and v2[1, 0] < 0 and v2[0, 1] > 0
    for k in (0, 13):
        with pytest.raises(ValueError, match="components must be 1 .. 12"):
            pca.decompose(gram, 50, k)


class TwinGenotype(object):
    """the three scans of ``pca.analyse`` answered by the twins on a matrix in memory"""

    def __init__(self, snps):
        self.snps = np.asarray(snps)

    def site_counts(self, acc_ix=None, rows=None):
        return sitestats_twin.site_counts(self.snps, acc_ix, rows)

    def gram(self, tab, acc_ix=None, rows=None):
        return twin.gram(self.snps, tab, acc_ix, rows)

    def loadings(self, tab, vec, acc_ix=None, rows=None):
        return twin.loadings(self.snps, tab, vec, acc_ix, rows)


def _classes_of(snps_rows):
    """panel calls [rows, n] as sample classes [n, rows]"""
    v = np.asarray(snps_rows).T
    return np.where((v >= 0) & (v <= 2), v, pca.NO_CLASS).astype(np.uint8)


def test_project_reproduces_the_eigenvector_entries_of_panel_accessions():
    """every accession of the 36 x 600 planted panel through ``project`` with all rows matched lands on its own eigenvector entries:
    sum_s t(s, i) load[s][c] = (Z'Z v_c)_i = R lambda_c v_ic.  Entries are at most 1 in magnitude; 1e-12 absolute."""
    case = twin.planted_case(0)
    res = pca.analyse(TwinGenotype(case["snps"]), case["panel"], 36, np.arange(600), 0.05, 0.1, 10)
    assert res["vec"].shape == (36, 10) and res["load"].shape == (res["R"], 10) and 300 < res["R"] <= 600
    coord, n_sites = pca.project(_classes_of(case["snps"][res["rows"]][:, case["panel"]]), res["tab"], res["load"], res["eigenvalues"], res["R"])
    assert np.abs(coord - res["vec"]).max() <= 1e-12 and coord.shape == (36, 10)
    assert (n_sites <= res["R"]).all() and (n_sites > 0.9 * res["R"]).all() and n_sites.dtype == np.int64
    # a sample without a call is not placed; one with records at half of the rows is scaled by the rows it has
    none = np.full((1, res["R"]), pca.NO_CLASS, dtype=np.uint8)
    coord, n_sites = pca.project(none, res["tab"], res["load"], res["eigenvalues"], res["R"])
    assert np.isnan(coord).all() and n_sites.tolist() == [0]
    half = np.arange(res["R"]) % 2 == 0
    one = _classes_of(case["snps"][res["rows"]][:, case["panel"][:1]])
    coord, n_sites = pca.project(one, res["tab"], res["load"], res["eigenvalues"], res["R"], half)
    t = twin.values(case["snps"], res["tab"], case["panel"][:1], res["rows"])[:, 0]
    assert np.allclose(coord[0], (t[half] @ res["load"][half]) / (half.sum() * res["eigenvalues"]), rtol=0, atol=1e-12) and n_sites[0] <= half.sum()


def nearest_centroid(points, vec2, pop):
    """the population whose centroid over the first two components is nearest to each point"""
    names = sorted(set(pop.tolist()))
    cents = np.stack([vec2[pop == q].mean(axis=0) for q in names])
    d = ((np.asarray(points)[:, None, :] - cents[None, :, :]) ** 2).sum(axis=2)
    return [names[k] for k in np.argmin(d, axis=1).tolist()]


@pytest.mark.parametrize("seed", range(20))
def test_planted_populations_are_recovered(seed):
    """three Balding-Nichols populations (Fst 0.15) of 12 + 12 + 12 accessions through ``pca`` with the defaults: nearest centroid on
    PC1 and PC2 assigns all 36 to their population, and each held-out accession, projected from a random half of the rows used, lands
    nearest its own population's centroid.  The assignment is asserted; no distance threshold is set."""
    case = twin.planted_case(seed)
    res = pca.analyse(TwinGenotype(case["snps"]), case["panel"], 36, np.arange(600), 0.05, 0.1, 10)
    pop = case["pop"][case["panel"]]
    assert nearest_centroid(res["vec"][:, :2], res["vec"][:, :2], pop) == pop.tolist()
    half = np.random.default_rng(77 + seed).permutation(res["R"]) < res["R"] // 2
    coord, n_sites = pca.project(_classes_of(case["snps"][res["rows"]][:, case["held"]]), res["tab"], res["load"], res["eigenvalues"], res["R"], half)
    assert nearest_centroid(coord[:, :2], res["vec"][:, :2], pop) == case["pop"][case["held"]].tolist() and (n_sites > 0.4 * res["R"]).all()


# ------------------------------------------------------------------------------------------------ the library's validation
def test_refusals_that_need_no_device():
    lib = _lib.load()
    cols = np.zeros(3, dtype=np.int32)
    tab = np.zeros((5, 4))
    gram = np.zeros((3, 3))
    vec = np.zeros((3, 2))
    load = np.zeros((5, 2))
    bad = _lib.SNPM_ERR_BADARG

    def call_gram(ncols=3, n_rows=5, cols=cols, tab=tab, gram=gram):
        rc = lib.snpm_panel_gram(None, _lib.ptr(cols), ncols, None, 0, n_rows, _lib.ptr(tab), _lib.ptr(gram))
        return rc, lib.snpm_last_error(None).decode()

    def call_load(ncols=3, n_rows=5, cols=cols, tab=tab, vec=vec, k=2, load=load):
        rc = lib.snpm_panel_loadings(None, _lib.ptr(cols), ncols, None, 0, n_rows, _lib.ptr(tab), _lib.ptr(vec), k, _lib.ptr(load))
        return rc, lib.snpm_last_error(None).decode()
    for call in (call_gram, call_load):
        assert call(ncols=-1) == (bad, "negative size") and call(n_rows=-1) == (bad, "negative size")
        rc, msg = call(ncols=11553, cols=None)
        assert rc == bad and "too many accessions" in msg and "SNPM_PCA_MAX_ACCESSIONS" in msg
        rc, msg = call(n_rows=2 ** 31, tab=None)
        assert rc == bad and "2^31 rows" in msg
        assert call(tab=None)[0] == bad and "tab" in call(tab=None)[1] and "NULL" in call(tab=None)[1]
        for poison in (np.nan, np.inf, -np.inf):
            t = tab.copy()
            t[4, 3] = poison
            assert call(tab=t) == (bad, "tab holds a value that is not finite")
        assert call() == (bad, "panel is NULL") and call(ncols=0, cols=None) == (bad, "panel is NULL")
    assert call_gram(gram=None) == (bad, "gram is NULL") and call_gram(n_rows=0, tab=None) == (bad, "panel is NULL")
    assert call_gram(ncols=0, gram=None, tab=None) == (bad, "panel is NULL")
    for k in (0, -1, 33):
        assert call_load(k=k) == (bad, "k outside 1 .. SNPM_PCA_MAX_COMPONENTS")
    assert call_load(k=32, vec=np.zeros((3, 32)), load=np.zeros((5, 32))) == (bad, "panel is NULL")
    assert call_load(vec=None) == (bad, "vec is NULL") and call_load(load=None) == (bad, "tab / load is NULL")
    assert call_load(n_rows=0, tab=None, load=None) == (bad, "panel is NULL") and call_load(ncols=0, vec=None, tab=None, load=None) == (bad, "panel is NULL")
    v = vec.copy()
    v[2, 1] = np.nan
    assert call_load(vec=v) == (bad, "vec holds a value that is not finite")
    assert {"snpm_panel_gram", "snpm_panel_loadings"} <= set(_lib.SYMBOLS)


def test_header_constants_are_the_python_ones():
    text = open(os.path.join(host_kernel_util.ROOT, "include", "snpmatch_hip.h")).read()
    kernels = open(os.path.join(host_kernel_util.ROOT, "snpmatch_amd", "csrc", "snpm_k_pca.hpp")).read()
    for src in (text, kernels):
        assert int(re.search(r"#define SNPM_PCA_MAX_ACCESSIONS (\d+)", src).group(1)) == engine.PCA_MAX_ACCESSIONS == engine.KIN_MAX_ACCESSIONS
        assert int(re.search(r"#define SNPM_PCA_MAX_COMPONENTS (\d+)", src).group(1)) == engine.PCA_MAX_COMPONENTS == pca.MAX_COMPONENTS == 32
    assert pca.NO_CLASS == engine.F1X_NO_CLASS


def test_group_and_streamed_panels_are_refused_with_the_reason():
    for cls, why in ((engine.GroupPanel, "spread over several GPUs"), (engine.StreamedPanel, "not a resident panel")):
        for name, call in (("gram", lambda p: engine.gram(p, np.zeros((0, 4)))), ("loadings", lambda p: engine.loadings(p, np.zeros((0, 4)), np.zeros((0, 1))))):
            with pytest.raises(TypeError, match="%s needs every accession column on one device" % name) as err:
                call(cls.__new__(cls))
            assert why in str(err.value)


# ------------------------------------------------------------------------------------------------ the command
PLANTED_COMMAND_SEED = 0


def write_planted_inputs(case, tmp_path):
    """db.npz (all 39 accessions), pops.tsv (the 36 of the panel), accs.txt (the same without populations) and held.vcf: the three
    held-out accessions as samples with records at every second DB row, and a fourth sample without a call"""
    db, pops, accs, vcf = (str(tmp_path / n) for n in ("db.npz", "pops.tsv", "accs.txt", "held.vcf"))
    np.savez(db, snps=case["snps"], accessions=case["names"], positions=case["positions"], chrs=case["chrs"], chr_regions=case["chr_regions"])
    with open(pops, "w") as fh:
        fh.write("# accession population\n")
        for a in case["panel"].tolist():
            fh.write("%s\t%s\n" % (case["names"][a], case["pop"][a]))
    with open(accs, "w") as fh:
        fh.write("".join("%s\n" % case["names"][a] for a in case["panel"].tolist()))
    chr_of = np.repeat(case["chrs"], np.diff(case["chr_regions"], axis=1).reshape(-1))
    text = {-1: "./.", 0: "0/0", 1: "1/1", 2: "0/1"}
    with open(vcf, "w") as fh:
        fh.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(case["names"][case["held"]].tolist()) + "\tblank\n")
        for r in range(0, 600, 2):
            fh.write("%s\t%d\t.\tA\tT\t.\tPASS\t.\tGT\t%s\t./.\n" % (chr_of[r], case["positions"][r], "\t".join(text[int(v)] for v in case["snps"][r, case["held"]])))
    return db, pops, accs, vcf


def _tsv(path):
    return [ln.split("\t") for ln in open(path).read().splitlines()]


def check_planted_outputs(case, out, k=10, with_pops=True, with_projection=True):
    """what both command tests (the twin here, the device in test_gpu_pca.py) ask of the files of a run on the 36 panel accessions"""
    names, pop = case["names"][case["panel"]].tolist(), case["pop"][case["panel"]]
    lines = _tsv(out + ".pca.tsv")
    assert lines[0] == ["accession"] + (["population"] if with_pops else []) + ["PC%d" % (c + 1) for c in range(k)]
    assert [ln[0] for ln in lines[1:]] == names and (not with_pops or [ln[1] for ln in lines[1:]] == pop.tolist())
    z = np.load(out + ".pca.npz")
    assert set(z.files) >= {"accessions", "populations", "eigenvalues", "explained", "eigenvectors", "chr", "pos", "p", "table", "loadings"}
    vec, R = z["eigenvectors"], len(z["pos"])
    assert vec.shape == (36, k) and np.array_equal(np.array([[float(x) for x in ln[-k:]] for ln in lines[1:]]), vec)
    assert z["accessions"].tolist() == names and z["populations"].tolist() == (pop.tolist() if with_pops else [])
    assert z["loadings"].shape == (R, k) and z["table"].shape == (R, 4) and z["p"].shape == (R,) and z["chr"].shape == (R,)
    stats = json.load(open(out + ".pca.json"))
    assert set(stats) >= {"min_maf", "max_missing", "components", "populations", "bed", "sites", "accessions", "rows_selected", "rows_used", "rows_dropped",
                          "trace", "eigenvalues", "explained", "top_loadings"}
    assert stats["rows_used"] == R and stats["accessions"] == 36 and stats["components"] == k and set(stats["rows_dropped"]) == set(pca.DROP_RULES)
    assert stats["rows_selected"] == R + sum(stats["rows_dropped"].values()) and np.allclose(stats["eigenvalues"], z["eigenvalues"], rtol=1e-15)
    assert (np.diff(z["eigenvalues"]) <= 0).all() and sum(stats["explained"]) <= 1.0 + 1e-12 and np.allclose(z["explained"], z["eigenvalues"] / stats["trace"])
    assert len(stats["top_loadings"]) == k and all(len(t) == min(10, R) for t in stats["top_loadings"])
    top = stats["top_loadings"][0][0]
    at = int(np.argmax(np.abs(z["loadings"][:, 0])))
    assert (top["chr"], top["pos"], top["loading"]) == (str(z["chr"][at]), int(z["pos"][at]), float(z["loadings"][at, 0]))
    # the rows used are those standardise keeps, the table is its table, and the vectors are eigenvectors of the twin's matrix
    where = {(str(c), int(p)): r for r, (c, p) in enumerate(zip(np.repeat(case["chrs"], np.diff(case["chr_regions"], axis=1).reshape(-1)), case["positions"]))}
    rows = np.array([where[(str(c), int(p))] for c, p in zip(z["chr"], z["pos"])])
    t = twin.values(case["snps"], z["table"], case["panel"], rows)
    assert np.allclose((t.T @ t / R) @ vec, vec * z["eigenvalues"], rtol=0, atol=1e-9) and np.allclose(t @ vec, z["loadings"], rtol=0, atol=1e-9)
    if with_pops and k >= 2:
        assert nearest_centroid(vec[:, :2], vec[:, :2], pop) == pop.tolist()
    if with_projection:
        proj = _tsv(out + ".projection.tsv")
        assert proj[0] == ["sample", "n_sites"] + ["PC%d" % (c + 1) for c in range(k)] + ["nearest_1", "nearest_2", "nearest_3"] + (["population"] if with_pops else [])
        assert [ln[0] for ln in proj[1:]] == case["names"][case["held"]].tolist() + ["blank"]
        assert proj[4][1] == "0" and set(proj[4][2:]) == {"NA"} and len(proj[4]) == len(proj[0])
        for ln, a in zip(proj[1:4], case["held"].tolist()):
            assert 0.35 * R < int(ln[1]) <= 0.6 * R and all(n in names for n in ln[k + 2:k + 5]) and len(set(ln[k + 2:k + 5])) == 3
            if with_pops:
                assert ln[-1] == case["pop"][a]
                assert nearest_centroid(np.array([[float(ln[2]), float(ln[3])]]), vec[:, :2], pop) == [case["pop"][a]]
    return stats, z


@pytest.fixture
def planted(monkeypatch, tmp_path):
    """the planted DB as an .npz; the three device calls are the twins"""
    case = twin.planted_case(PLANTED_COMMAND_SEED)
    snps = case["snps"]
    calls = []
    stub = engine.Panel.__new__(engine.Panel)
    stub.h = None

    def gram(panel, tab, cols=None, rows=None):
        calls.append(("gram", cols, rows))
        return twin.gram(snps, tab, cols, rows)

    def loadings(panel, tab, vec, cols=None, rows=None):
        calls.append(("loadings", cols, rows))
        return twin.loadings(snps, tab, vec, cols, rows)
    monkeypatch.setattr(snp_genotype.Genotype, "panel", lambda self, ctx=None, packed=None: stub)
    monkeypatch.setattr(engine, "site_counts", lambda panel, groups=None, rows=None: sitestats_twin.site_counts(snps, groups, rows))
    monkeypatch.setattr(engine, "gram", gram)
    monkeypatch.setattr(engine, "loadings", loadings)
    return (case,) + write_planted_inputs(case, tmp_path) + (calls,)


def test_command_on_the_planted_panel(planted, tmp_path):
    case, db, pops, accs, vcf, calls = planted
    out = str(tmp_path / "out")
    assert cli.main(["pca", "-d", db, "--pops", pops, "-i", vcf, "-o", out]) == 0
    stats, z = check_planted_outputs(case, out)
    assert [c[0] for c in calls] == ["gram", "loadings"] and np.array_equal(calls[0][1], case["panel"]) and np.array_equal(calls[0][2], calls[1][2])
    assert (stats["min_maf"], stats["max_missing"], stats["populations"], stats["rows_selected"]) == (0.05, 0.1, ["pop0", "pop1", "pop2"], 600)
    assert "grm" not in z.files and stats["rows_dropped"]["other_code"] == 0 and stats["rows_dropped"]["maf"] > 0
    # -a, --keep_grm, fewer components, no samples: no population column, no projection file of this run
    out2 = str(tmp_path / "out2")
    assert cli.main(["pca", "-d", db, "-a", accs, "--components", "3", "--keep_grm", "-o", out2]) == 0
    stats2, z2 = check_planted_outputs(case, out2, k=3, with_pops=False, with_projection=False)
    assert not os.path.exists(out2 + ".projection.tsv") and np.allclose(z2["eigenvectors"], z["eigenvectors"][:, :3], rtol=0, atol=1e-9)
    assert z2["grm"].shape == (36, 36) and np.array_equal(z2["grm"], z2["grm"].T) and abs(np.trace(z2["grm"]) - stats2["trace"]) < 1e-9
    # --bed: the rows of a region, as a dense range; --sites: the listed rows
    assert cli.main(["pca", "-d", db, "--pops", pops, "--bed", "Chr2,1,100000", "-o", out2]) == 0
    z3 = np.load(out2 + ".pca.npz")
    assert set(z3["chr"].tolist()) == {"Chr2"} and z3["pos"].max() < 100000 and json.load(open(out2 + ".pca.json"))["rows_selected"] == 100
    sites = str(tmp_path / "x.pruned.tsv")
    with open(sites, "w") as fh:
        fh.write("chr\tpos\n" + "".join("%s\t%d\n" % (c, p) for c, p in list(zip(z["chr"], z["pos"]))[::2]))
    assert cli.main(["pca", "-d", db, "--pops", pops, "--sites", sites, "--min_maf", "0", "--max_missing", "1", "-o", out2]) == 0
    z4 = np.load(out2 + ".pca.npz")
    assert z4["pos"].tolist() == z["pos"][::2].tolist() and z4["chr"].tolist() == z["chr"][::2].tolist()
    # all accessions of the DB: the held-out ones are part of the analysis
    assert cli.main(["pca", "-d", db, "--components", "2", "-o", out2]) == 0 and len(np.load(out2 + ".pca.npz")["accessions"]) == 39 and calls[-1][1] is None
    # refusals: exit code 2, and the device is not asked for a matrix
    asked = len(calls)
    one = tmp_path / "one.txt"
    one.write_text("%s\n" % case["names"][0])
    twice = tmp_path / "twice.txt"
    twice.write_text("%s\n%s\n" % (case["names"][0], case["names"][0]))
    for bad in (["-a", str(one)], ["-a", str(twice)], ["--components", "0"], ["--components", "33"], ["-a", accs, "--components", "37"], ["--min_maf", "0.6"],
                ["--max_missing", "-0.1"], ["--bed", "Chr1,1,1000", "--sites", sites], ["--pops", pops, "-a", accs], ["--min_maf", "0.5", "--bed", "Chr1,1,5000"]):
        assert cli.main(["pca", "-d", db, "-o", out2] + bad) == 2, bad
    assert len(calls) == asked and pca.potatoPCA.__doc__
    args = cli.get_options("d", "v").parse_args(["pca", "-d", "db.snpm", "-o", "out"])
    assert (args.min_maf, args.max_missing, args.components, args.keep_grm, args.inFile) == (0.05, 0.1, 10, False, None)


# ------------------------------------------------------------------------------------------------ the kernels, on the host
def test_kernel_source_on_the_host_under_asan_and_ubsan(tmp_path):
    """every block of k_win_planes / k_pca_gram / k_pca_fold / k_pca_load run by 256 real threads with a barrier and the exchanges of a
    wave, exact-size heap buffers, arbitrary pad bytes, stale workspaces, integer tables against a plain loop (exact): the widths
    around a tile of 64, the row counts around a word, a pass of 32 rows and a plane step of 1024; column and row lists with repeats;
    a dense range with row0 > 0; rows that are all missing; code 3 with its own value; three slabs with a partial last one; k of 1,
    2, 10 and 32"""
    cases = host_kernel_util.run_driver("pca_host_driver", tmp_path)
    field = lambda ln, k: next(f.split("=")[1] for f in ln.split() if f.startswith(k + "="))      # noqa: E731
    grid = [ln for ln in cases if ln.split()[1] == "grid"]
    assert {int(field(ln, "cols")) for ln in grid} == {1, 2, 31, 32, 33, 63, 64, 65, 129, 130}
    assert {int(field(ln, "rows")) for ln in grid} == {1, 63, 64, 65, 1023, 1024, 1025, 2500}
    assert {field(ln, "layout") for ln in grid} == {"0", "1", "2"} and {field(ln, "k") for ln in cases if "k=" in ln} >= {"1", "2", "10", "32"}
    by_name = {ln.split()[1]: ln for ln in cases}
    assert int(field(by_name["three-slabs"], "slabs")) == 3 and int(field(by_name["three-slabs"], "rows")) % 1024 != 0
    assert {"lists", "lists-packed", "row0", "all-missing", "code3", "split-wide", "plan-one-step", "plan-splits"} <= set(by_name)
