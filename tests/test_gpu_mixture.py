"""mixture on the device: ``snpm_panel_mix_counts`` / ``k_win_planes`` + ``k_mix_count<2 / 4 / 8>`` against the numpy twin
(tests/mixture_twin.py), cell by cell and without a tolerance, on panels filled through the normal upload path in each of the three
layouts (int8, packed whole rows, packed split rows), at the shapes where the decomposition could break: the accessions per tile side
of the count kernel (a 2 x 2 register tile of pairs per lane; the plane kernel works on 64 accessions x 64 rows), 64 rows per word,
the rows per LDS step and per chunk, the largest count at which the number of bit slices changes, slabs of the row axis;
``Genotype.mix_counts``; and the ``mixture`` command end to end on the planted pool, byte for byte what the twin-backed run writes."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mixture_twin
from snpmatch_amd import cli, engine
from snpmatch_amd.core import snp_genotype

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = ["int8", "packed", "split"]


def _kernel_constant(name):
    """a ``constexpr int`` of csrc/snpm_k_mix.hpp"""
    text = open(os.path.join(os.path.dirname(os.path.abspath(engine.__file__)), "csrc", "snpm_k_mix.hpp")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


TILE = _kernel_constant("MIX_TILE")                       # accessions per tile side of k_mix_count
CHUNK = _kernel_constant("MIX_CHUNK_WORDS") * 64          # rows per block of k_mix_count
STEP = _kernel_constant("MIX_STEP_WORDS") * 64            # rows per LDS step


@pytest.fixture(scope="module")
def ctx():
    return engine.default_context()


def _calls(rng, n_rows, n_acc, other=False):
    v = rng.choice(np.array([-1, 0, 1, 2], dtype=np.int8), size=(n_rows, n_acc), p=[0.12, 0.45, 0.35, 0.08])
    if other:
        v[rng.random((n_rows, n_acc)) < 0.05] = 3
    return v


def _reads(rng, n, largest):
    """alt and ref counts 0 .. largest, a quarter of them 0, the largest present"""
    alt, ref = (np.where(rng.random(n) < 0.25, 0, rng.integers(0, largest + 1, n)).astype(np.uint8) for _ in range(2))
    if n:
        (alt if rng.random() < 0.5 else ref)[rng.integers(0, n)] = largest
    return alt, ref


def _panel(ctx, snps, layout, monkeypatch):
    """the normal upload path; packed panels are split (main part + ragged tail) wherever that saves memory, SNPM_PACKED_SPLIT=0
    keeps whole rows"""
    if layout == "packed":
        monkeypatch.setenv("SNPM_PACKED_SPLIT", "0")
    panel = engine.Panel.from_host(ctx, snps, packed=layout != "int8")
    monkeypatch.delenv("SNPM_PACKED_SPLIT", raising=False)
    return panel


def _check(panel, snps, alt, ref, cols=None, rows=None):
    got = engine.mix_counts(panel, alt, ref, cols, rows)
    want = mixture_twin.mix_counts(snps, alt, ref, cols, None if rows is None else (np.arange(rows.start, rows.stop) if isinstance(rows, range) else rows))
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want), "%d cells differ" % int((got != want).sum())
    assert np.array_equal(got, got.transpose(0, 2, 1, 4, 3))
    return got


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n_acc", [1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 130])
def test_tile_edges_of_accessions_and_words_of_rows(n_acc, layout, ctx, monkeypatch):
    rng = np.random.default_rng(1000 + n_acc)
    snps = _calls(rng, 70, n_acc, other=layout == "int8")
    assert layout != "int8" or (snps == 3).any()
    panel = _panel(ctx, snps, layout, monkeypatch)
    for k, n_rows in enumerate((1, 63, 64, 65)):
        _check(panel, snps, *_reads(rng, n_rows, (3, 15, 255, 15)[k]), rows=range(5, 5 + n_rows))
    _check(panel, snps, *_reads(rng, 70, 15))
    panel.free()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_step_and_chunk_of_the_count_kernel_minus_one_exact_plus_one(layout, ctx, monkeypatch):
    rng = np.random.default_rng(2000)
    snps = _calls(rng, CHUNK + 2, 33, other=layout == "int8")
    alt, ref = _reads(rng, CHUNK + 2, 15)
    panel = _panel(ctx, snps, layout, monkeypatch)
    for n_rows in (STEP - 1, STEP, STEP + 1, CHUNK - 1, CHUNK, CHUNK + 1):
        _check(panel, snps, alt[:n_rows], ref[:n_rows], rows=range(0, n_rows))
    _check(panel, snps, alt[:CHUNK], ref[:CHUNK], rows=range(2, CHUNK + 2))
    panel.free()


@pytest.mark.parametrize("largest", [3, 4, 15, 16, 255])
def test_largest_count_on_either_side_of_every_number_of_slices(largest, ctx, monkeypatch):
    rng = np.random.default_rng(2500 + largest)
    layout = LAYOUTS[largest % 3]
    snps = _calls(rng, STEP + 70, 33, other=layout == "int8")
    panel = _panel(ctx, snps, layout, monkeypatch)
    alt, ref = _reads(rng, len(snps), largest)
    assert max(alt.max(), ref.max()) == largest and ((alt == 0) & (ref == 0)).any()       # rows without a read among the others
    got = _check(panel, snps, alt, ref)
    assert got.max() > largest
    panel.free()


def test_all_counts_zero_and_one_row_at_255_among_zeros(ctx, monkeypatch):
    rng = np.random.default_rng(2700)
    snps = _calls(rng, STEP + 70, 33)
    snps[STEP + 3, :2] = [1, 0]
    panel = _panel(ctx, snps, "packed", monkeypatch)
    zero = np.zeros(len(snps), dtype=np.uint8)
    assert not _check(panel, snps, zero, zero).any()
    one = zero.copy()
    one[STEP + 3] = 255
    got = _check(panel, snps, one, zero)
    assert got[0, 1, 0, 0, 1] == 255 and got[0, 0, 1, 1, 0] == 255 and not got[1].any()
    got = _check(panel, snps, zero, one)
    assert got[1, 1, 0, 0, 1] == 255 and not got[0].any()
    panel.free()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_forms_of_rows_and_cols(layout, ctx, monkeypatch):
    rng = np.random.default_rng(4000)
    snps = _calls(rng, 1500, 70, other=layout == "int8")
    snps[:, 11] = -1                                                                  # a column without a call
    if layout == "int8":
        snps[:, 12] = 3                                                               # ... and one of "other" calls only
    panel = _panel(ctx, snps, layout, monkeypatch)
    alt, ref = _reads(rng, 1500, 15)
    whole = _check(panel, snps, alt, ref)                                             # rows None
    assert not whole[:, :, :, 11].any() and not whole[:, :, :, :, 11].any() and (layout != "int8" or not whole[:, :, :, 12].any())
    dense = _check(panel, snps, alt[:1100], ref[:1100], rows=range(200, 1300))
    listed = _check(panel, snps, alt[:1100], ref[:1100], rows=np.arange(200, 1300, dtype=np.int64))
    assert np.array_equal(dense, listed)
    rows = np.sort(rng.integers(0, 1500, size=1100).astype(np.int64))[::-1].copy()    # descending, with repeats
    assert (np.diff(rows) == 0).any() and (np.diff(rows) <= 0).all()
    cols = rng.permutation(70)[:41].astype(np.int32)
    cols[-1] = cols[3]
    got = _check(panel, snps, alt[:1100], ref[:1100], cols=cols, rows=rows)
    assert np.array_equal(got[:, :, :, -1], got[:, :, :, 3]) and np.array_equal(got[:, :, :, 3, -1], got[:, :, :, 3, 3])
    perm = rng.permutation(70).astype(np.int32)                                       # a permutation of all columns
    moved = _check(panel, snps, alt, ref, cols=perm)
    assert np.array_equal(moved, whole[:, :, :, perm][:, :, :, :, perm])
    panel.free()


def test_empty_calls_refusals_and_a_smaller_second_call(ctx, monkeypatch):
    rng = np.random.default_rng(6000)
    snps = _calls(rng, 3000, 130, other=True)
    big = _panel(ctx, snps, "int8", monkeypatch)
    _check(big, snps, *_reads(rng, 3000, 255))
    tiny = _calls(rng, 9, 3)
    small = _panel(ctx, tiny, "split", monkeypatch)
    _check(small, tiny, *_reads(rng, 9, 3))
    _check(big, snps, *_reads(rng, 1, 15), cols=np.array([5, 6], dtype=np.int32), rows=range(0, 1))
    none8 = np.zeros(0, dtype=np.uint8)
    empty = engine.mix_counts(big, none8, none8, cols=np.array([1, 2, 3], dtype=np.int32), rows=range(0, 0))      # n_rows == 0: zeros
    assert empty.shape == (2, 2, 2, 3, 3) and empty.dtype == np.int32 and not empty.any()
    nothing = engine.mix_counts(big, *_reads(rng, 3000, 3), cols=np.zeros(0, dtype=np.int32))                   # ncols == 0: nothing
    assert nothing.shape == (2, 2, 2, 0, 0)
    with pytest.raises(AssertionError, match="accession index outside the panel"):
        engine.mix_counts(big, *_reads(rng, 3000, 3), cols=np.array([0, 130], dtype=np.int32))
    with pytest.raises(AssertionError, match="row index outside the panel"):
        engine.mix_counts(big, *_reads(rng, 2, 3), rows=np.array([0, 3000], dtype=np.int64))
    with pytest.raises(AssertionError, match="row range outside the panel"):
        engine.mix_counts(big, *_reads(rng, 2, 3), rows=range(2999, 3001))
    big.free()
    small.free()


@pytest.mark.parametrize("layout", ["int8", "split"])
def test_three_slabs_equal_one_slab(layout, ctx, monkeypatch, tmp_path):
    """SNPM_MIX_WS_MB=1 in a fresh child process: 130 accessions are 192 padded columns, 96 KiB of planes per LDS step -- the budget
    holds 10 such steps, cut to one whole chunk per slab.  Two chunks and 1030 rows are three slabs, once as a range and once as a
    row list with repeats.  The budget changes the launches, not the sums: the same scans under the default budget are one slab
    each and give the same table; twelve of the columns are also compared with the twin."""
    step_bytes = 4 * 192 * (STEP // 64) * 8
    steps = (1 << 20) // step_bytes
    assert steps >= CHUNK // STEP and steps // (CHUNK // STEP) * (CHUNK // STEP) * STEP == CHUNK
    rng = np.random.default_rng(3000)
    snps = _calls(rng, 2 * CHUNK + 1030, 130, other=layout == "int8")
    alt, ref = _reads(rng, len(snps), 15)
    order = rng.integers(0, len(snps), size=2 * CHUNK + 5).astype(np.int64)
    order[-1] = order[0]
    alt_rows, ref_rows = _reads(rng, len(order), 255)
    np.savez(tmp_path / "in.npz", snps=snps, packed=layout != "int8", alt=alt, ref=ref, rows=order, alt_rows=alt_rows, ref_rows=ref_rows)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mix_slab_worker.py"), str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       capture_output=True, text=True, env=dict(os.environ, SNPM_MIX_WS_MB="1"), timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    z = np.load(tmp_path / "out.npz")
    assert z["launches"].tolist() == [[3, 3], [3, 3]]
    panel = _panel(ctx, snps, layout, monkeypatch)
    ctx.profile(True)
    ctx.profile_reset()
    once = engine.mix_counts(panel, alt, ref)
    assert ctx.profile_read("mix_count")[0] == 1 and ctx.profile_read("win_planes")[0] == 1
    ctx.profile(False)
    assert np.array_equal(z["range"], once)
    assert np.array_equal(z["list"], engine.mix_counts(panel, alt_rows, ref_rows, rows=order))
    few = np.array([0, 31, 32, 33, 63, 64, 65, 95, 96, 127, 128, 129])
    assert np.array_equal(once[:, :, :, few][:, :, :, :, few], mixture_twin.mix_counts(snps, alt, ref, few))
    assert np.array_equal(z["list"][:, :, :, few][:, :, :, :, few], mixture_twin.mix_counts(snps, alt_rows, ref_rows, few, order))
    panel.free()


def test_two_calls_on_the_same_inputs_return_the_same_bits(ctx, monkeypatch):
    rng = np.random.default_rng(7000)
    snps = _calls(rng, CHUNK + STEP + 5, 65)
    alt, ref = _reads(rng, len(snps), 255)
    panel = _panel(ctx, snps, "split", monkeypatch)
    first = engine.mix_counts(panel, alt, ref)
    assert np.array_equal(first, engine.mix_counts(panel, alt, ref)) and first.any()
    panel.free()


def test_genotype_method_and_the_command_end_to_end_on_the_planted_pool(ctx, tmp_path, monkeypatch):
    case = mixture_twin.planted_case(0.2)
    for d in ("twin", "device"):
        (tmp_path / d).mkdir()
    db, vcf = mixture_twin.write_planted(case, tmp_path)
    with monkeypatch.context() as patch:                 # the twin-backed run of tests/test_mixture_cpu.py
        calls = mixture_twin.install_twin(patch)
        assert cli.main(["mixture", "-i", vcf, "-d", db, "-o", str(tmp_path / "twin" / "out")]) == 0 and len(calls) == 1
    assert cli.main(["mixture", "-i", vcf, "-d", db, "-o", str(tmp_path / "device" / "out")]) == 0
    for ext in (".mixture.json", ".mixture.npz", ".mixture.scores.txt"):
        want, got = (open(str(tmp_path / d / "out") + ext, "rb").read() for d in ("twin", "device"))
        assert len(want) > 100 and got == want, ext
    g = snp_genotype.Genotype.from_arrays(case["snps"], case["names"], case["positions"], case["chrs"], case["chr_regions"])
    g.panel(ctx)
    rows = np.asarray(calls[0][1])
    keep = np.isin(case["pos"], case["positions"]) & (case["alt"] + case["ref"] > 0)
    alt, ref = case["alt"][keep], case["ref"][keep]
    assert len(rows) == len(alt)
    table = g.mix_counts(alt, ref, None, rows)
    assert np.array_equal(table, np.load(str(tmp_path / "device" / "out") + ".mixture.npz")["table"])
    sub = g.mix_counts(alt[40:200], ref[40:200], np.arange(40)[::-1], rows[40:200])
    assert np.array_equal(sub, mixture_twin.mix_counts(case["snps"], alt[40:200], ref[40:200], np.arange(40)[::-1], rows[40:200]))
    g.panel().free()
