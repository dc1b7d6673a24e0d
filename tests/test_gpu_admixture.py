"""admixture on the device: ``snpm_panel_admix`` (``k_adm_rows`` + ``k_adm_cols`` + ``k_adm_fold``) against the numpy twin evaluated in
long double (tests/admixture_twin.py) on panels filled through the normal upload path in each of the three layouts (int8, packed whole
rows, packed split rows).  The bounds are the issue's, derived from the roundings of the sums and not from what the device gives: every
entry of F' within (ncols + 64) 2^-52 relative, every entry of Q' within (n_rows + 64) 2^-52 relative, |ll - ref| <= 2^-52 ((K + 2)
cells + (ceil(ncols / 64) + 64) |ref|).  The shapes are those where the decomposition could break: 64 lanes per wave and 256 columns per
block of ``k_adm_cols``, 8 rows per wave and 32 per block of ``k_adm_rows``, 16 rows per chunk and per shortest split, the row count at
which the splits stop growing in number and start growing in length (512 / column blocks x 16), every step of K (4 / 8 / 16).  Every
reference is computed once per width and shared by the three layouts."""
import functools

import numpy as np
import pytest

import admixture_twin as twin
import test_admixture_cpu as cpu
import test_pca_cpu as pca_cpu
from snpmatch_amd import _lib, cli, engine

pytestmark = pytest.mark.gpu

LAYOUTS = ["int8", "packed", "split"]
KERNELS = ("adm_rows", "adm_cols", "adm_fold")
WIDTHS = [1, 2, 63, 64, 65, 129, 130, 255, 256, 257]
BASE_ROWS = [1, 63, 64, 65, 1023, 1025, 2500]
KS = [1, 2, 3, 4, 5, 8, 9, 16]
FLAGS = [3, 1, 2, 0]
COLS_THREADS, BLOCKS_WANTED, SPLIT_MIN_ROWS = 256, 512, 16      # ADM_COLS_THREADS, ADM_BLOCKS_WANTED, ADM_SPLIT_MIN_ROWS of csrc/snpm_k_adm.hpp
ROW0 = 3


@pytest.fixture(scope="module")
def ctx():
    return engine.default_context()


def _calls(rng, n_rows, n_acc, other=False):
    v = rng.choice(np.array([-1, 0, 1, 2], dtype=np.int8), size=(n_rows, n_acc), p=[0.12, 0.45, 0.35, 0.08])
    if other:
        v[rng.random((n_rows, n_acc)) < 0.05] = 3
    return v


def _panel(ctx, snps, layout, monkeypatch):
    """the normal upload path; packed panels are split (main part + ragged tail) wherever that saves memory, SNPM_PACKED_SPLIT=0
    keeps whole rows"""
    if layout == "packed":
        monkeypatch.setenv("SNPM_PACKED_SPLIT", "0")
    panel = engine.Panel.from_host(ctx, snps, packed=layout != "int8")
    monkeypatch.delenv("SNPM_PACKED_SPLIT", raising=False)
    return panel


def _start(rng, n, R, K):
    """a valid pair with entries of F at both clamps and a zero entry of Q now and then"""
    Q, F = twin.random_start(rng, n, R, K)
    edge = rng.random(F.shape)
    F[edge < 0.03] = twin.EPS
    F[edge > 0.97] = twin.ONE_MINUS_EPS
    if K > 1:
        Q[::7, 0] = 0.0
        Q /= Q.sum(axis=1, keepdims=True)
    return Q, F


def _reference(snps, Q, F, cols, rows, flags):
    ref = twin.step(snps, Q, F, cols, rows, bool(flags & 2), bool(flags & 1), dtype=np.longdouble)
    for a in ref[:2]:
        a.setflags(write=False)
    return ref


def _check(panel, snps, Q, F, ref, cols, rows, flags, what):
    """one iteration on the device within the bounds of ``ref``; a component that is not updated keeps its bits"""
    Qn, Fn, ll = engine.admix(panel, Q, F, 1, cols, rows, update_q=bool(flags & 2), update_f=bool(flags & 1))
    assert Qn.dtype == Fn.dtype == ll.dtype == np.float64 and Qn.shape == Q.shape and Fn.shape == F.shape and ll.shape == (1,)
    assert (flags & 2) or np.array_equal(Qn, Q)
    assert (flags & 1) or np.array_equal(Fn, F)
    ratios = twin.worst_ratios((Qn, Fn, ll[0]), ref, snps, cols, rows)
    print("%s: worst error / bound F %.4f Q %.4f ll %.4f" % ((what,) + ratios))
    assert max(ratios) <= 1.0, (what, ratios)
    assert (np.abs(Qn.sum(axis=1) - 1.0) <= Q.shape[1] * twin.U52).all() and (Fn >= twin.EPS).all() and (Fn <= twin.ONE_MINUS_EPS).all()
    return Qn, Fn, ll


# ------------------------------------------------------------------------------------------------ one iteration at every edge
def _row_counts(n_acc):
    """the base list, the shortest split, and the row counts around the one where ``k_adm_cols`` has all the splits it wants"""
    wanted = -(-BLOCKS_WANTED // -(-n_acc // COLS_THREADS))
    edge = wanted * SPLIT_MIN_ROWS
    return BASE_ROWS + [15, 16, 17, edge - 1, edge, edge + 1]


@functools.lru_cache(maxsize=None)
def _grid_case(n_acc):
    """the panel of a width and, per row count, (n_rows, K, flags, Q, F, long-double reference): computed once, read-only"""
    rng = np.random.default_rng(1000 + n_acc)
    counts = _row_counts(n_acc)
    snps = _calls(rng, max(counts) + ROW0 + 2, n_acc)
    snps.setflags(write=False)
    items = []
    for at, n_rows in enumerate(counts):
        shift = at + WIDTHS.index(n_acc)
        K = 2 if n_rows > 4000 else KS[shift % len(KS)]              # (the long rows keep the long-double reference cheap)
        flags = FLAGS[shift % len(FLAGS)]
        Q, F = _start(rng, n_acc, n_rows, K)
        items.append((n_rows, K, flags, Q, F, _reference(snps, Q, F, None, range(ROW0, ROW0 + n_rows), flags)))
    return snps, items


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n_acc", WIDTHS)
def test_one_iteration_at_every_edge_of_width_rows_and_k(n_acc, layout, ctx, monkeypatch):
    snps, items = _grid_case(n_acc)
    panel = _panel(ctx, snps, layout, monkeypatch)
    for n_rows, K, flags, Q, F, ref in items:
        _check(panel, snps, Q, F, ref, None, range(ROW0, ROW0 + n_rows), flags, "grid acc=%d rows=%d K=%d flags=%d %s" % (n_acc, n_rows, K, flags, layout))
    panel.free()


def test_the_grid_covers_every_k_and_flag_with_every_layout():
    seen = set()
    for n_acc in WIDTHS:
        for at, n_rows in enumerate(_row_counts(n_acc)):
            shift = at + WIDTHS.index(n_acc)
            seen.add((2 if n_rows > 4000 else KS[shift % len(KS)], FLAGS[shift % len(FLAGS)]))
    assert {k for k, _ in seen} == set(KS) and {f for _, f in seen} == set(FLAGS)
    assert _row_counts(256)[-3:] == [8191, 8192, 8193] and _row_counts(257)[-3:] == [4095, 4096, 4097]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("K", KS)
def test_every_k_with_both_updates(K, layout, ctx, monkeypatch):
    rng = np.random.default_rng(1500 + K)
    snps = _calls(rng, 300, 70)
    panel = _panel(ctx, snps, layout, monkeypatch)
    Q, F = _start(rng, 70, 300, K)
    _check(panel, snps, Q, F, _reference(snps, Q, F, None, None, 3), None, None, 3, "K=%d %s" % (K, layout))
    panel.free()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_lists_ranges_missing_rows_and_columns_and_the_other_code(layout, ctx, monkeypatch):
    rng = np.random.default_rng(2000)
    snps = _calls(rng, 400, 90, other=layout == "int8")
    snps[100:180] = -1                                              # rows that are all missing
    snps[:, 40] = -1                                                # a column that is all missing
    panel = _panel(ctx, snps, layout, monkeypatch)
    cols = np.arange(89, 20, -1)                                    # descending, with repeats
    cols[5], cols[-1] = cols[4], cols[0]
    rows = rng.integers(0, 400, size=333)                           # unsorted, with repeats
    rows[7] = rows[6]
    for K, c, r in ((5, cols, None), (2, None, rows), (16, cols, rows), (3, None, range(57, 400)), (9, None, None)):
        n, R = (90 if c is None else len(c)), (400 if r is None else len(r))
        Q, F = _start(rng, n, R, K)
        Qn, Fn, _ = _check(panel, snps, Q, F, _reference(snps, Q, F, c, r, 3), c, r, 3, "lists K=%d %s" % (K, layout))
        g, called = twin.dosage(snps, c, r)
        blank_rows, blank_cols = ~called.any(axis=1), ~called.any(axis=0)
        assert np.array_equal(Fn[blank_rows], F[blank_rows]) and np.array_equal(Qn[blank_cols], Q[blank_cols])      # unchanged, bit for bit
    if layout == "int8":                                            # the "other" code is no call: the same results with those calls missing
        assert (snps == 3).sum() > 1000
        Q, F = _start(rng, 90, 400, 4)
        plain = np.where(snps == 3, -1, snps).astype(np.int8)
        other = engine.Panel.from_host(ctx, plain, packed=False)
        for a, b in zip(engine.admix(panel, Q, F, 2), engine.admix(other, Q, F, 2)):
            assert np.array_equal(a, b)
        other.free()
    # calls that do no work
    Q, F = _start(rng, 90, 0, 3)
    Q0, F0, ll0 = engine.admix(panel, Q, F, 4, rows=range(5, 5))
    assert np.array_equal(Q0, Q) and F0.shape == (0, 3) and ll0.tolist() == [0.0] * 4
    Qe, Fe, lle = engine.admix(panel, np.zeros((0, 3)), np.full((400, 3), 0.5), 2, cols=[])
    assert Qe.shape == (0, 3) and np.array_equal(Fe, np.full((400, 3), 0.5)) and lle.tolist() == [0.0, 0.0]
    panel.free()


# ------------------------------------------------------------------------------------------------ the realistic width
@functools.lru_cache(maxsize=None)
def _wide_case():
    rng = np.random.default_rng(3000)
    snps = _calls(rng, 3000, 1135)
    Q, F = _start(rng, 1135, 3000, 8)
    for a in (snps, Q, F):
        a.setflags(write=False)
    return snps, Q, F, _reference(snps, Q, F, None, None, 3)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_realistic_width(layout, ctx, monkeypatch):
    """1135 accessions x 3000 rows, K = 8, both updates, one iteration: five column blocks, 103 splits of 30 rows"""
    snps, Q, F, ref = _wide_case()
    panel = _panel(ctx, snps, layout, monkeypatch)
    _check(panel, snps, Q, F, ref, None, None, 3, "wide %s" % layout)
    panel.free()


# ------------------------------------------------------------------------------------------------ determinism and state
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("K", [3, 8, 16])
def test_same_bits_chained_calls_and_evaluation(K, layout, ctx, monkeypatch):
    rng = np.random.default_rng(4000 + K)
    snps = _calls(rng, 1500, 300)
    panel = _panel(ctx, snps, layout, monkeypatch)
    Q, F = _start(rng, 300, 1500, K)
    keep = Q.copy(), F.copy()
    first = engine.admix(panel, Q, F, 3)
    assert np.array_equal(Q, keep[0]) and np.array_equal(F, keep[1])      # the inputs are not written
    for a, b in zip(first, engine.admix(panel, Q, F, 3)):            # the same call twice: the same bits
        assert np.array_equal(a, b)
    Qc, Fc, trace = Q, F, []
    for _ in range(3):                                               # three chained calls of one iteration: the same bits
        Qc, Fc, ll = engine.admix(panel, Qc, Fc, 1)
        trace.append(ll[0])
    assert np.array_equal(Qc, first[0]) and np.array_equal(Fc, first[1]) and np.array_equal(np.array(trace), first[2]) and (np.diff(first[2]) > 0).all()
    # evaluation only: Q and F come back bit for bit, with the likelihood a both-updates call reports for the same input
    Q0, F0, ll0 = engine.admix(panel, Q, F, 1, update_q=False, update_f=False)
    assert np.array_equal(Q0, Q) and np.array_equal(F0, F) and ll0[0] == first[2][0]
    ll2 = engine.admix(panel, Q, F, 2, update_q=False, update_f=False)[2]
    assert ll2[0] == ll2[1] == ll0[0]
    # one component alone: the other keeps its bits through every iteration, the updated one is the both-updates result of iteration 1
    Qf, Ff, llf = engine.admix(panel, Q, F, 2, update_q=False)
    assert np.array_equal(Qf, Q) and llf[0] == ll0[0] and llf[1] > llf[0]
    Qq, Fq, llq = engine.admix(panel, Q, F, 2, update_f=False)
    assert np.array_equal(Fq, F) and llq[0] == ll0[0] and llq[1] > llq[0]
    one = engine.admix(panel, Q, F, 1)
    assert np.array_equal(engine.admix(panel, Q, F, 1, update_q=False)[1], one[1]) and np.array_equal(engine.admix(panel, Q, F, 1, update_f=False)[0], one[0])
    panel.free()


# ------------------------------------------------------------------------------------------------ the command
def test_command_end_to_end_on_the_planted_panel(ctx, tmp_path):
    """the assertions of the CPU test of the planted panel, with the device in the twin's place: the likelihood rises at each of the 300
    iterations, every pure accession has its largest share, at least 0.5, on its own population"""
    case = twin.planted_case(cpu.PLANTED_COMMAND_SEED)
    db, pops, accs, vcf = pca_cpu.write_planted_inputs(case, tmp_path)
    out = str(tmp_path / "out")
    assert cli.main(["admixture", "-d", db, "-K", "3", "--seed", str(cpu.PLANTED_COMMAND_SEED), "--max_iter", str(cpu.PLANTED_ITERATIONS), "--tol", "0",
                     "--pops", pops, "-i", vcf, "-o", out]) == 0
    cpu.check_planted_outputs(case, out)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_that_need_a_panel_launch_nothing(ctx):
    snps = _calls(np.random.default_rng(6000), 50, 20)
    panel = engine.Panel.from_host(ctx, snps, packed=False)
    Q, F = twin.random_start(np.random.default_rng(6001), 20, 50, 3)
    ctx.profile(True)
    ctx.profile_reset()
    try:
        def refused(call, text):
            with pytest.raises(AssertionError) as err:         # (SNPM_ERR_BADARG: ``_lib.check`` raises it as the reference's assert)
                call()
            assert text in str(err.value), str(err.value)
        refused(lambda: engine.admix(panel, Q[:2], F[:2], cols=[0, 20], rows=range(0, 2)), "accession index outside the panel")
        refused(lambda: engine.admix(panel, Q[:1], F[:2], cols=[-1], rows=range(0, 2)), "accession index outside the panel")
        refused(lambda: engine.admix(panel, Q, F[:2], rows=np.array([0, 50])), "row index outside the panel")
        refused(lambda: engine.admix(panel, Q, F[:2], rows=np.array([-1, 5])), "row index outside the panel")
        refused(lambda: engine.admix(panel, Q, F, rows=range(1, 51)), "row range outside the panel")
        ll = np.zeros(1)
        rc = ctx.lib.snpm_panel_admix(panel.h, None, 19, None, 0, 50, 3, 1, 3, _lib.ptr(Q[:19].copy()), _lib.ptr(F.copy()), _lib.ptr(ll))
        assert rc == _lib.SNPM_ERR_BADARG and "cols is NULL (all accessions)" in ctx.lib.snpm_last_error(ctx.h).decode()
        q = Q.copy()
        q[19, 2] = np.nan
        refused(lambda: engine.admix(panel, q, F), "Q holds an entry that is not finite or is negative")
        q = Q.copy()
        q[19, 2] += 1e-6
        refused(lambda: engine.admix(panel, q, F), "a row of Q does not sum to 1")
        for poison in (np.nan, 0.0, 1.0):
            f = F.copy()
            f[49, 2] = poison
            refused(lambda: engine.admix(panel, Q, f), "F holds an entry outside")
        refused(lambda: engine.admix(panel, Q, F, 0), "n_iter outside 1 .. 10000")
        refused(lambda: engine.admix(panel, np.full((20, 17), 1.0 / 17), np.full((50, 17), 0.5)), "K outside 1 .. SNPM_ADMIX_MAX_K")
        assert [ctx.profile_read(name)[0] for name in KERNELS] == [0, 0, 0]
        # ... and sound calls do launch: rows and fold per iteration, cols with the update of Q
        engine.admix(panel, Q, F, 3)
        assert [ctx.profile_read(name)[0] for name in KERNELS] == [3, 3, 3]
        engine.admix(panel, Q, F, 2, update_q=False)
        engine.admix(panel, Q, F, 1, update_q=False, update_f=False)
        assert [ctx.profile_read(name)[0] for name in KERNELS] == [6, 3, 6]
    finally:
        ctx.profile(False)
        panel.free()


def test_group_and_streamed_panels_are_refused_with_the_reason():
    cpu.test_group_and_streamed_panels_are_refused_with_the_reason()
