"""The one device scratch of the resident-panel scans (``ws_scan``, snpmatch_amd/csrc/snpm_scratch.hpp): every scan of
tests/scan_cases.py lays its parts out in the same block, call after call, so a call finds there what ANY earlier scan left.  The
scans run here in sequences on one context -- each after each of its neighbours in table order and in reverse, each straight after
``ibd_counts`` and after ``marker_select`` (the two with the most and the largest parts), with and without the row and column
parts, and across a growth of the block -- and every result is checked with the scan's own ``check`` against its numpy twin: a part
read before the call wrote it, two parts that overlap or a block that moved under queued work changes counts, which are compared
exactly.

Two host panels, each once per layout.  NARROW, 2200 rows x 130 accessions (int8, packed whole rows, packed split rows: at 130
accessions a row of 0 + 64 bytes), with a shuffled list of 2100 rows and a list of 87 columns, a repeat in each.  Every
``SNPM_*_WS_MB`` is 1 when the contexts are made, but at this width 1 MiB of planes still holds 10 to 14 steps of 1024 rows (see
the slab tests of the per-scan files): every call on it is one slab.  So the order sequence also runs on WIDE, 2200 rows x 1135
accessions (rows of 1152, 512 and 256 + 32 bytes) with the same row list and a list of 1101 columns, one of them twice: 1152 padded
columns are 432 to 1008 KiB of planes per step, and a call of 2100 rows is 2 slabs to ``kinship_counts``, ``ld_band`` and
``mosaic`` (a chain per slab) and 3 to ``f1_counts``, ``mix_counts``, ``parent_counts``, ``ibd_counts``, ``sim_counts``, ``gram``
and ``window_counts`` -- the row part is uploaded again per slab, the parts are sized for the largest slab before the one commit,
the per-slab tables and cells are written again, all inside a block that holds another scan's leftovers.  (``site_counts`` and
``loadings`` would need 65 536 and about 16 000 rows to split at 1 MiB and stay one slab; ``marker_select`` and ``admix`` have no
slabs.)  ``ld_band`` refuses a repeated column: it gets the column list without its repeat.  The twins are computed once per
selection and shared by the layouts and by every place of a sequence (17 s on the host for WIDE, 11 of them the int64 twin of
``mix_counts``).

The last test is the one observable the shared block is meant to change: what six scans hold on the device after they returned."""

import numpy as np
import pytest

import scan_cases
from snpmatch_amd import engine

pytestmark = pytest.mark.gpu

N_ROWS, N_ACC, N_WIDE = 2200, 130, 1135
LAYOUTS = ["int8", "packed", "split"]
PITCH = {N_ACC: {"int8": 256, "packed": 256, "split": 64}, N_WIDE: {"int8": 1152, "packed": 512, "split": 256 + 32}}
BUDGETS = ["SNPM_%s_WS_MB" % k for k in ("SHARED", "KIN", "SITE", "LD", "WIN", "F1X", "PAR", "SIM", "MOS", "IBD", "MK", "PCA", "MIX")]
ORDER = list(scan_cases.SCANS)                  # table order
_rng = np.random.default_rng(20261021)
SNPS, SNPS_WIDE = (_rng.choice(np.array([-1, 0, 1, 2], dtype=np.int8), size=(N_ROWS, n), p=[0.08, 0.5, 0.34, 0.08]) for n in (N_ACC, N_WIDE))
SNPS.setflags(write=False)
SNPS_WIDE.setflags(write=False)
ROWS = _rng.permutation(N_ROWS)[:2099].astype(np.int64)
ROWS = _rng.permutation(np.append(ROWS, ROWS[11]))                  # 2100 rows, shuffled, one of them twice


def column_list(n_acc, n):
    """(n distinct columns, the same n and one of them again, shuffled)"""
    once = _rng.permutation(n_acc)[:n].astype(np.int32)
    return once, _rng.permutation(np.append(once, once[3]))


COLS = dict(zip(("narrow", "wide"), (column_list(N_ACC, 86), column_list(N_WIDE, 1100))))      # 87 and 1101 listed columns
_args, _twins = {}, {}


def make_ctx(mb):
    """a context whose scan budgets are ``mb`` MiB: the knobs are read when the context is created"""
    with pytest.MonkeyPatch.context() as env:
        for k in BUDGETS:
            env.setenv(k, str(mb))
        return engine.Context(0)


def make_panel(ctx, layout, snps):
    with pytest.MonkeyPatch.context() as env:       # packed panels are split wherever that saves memory; SNPM_PACKED_SPLIT=0 keeps whole rows
        if layout == "packed":
            env.setenv("SNPM_PACKED_SPLIT", "0")
        else:
            env.delenv("SNPM_PACKED_SPLIT", raising=False)
        panel = engine.Panel.from_host(ctx, snps, packed=layout != "int8")
    assert panel.pitch == PITCH[snps.shape[1]][layout], "the pitch policy changed: the three layouts are no longer three"
    return panel


def run_and_check(panel, scan, name, snps, rows, width=None):
    """one call of ``scan`` on ``rows`` of ``panel`` (which holds ``snps``) and the column list of ``width`` ("narrow" / "wide"; None:
    ``cols=None``), checked against the twin of selection ``name``"""
    cols = None if width is None else COLS[width][0 if scan == "ld_band" else 1]
    sel = snps if rows is None else snps[rows]
    if name not in _args:
        _args[name] = scan_cases.make_args(np.random.default_rng(len(sel)), len(sel), snps.shape[1] if cols is None else len(COLS[width][1]))
    a, entry = _args[name], scan_cases.SCANS[scan]
    if (scan, name) not in _twins:
        _twins[scan, name] = entry.twin(sel, a, cols)
    entry.check(entry.call(panel, a, cols, rows), _twins[scan, name], sel, a, cols)


def sequence():
    """all scans in table order, then in reverse, then each again straight after ``ibd_counts`` and after ``marker_select``"""
    seq = ORDER + ORDER[::-1]
    for scan in ORDER:
        seq += ["ibd_counts", scan, "marker_select", scan]
    return seq


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("width", ["narrow", "wide"])
def test_every_scan_after_every_kind_of_neighbour_on_one_context(width, layout):
    """with a row list and a column list: every layout holds a rows part and a cols part; on the wide panel most calls take 2 or 3 slabs"""
    snps = SNPS if width == "narrow" else SNPS_WIDE
    ctx = make_ctx(1)
    try:
        panel = make_panel(ctx, layout, snps)
        for scan in sequence():
            run_and_check(panel, scan, "listed " + width, snps, ROWS, width)
    finally:
        ctx.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_same_sequence_without_the_row_and_column_parts(layout):
    """``rows=None, cols=None`` on a panel of the first 300 rows: no layout has a rows or a cols part, every later part moves"""
    ctx = make_ctx(1)
    try:
        panel = make_panel(ctx, layout, SNPS[:300])
        for scan in sequence():
            run_and_check(panel, scan, "all", SNPS[:300], None)
    finally:
        ctx.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_the_block_grows_between_two_calls_of_a_scan_and_is_used_again(layout):
    """a fresh context PER SCAN, so that every scan lives through the growth: on 64 rows, on 2100 rows -- the block must grow -- and
    on 64 rows again"""
    for scan in ORDER:
        ctx = make_ctx(1)
        try:
            panel = make_panel(ctx, layout, SNPS)
            run_and_check(panel, scan, "few", SNPS, ROWS[:64], "narrow")
            run_and_check(panel, scan, "listed narrow", SNPS, ROWS, "narrow")
            run_and_check(panel, scan, "few", SNPS, ROWS[:64], "narrow")
        finally:
            ctx.close()


def test_six_scans_hold_the_scratch_of_the_largest_not_of_all():
    """1135 accessions x 120 000 rows, 64 MiB budgets: a slab of planes takes most of its budget (120 000 rows: 30 windows of 4000,
    so that the two window bitsets of ``ibd_counts`` stay at 10 MB).  Free device memory before the first scan, after
    ``kinship_counts`` (it dropped by d1) and after all six (by d6): d6 <= 2 * d1.  With a block per scan d6 is about 6 * d1.  The
    results are not compared here."""
    ctx = make_ctx(64)
    try:
        panel = engine.Panel(ctx, 120000, 1135)
        panel.fill_synthetic(77)
        a = scan_cases.make_args(np.random.default_rng(8), 120000, 1135, windows=4000)
        ctx.synchronize()
        first, again = ctx.mem_info()[0], ctx.mem_info()[0]
        if abs(first - again) > 16 << 20:
            pytest.skip("free device memory moved by itself between two readings, %d then %d bytes: others are using the device" % (first, again))
        d = []
        for scan in ["kinship_counts", "f1_counts", "parent_counts", "sim_counts", "ibd_counts", "mix_counts"]:
            scan_cases.SCANS[scan].call(panel, a, None, None)
            d.append(first - ctx.mem_info()[0])
        d1, d6 = d[0], d[-1]
        print("free memory dropped by %s MiB after each of the six scans" % [round(x / 2.0 ** 20, 1) for x in d])
        assert d1 >= 48 << 20, d                     # (the planes of a kinship slab take most of the 64 MiB budget: a much smaller drop measures nothing)
        assert d6 <= 2 * d1, d
    finally:
        ctx.close()
