"""
The three narrow changes of the int8 step (-m gpu), each pinned where it could go wrong.

  1. k_fast never fetches a cache line that holds only padding: the lanes of such a line (bytes from roundup(n_acc, 128) up to the
     pitch) read the dword of the last valid byte instead and take 0xFF for it.  Widths with such a line (the last valid byte at
     every position of its dword, valid bytes that end exactly on a line, eight valid bytes in the last wave, the workload's
     10 000) and widths without one, dense / gathered / segmented, against the C oracle; and the fp64 bits of the valid columns
     of a padded panel against a panel of the same pitch and geometry whose pad columns hold random calls.
  2. every (part, column block) of the fast pass is scored exactly once: part counts 1, 3, 7 and 24 with two / three / five column
     blocks (far fewer parts than resident blocks), on widths with a pad line (the PAD instantiations) and without -- a pair scored
     twice or never is a wrong count.
  3. the sparse re-evaluation of a long segment list runs in one-wave blocks: explicit column lists of 1, 2, 3, 63 and 64
     accessions over slabs of 1, 7 and 130 chunks (fewer pairs than a wave, exactly 64, no multiple of 64) and over slabs on both
     sides of the switch to one-wave blocks, int8 and packed, through a column-list carry and through the resident query's tier
     (row-major and accession-major read), against the oracle's reference-order bits.

Panels hold a few thousand rows (tens of MB); every oracle result is computed once per shape and shared read-only.
"""
import contextlib
import functools
import os

import numpy as np
import pytest

from oracle import c_oracle
from snpmatch_amd import engine, synth

pytestmark = pytest.mark.gpu

SWITCHES = ("SNPM_DEBUG_MAX_PARTS", "SNPM_DEBUG_REEVAL", "SNPM_ACC_MAJOR_MIN_ROWS")
SKIPS = [pytest.param(False, id="hets"), pytest.param(True, id="skip_hets")]
FORMATS = [pytest.param(False, id="int8"), pytest.param(True, id="packed")]
_CODES = np.array([-1] * 5 + [0] * 60 + [1] * 33 + [2] * 2, dtype=np.int8)      # P(-1, 0, 1, 2) = (0.05, 0.60, 0.33, 0.02)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def rand_db(rng, n, n_acc):
    return _CODES[rng.integers(0, 100, size=(n, n_acc), dtype=np.uint8)]


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@contextlib.contextmanager
def context(**env):
    """a context created with exactly the given test switches set (the environment is as before once it exists), closed at the end"""
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    for k, v in env.items():
        assert k in SWITCHES
        os.environ[k] = str(v)
    try:
        ctx = engine.Context(0)
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    try:
        yield ctx
    finally:
        ctx.close()


def pure_pad_bytes(ctx, n_acc):
    """bytes of a row that lie in cache lines without a valid byte"""
    return ctx.row_pitch(n_acc) - (n_acc + 127) // 128 * 128


# ----------------------------------------------------------------------------------------------- 1a. pad line against the oracle
PAD_WIDTHS = [2600, 2601, 2602, 2603, 2688, 8200, 10000]
CONTROL_WIDTHS = [2689, 1135, 1250]
ROWS = [2999, 4001]


def pad_job(n_acc, n):
    """panel, dense weights, a sorted random row list with its weights, uneven windows of both"""
    rng = np.random.default_rng(n_acc * 7 + n)
    db = rand_db(rng, n, n_acc)
    codes = rng.choice(np.array([0, 1, 2], dtype=np.int8), size=n, p=[0.6, 0.35, 0.05])
    wei = synth.sample_weights(rng, codes, 0.8)
    rows = np.sort(rng.choice(n, size=n * 2 // 3 + 1, replace=False)).astype(np.int64)
    wei_g = np.ascontiguousarray(wei[:len(rows)])
    offs = []
    for m in (n, len(rows)):
        cuts = np.sort(rng.choice(np.arange(1, m), size=9, replace=False))
        offs.append(np.concatenate([[0, 0, 1], cuts, [m]]).astype(np.int64))         # an empty window, a window of one row
    return frozen(db, wei, rows, wei_g, offs[0], offs[1])


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("n_acc", PAD_WIDTHS + CONTROL_WIDTHS)
def test_pad_line_widths_against_oracle(n_acc, n):
    """MODE_EXACT counts and ninfo of the dense, the gathered and the segmented fast pass equal c_oracle.genotyper / windows on
    widths with and without a pure pad line, rows with tails of 1-3 rows and an odd group count, with and without skip_hets"""
    db, wei, rows, wei_g, off_d, off_g = pad_job(n_acc, n)
    with context() as ctx:
        pad = pure_pad_bytes(ctx, n_acc)
        assert (pad >= 128) == (n_acc in PAD_WIDTHS), (n_acc, ctx.row_pitch(n_acc), pad)
        panel = engine.Panel.from_host(ctx, db)
        for idx, w, off in ((None, wei, off_d), (rows, wei_g, off_g)):
            q = engine.Query(panel, idx, w)
            for skip in (False, True):
                want_s, want_n = c_oracle.genotyper(db, idx, w, 1000, skip)
                s, ninfo = q.run(1000, skip, engine.MODE_EXACT)
                assert np.array_equal(ninfo, want_n), (idx is not None, skip, np.flatnonzero(ninfo != want_n)[:8])
                assert np.array_equal(s.astype(np.int64), want_s.astype(np.int64)), (idx is not None, skip)
                ws, wn, wts, wtn = c_oracle.windows(db, idx, w, off, skip)
                fs, fn, fts, ftn = q.run_windows(off, skip, fast=True)
                assert np.array_equal(fn, wn) and np.array_equal(ftn, wtn), (idx is not None, skip)
                assert np.array_equal(fs.astype(np.int64), ws.astype(np.int64)), (idx is not None, skip)
                assert np.array_equal(fts.astype(np.int64), wts.astype(np.int64)), (idx is not None, skip)
            q.free()
        panel.free()


# ------------------------------------------------------------------------------------------------ 1b. pad line, bit invariance
# (valid width, full width of the same pitch and geometry, rows): 17 001 rows are 133 tiles of 128 rows -- three epochs of one
# part, two of each of three parts; 9001 rows are 71 tiles -- two epochs of one part
INVARIANCE = [pytest.param(2600, 2816, 17001, id="2600_in_2816"), pytest.param(10000, 10240, 9001, id="10000_in_10240")]


@pytest.mark.parametrize("n_acc,n_full,n", INVARIANCE)
def test_pad_columns_do_not_reach_valid_columns(n_acc, n_full, n):
    """MODE_FAST totals and ninfo of columns 0 .. n_acc-1 carry the same bits whether the columns behind them are padding (their
    lanes read elsewhere and take 0xFF) or random calls (their lanes read their own bytes) -- with the default parts and with
    the part cap at 1, 3 and 7 (several epochs per part)"""
    rng = np.random.default_rng(n_acc)
    full = rand_db(rng, n, n_full)
    codes = rng.choice(np.array([0, 1, 2], dtype=np.int8), size=n, p=[0.6, 0.35, 0.05])
    wei = synth.sample_weights(rng, codes, 0.8)
    views = {n_acc: np.ascontiguousarray(full[:, :n_acc]), n_full: full}
    want_s, want_n = c_oracle.genotyper(views[n_acc], None, wei, 1000, False)
    for cap in (0, 1, 3, 7):
        with context(**({"SNPM_DEBUG_MAX_PARTS": cap} if cap else {})) as ctx:
            assert ctx.row_pitch(n_acc) == ctx.row_pitch(n_full) == n_full and pure_pad_bytes(ctx, n_acc) >= 128
            got = []
            for width in (n_acc, n_full):
                panel = engine.Panel.from_host(ctx, views[width])
                q = engine.Query(panel, None, wei)
                s, ninfo = q.run(1000, False, engine.MODE_FAST)
                got.append((s[:n_acc].copy(), ninfo[:n_acc].copy()))
                q.free()
                panel.free()
        diff = np.flatnonzero(bits(got[0][0]) != bits(got[1][0]))
        print("cap %d: %d of %d totals differ" % (cap, len(diff), n_acc))
        assert len(diff) == 0, (cap, diff[:8])
        assert np.array_equal(got[0][1], got[1][1]) and np.array_equal(got[0][1], want_n), cap
        np.testing.assert_allclose(got[0][0], want_s, rtol=1e-11)


# -------------------------------------------------------------------------------------------------------------- 2. placement
# width -> column blocks: 4000 -> 2 (eight-wave blocks), 2600 -> 3 (four-wave), 4100 -> 3 (six-wave), 10 000 -> 5 (eight-wave)
PLACEMENT_WIDTHS = [4000, 2600, 4100, 10000]


@functools.lru_cache(maxsize=None)
def placement_job(n_acc):
    n = 2999
    rng = np.random.default_rng(n_acc + 1)
    db = rand_db(rng, n, n_acc)
    codes = rng.choice(np.array([0, 1, 2], dtype=np.int8), size=n, p=[0.6, 0.35, 0.05])
    wei = synth.sample_weights(rng, codes, 0.8)
    rows = np.sort(rng.choice(n, size=1777, replace=False)).astype(np.int64)
    return frozen(db, wei, rows) + tuple(c_oracle.genotyper(db, None, wei, 1000, False)) + \
        tuple(c_oracle.genotyper(db, rows, wei[:1777], 1000, False))


@pytest.mark.parametrize("cap", [1, 3, 7, 0])
@pytest.mark.parametrize("n_acc", PLACEMENT_WIDTHS)
def test_every_part_and_column_block_is_scored_once(n_acc, cap):
    """2999 rows are 24 tiles: with the part cap at 1, 3 and 7 there are far fewer (part, column block) pairs than resident blocks
    and every part walks several tiles; without a cap there are 24 parts.  Widths 2600, 4100 and 10 000 have a pad line, 4000
    has none.  Every accession equals the oracle, dense and gathered."""
    db, wei, rows, want_s, want_n, want_sg, want_ng = placement_job(n_acc)
    with context(**({"SNPM_DEBUG_MAX_PARTS": cap} if cap else {})) as ctx:
        panel = engine.Panel.from_host(ctx, db)
        s, ninfo = engine.Query(panel, None, wei).run(1000, False, engine.MODE_EXACT)
        sg, ng = engine.Query(panel, rows, wei[:len(rows)]).run(1000, False, engine.MODE_EXACT)
    assert np.array_equal(ninfo, want_n), np.flatnonzero(ninfo != want_n)[:8]
    assert np.array_equal(s.astype(np.int64), want_s.astype(np.int64))
    assert np.array_equal(ng, want_ng), np.flatnonzero(ng != want_ng)[:8]
    assert np.array_equal(sg.astype(np.int64), want_sg.astype(np.int64))


# -------------------------------------------------------------------------------------------------------------- 3. sparse tier
CHUNK = 40                                          # one 32-row batch of the kernel and a tail of 8 rows per chunk
# 1, 7 and 130 chunks, then both sides of the launch's switch from four-wave to one-wave blocks (more than 4 chunks per CU: 1024
# on the 256 CUs of an MI355X), the last slab with a short last chunk
SLABS = (1 * CHUNK, 7 * CHUNK, 130 * CHUNK, 1024 * CHUNK, 1025 * CHUNK, 1100 * CHUNK + 17)
N_ACC_SPARSE = 300
COLUMN_COUNTS = [1, 2, 3, 63, 64]


@functools.lru_cache(maxsize=None)
def sparse_job(skip, first_rows=0):
    """the job of all slabs, or its first `first_rows` rows"""
    n = sum(SLABS)
    rng = np.random.default_rng(31 + skip)
    db = rand_db(rng, n, N_ACC_SPARSE)
    codes = rng.choice(np.array([0, 1, 2], dtype=np.int8), size=n)
    wei = synth.sample_weights(rng, codes, frac_pl=1.0)
    if first_rows:
        db, wei = np.ascontiguousarray(db[:first_rows]), np.ascontiguousarray(wei[:first_rows])
    return frozen(db, wei) + tuple(frozen(*c_oracle.genotyper(db, None, wei, CHUNK, skip)))


def column_list(ncols):
    """a sorted list that holds the first, the last and both sides of a wave boundary of the accessions"""
    rng = np.random.default_rng(ncols)
    fixed = [0, N_ACC_SPARSE - 1, 63, 64][:ncols]
    rest = rng.choice(np.setdiff1d(np.arange(N_ACC_SPARSE), fixed), size=ncols - len(fixed), replace=False)
    return np.sort(np.concatenate([fixed, rest])).astype(np.int32)


@pytest.mark.parametrize("skip", SKIPS)
@pytest.mark.parametrize("packed", FORMATS)
@pytest.mark.parametrize("ncols", COLUMN_COUNTS)
def test_column_list_carry_gets_reference_bits(ncols, packed, skip):
    """A fast job over the three slabs, then the listed columns through a column-list carry in MODE_STRICT (the chain continued
    from slab to slab) and patched in: the listed totals carry the oracle's bits, every other total is bit-equal to the fast
    pass's, the counts are the oracle's"""
    db, wei, want_s, want_n = sparse_job(skip)
    starts = np.concatenate([[0], np.cumsum(SLABS)])
    cols = column_list(ncols)
    with context() as ctx:
        panel = engine.Panel(ctx, max(SLABS), N_ACC_SPARSE, packed=packed)
        totals, listed = engine.Carry(ctx, N_ACC_SPARSE), engine.Carry(ctx, N_ACC_SPARSE)
        listed.set_columns(cols)
        queries = [engine.Query(panel, None, wei[starts[k]:starts[k + 1]]) for k in range(len(SLABS))]
        for carry, mode in ((totals, engine.MODE_FAST), (listed, engine.MODE_STRICT)):
            for k, q in enumerate(queries):
                panel.upload_rows(0, db[starts[k]:starts[k + 1]])
                q.run_carry(carry, CHUNK, skip, mode, sum(-(-s // CHUNK) for s in SLABS[k + 1:]))
            if carry is totals:
                s_fast, n_fast, _ = totals.finish()
        totals.patch_from(listed)
        s, ninfo, _ = totals.finish()
    assert np.array_equal(ninfo, want_n) and np.array_equal(n_fast, want_n)
    assert np.array_equal(bits(s)[cols], bits(want_s)[cols]), (cols, s[cols], want_s[cols])
    quiet = np.ones(N_ACC_SPARSE, dtype=bool)
    quiet[cols] = False
    assert np.array_equal(bits(s)[quiet], bits(s_fast)[quiet]), np.flatnonzero(quiet & (bits(s) != bits(s_fast)))
    np.testing.assert_allclose(s_fast, want_s, rtol=1e-11)


@pytest.mark.parametrize("acc_major", [pytest.param(False, id="row_major_read"), pytest.param(True, id="acc_major_read")])
@pytest.mark.parametrize("packed", FORMATS)
@pytest.mark.parametrize("count", COLUMN_COUNTS)
def test_resident_query_tier_gets_reference_bits(count, packed, acc_major):
    """The same kernels behind one query on a resident panel: accessions 0 .. count-1 forced through the sparse tier, read from
    the row-major panel (path 2) or from the accession-major copy (path 1, k_strict_sparse_T), skip_hets on and off: the whole
    job (3288 chunks: one-wave blocks) and its first 138 chunks (four-wave blocks)"""
    env = {"SNPM_DEBUG_REEVAL": count}
    if acc_major:
        env["SNPM_ACC_MAJOR_MIN_ROWS"] = 0
    for skip, short in ((False, False), (True, False), (False, True), (True, True)):
        db, wei, want_s, want_n = sparse_job(skip, 138 * CHUNK if short else 0)
        with context(**env) as ctx:
            panel = engine.Panel.from_host(ctx, db, packed=packed)
            s, ninfo, info = engine.Query(panel, None, wei).run(CHUNK, skip, engine.MODE_EXACT, return_info=True)
        print(count, skip, info)
        assert info["n_strict_reeval"] == count and info["reeval_path"] == (1 if acc_major else 2), info
        assert np.array_equal(ninfo, want_n)
        assert np.array_equal(bits(s)[:count], bits(want_s)[:count]), (s[:count], want_s[:count])
        assert np.array_equal(s.astype(np.int64), want_s.astype(np.int64))
