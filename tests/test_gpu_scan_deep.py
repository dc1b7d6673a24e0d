"""The resident-panel scans past 4 GiB of panel: every scan of tests/scan_cases.py reads rows whose byte offset in the panel lies
beyond 2^31 and 2^32, in each of the three layouts, and is compared with its numpy twin on the same rows.

One panel of 1135 accessions per layout -- byte pitches 1152 (int8), 512 (packed whole rows) and 256 + 32 (packed split rows: in
that layout the whole tail matrix lies behind ``tail_off`` = D x 256 > 2^32) -- of D rows, D the smallest multiple of 1024 with
(D - 4096) x main pitch > 2^32: 3 732 480, 8 393 728 and 16 782 336 rows, 4.3 to 4.9 GB on the device, one at a time.  The panel
is filled on the device with the counter-based synthetic panel; its last 2500 rows are then overwritten with a host-made block
through ``upload_rows`` (int8: about 5 % code 3 and 12 % missing; packed: no code 3).  The truth never comes from the device:
``synth.panel_rows`` for the synthetic rows, the host block for the last 2500.

Two selections serve every scan: ``tail``, the dense range of the last 2500 rows (a huge ``row0``, two 1024-row steps and a part),
and ``straddle``, a shuffled int64 row LIST with one repeat of the 65 rows around each of 2^31 // main pitch and 2^32 // main pitch,
rows 0 .. 31 and the last 32 rows: 195 entries.  A reader that formed ``row * pitch`` in 32 bits would go wrong for every row of
``tail`` and for 65 (an unsigned product: the rows from 2^32 on, read 2^32 bytes earlier, e.g. packed row 8 388 636 as row 28) to 131
(a signed one: the rows from 2^31 on as well) rows of ``straddle``, and count the calls of other rows.

Every scan runs on all 1135 columns (``cols=None``), except ``mix_counts``: its twin contracts in int64 without BLAS, so it gets a
list of 131 columns with 0, 1023, 1024 (the first accession of the split layout's tail matrix) and 1134 and one repeat.  Window,
chain and group offsets are relative to the selection and hold an empty window.  The twins' results on ``tail`` are computed once
per host block and shared by the layouts that hold it."""
import types

import numpy as np
import pytest

import scan_cases
from snpmatch_amd import engine, synth

pytestmark = pytest.mark.gpu

N_ACC, TAIL, SEED = 1135, 2500, 20261021
LAYOUTS = ["int8", "packed", "split"]
PITCH = {"int8": 1152, "packed": 512, "split": 256 + 32}
MAIN_PITCH = {"int8": 1152, "packed": 512, "split": 256}
BOUNDARIES = (1 << 31, 1 << 32)
LISTED = {"mix_counts"}                         # the scans that get COLS instead of all columns
_rng = np.random.default_rng(515)
COLS = np.concatenate([[0, 1023, 1024, 1134], _rng.choice(np.setdiff1d(np.arange(N_ACC), [0, 1023, 1024, 1134]), size=126, replace=False)])
COLS = _rng.permutation(np.append(COLS, COLS[7])).astype(np.int32)
_blocks, _args, _twins = {}, {}, {}


def depth(layout):
    """the smallest multiple of 1024 with (D - 4096) * main pitch > 2^32"""
    return -(-((1 << 32) // MAIN_PITCH[layout] + 1 + 4096) // 1024) * 1024


def block_of(kind):
    """the host block of the last TAIL rows, made once: -1 / 0 / 1 / 2 as in the other device tests, the int8 one with code 3"""
    if kind not in _blocks:
        rng = np.random.default_rng(900 + len(kind))
        v = rng.choice(np.array([-1, 0, 1, 2], dtype=np.int8), size=(TAIL, N_ACC), p=[0.12, 0.45, 0.35, 0.08])
        if kind == "int8":
            v[rng.random(v.shape) < 0.05] = 3
        v.setflags(write=False)
        _blocks[kind] = v
    return _blocks[kind]


def straddle_runs(layout):
    mp, D = MAIN_PITCH[layout], depth(layout)
    return [range(0, 32)] + [range(B // mp - 32, B // mp + 33) for B in BOUNDARIES] + [range(D - 32, D)]


def straddle_rows(layout):
    rows = np.concatenate([np.arange(r.start, r.stop, dtype=np.int64) for r in straddle_runs(layout)])
    rows = np.random.default_rng(31).permutation(rows)
    return np.append(rows, rows[5])


def args_of(n_rows):
    if n_rows not in _args:
        _args[n_rows] = scan_cases.make_args(np.random.default_rng(7000 + n_rows), n_rows, N_ACC)
    return _args[n_rows]


@pytest.fixture(scope="module", params=LAYOUTS)
def deep(request):
    layout = request.param
    kind = "int8" if layout == "int8" else "packed"
    D = depth(layout)
    assert D % 1024 == 0 and (D - 4096) * MAIN_PITCH[layout] > 1 << 32 >= (D - 1024 - 4096) * MAIN_PITCH[layout]
    with pytest.MonkeyPatch.context() as env:       # packed panels are split wherever that saves memory; SNPM_PACKED_SPLIT=0 keeps whole rows
        if layout == "packed":
            env.setenv("SNPM_PACKED_SPLIT", "0")
        else:
            env.delenv("SNPM_PACKED_SPLIT", raising=False)
        panel = engine.Panel(engine.default_context(), D, N_ACC, packed=layout != "int8")
    try:
        assert panel.pitch == PITCH[layout], "the pitch policy changed: this file would no longer reach 2^32 where it says"
        panel.fill_synthetic(SEED)
        panel.upload_rows(D - TAIL, block_of(kind))
        yield types.SimpleNamespace(layout=layout, kind=kind, D=D, panel=panel, block=block_of(kind))
    finally:
        panel.free()


def truth(deep, rows):
    """int8 [len(rows), N_ACC]: what the panel holds at ``rows``, from the host"""
    rows = np.asarray(rows, dtype=np.int64)
    out = synth.panel_rows(SEED, rows, 0, N_ACC)
    late = rows >= deep.D - TAIL
    out[late] = deep.block[rows[late] - (deep.D - TAIL)]
    return out


def test_rows_past_both_boundaries_are_selected_and_download_as_uploaded(deep):
    mp, D = MAIN_PITCH[deep.layout], deep.D
    listed = straddle_rows(deep.layout)
    assert listed.dtype == np.int64 and len(np.unique(listed)) == len(listed) - 1 and listed.max() == D - 1 and listed.min() == 0
    for B in BOUNDARIES:
        assert int((listed * mp >= B).sum()) >= 32 and int((listed * mp < B).sum()) >= 32
        assert (D - TAIL) * mp > B                              # every row of ``tail`` lies past both
        print("%s: D = %d, row %d is the first at or past byte 2^%d" % (deep.layout, D, -(-B // mp), B.bit_length() - 1))
    assert np.array_equal(deep.panel.download_rows(D - TAIL, TAIL), deep.block)
    for run in straddle_runs(deep.layout):
        got = deep.panel.download_rows(run.start, len(run))
        assert np.array_equal(got, truth(deep, np.arange(run.start, run.stop))), "rows %d .. %d" % (run.start, run.stop - 1)


@pytest.mark.parametrize("selection", ["tail", "straddle"])
@pytest.mark.parametrize("scan", sorted(scan_cases.SCANS))
def test_scan_equals_its_twin_on_the_truth_rows(deep, scan, selection):
    entry = scan_cases.SCANS[scan]
    cols = COLS if scan in LISTED else None
    if selection == "tail":
        rows, sel, key = range(deep.D - TAIL, deep.D), deep.block, (scan, deep.kind)
    else:
        rows, key = straddle_rows(deep.layout), None
        sel = truth(deep, rows)
    a = args_of(len(sel))
    if key is None or key not in _twins:
        want = entry.twin(sel, a, cols)
        if key is not None:
            _twins[key] = want
    else:
        want = _twins[key]
    got = entry.call(deep.panel, a, cols, rows)
    entry.check(got, want, sel, a, cols)
