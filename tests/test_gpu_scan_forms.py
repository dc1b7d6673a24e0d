"""The forms of ``rows`` and ``cols`` of the eleven resident-panel scans that take a free column list, on the device (``mix_counts``
is the eleventh; the calls are those of the table in tests/scan_cases.py): a scan asked for every row as ``None``, as
``slice(0, n)`` and as ``range(0, n)``, and for every column as ``None`` and as ``arange(n_acc)``, gives the same bits; the scans
that count integers give the same counts for the row LIST ``arange(n)`` too.  The fp64 scans (``gram``, ``loadings``, ``admix``) are
compared among the dense forms only: their summation order is fixed by the arguments, and a row list is a different argument.  One
int8 and one packed panel of 70 rows by 67 accessions: 67 crosses the 64-column tile, 70 a 64-row step.  No tolerance anywhere."""
import types

import numpy as np
import pytest

import scan_cases
from snpmatch_amd import engine
from snpmatch_amd.core import admixture

pytestmark = pytest.mark.gpu

N_ROWS, N_ACC = 70, 67
WIN_OFF = [0, 20, 20, 45, N_ROWS]               # an empty window among them
_rng = np.random.default_rng(2024)
CLASSES = _rng.choice(np.array([0, 1, 2, 0xFF], dtype=np.uint8), size=(2, N_ROWS), p=[0.4, 0.35, 0.15, 0.1])
TAB = _rng.normal(size=(N_ROWS, 4))
VEC = _rng.normal(size=(N_ACC, 3))
Q0, F0 = admixture.random_start(7, N_ACC, N_ROWS, 2)
COST = np.array([[0, 2, 1, 2], [2, 0, 1, 2], [1, 1, 0, 2]], dtype=np.uint8)

ALT, REF = (_rng.integers(0, 256, size=N_ROWS).astype(np.uint8) for _ in range(2))
# the arguments of tests/scan_cases.py, whose table holds the calls
ARGS = types.SimpleNamespace(cls=CLASSES, win_off=WIN_OFF, par_min_sites=1, ibd=(2, 100000, 1), tab=TAB, vec=VEC, Q=Q0, F=F0, n_iter=2, mk_depth=1, mk_max=None,
                             grp_off=[0, 30, N_ROWS], err_rate=0.01, seed=5, chain_off=[0, 40, N_ROWS], cost=COST, switch=5, alt=ALT, ref=REF)
# the scans of the table with ``cols`` any list and ``rows``; ``site_counts`` (groups), ``ld_band`` (distinct columns) and ``window_counts`` (pairs)
# have their forms in their own files
SCANS = ["kinship_counts", "f1_counts", "parent_counts", "ibd_counts", "mix_counts", "gram", "loadings", "admix", "marker_select", "sim_counts", "mosaic"]


@pytest.fixture(scope="module", params=["int8", "packed"])
def panel(request):
    p = engine.Panel(engine.default_context(), N_ROWS, N_ACC, packed=request.param == "packed")
    p.fill_synthetic(4242)
    yield p
    p.free()


def _same_bits(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(_same_bits(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(_same_bits(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return type(a) is type(b) and a == b            # None, and the integers of ``marker_select``


@pytest.mark.parametrize("scan", sorted(SCANS))
def test_every_form_of_all_rows_and_all_columns_gives_the_same_bits(panel, scan):
    entry = scan_cases.SCANS[scan]
    call, counts_integers = (lambda p, c, r: entry.call(p, ARGS, c, r)), entry.counts_integers
    first = call(panel, None, None)
    assert any(np.asarray(a).any() for a in (first.values() if isinstance(first, dict) else first if isinstance(first, tuple) else [first])
               if isinstance(a, np.ndarray)), "a result of zeros compares nothing"
    row_forms = [None, slice(0, N_ROWS), range(0, N_ROWS)] + ([np.arange(N_ROWS)] if counts_integers else [])
    for rows in row_forms:
        for cols in (None, np.arange(N_ACC)):
            assert _same_bits(call(panel, cols, rows), first), "rows as %r, cols as %s" % (rows, "None" if cols is None else "arange")
