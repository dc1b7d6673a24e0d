"""the whole argument space of ``gc_decide`` (test infrastructure, no device): every count triple of every window size up to 40
rows as one table of call codes, the counts the kernel must report for it in closed form, and the rule of ``getWindowGenotype``
(core/genotype_cross.py:21-49 of the reference, ``likeliTest`` of core/snpmatch.py:40-55) at 50 digits in ``mpmath``.

``tests/golden/gcross_table.npz`` (written by ``tests/golden/make_golden_gcross_table.py``) holds what ``reference_decide`` says of
every distinct ``(m1, mh, m2, tot)`` the tables produce, so a machine without ``mpmath`` checks against the same decisions.

``stored_decide`` is one more copy of the rule, in numpy over the fixture's 50-digit parts (``high``, ``tie``, ``ratio``).  It
exists because the recorded calls hold for ``n_marker_thres`` 5 only, while the device is also run with 1, 6 and 41 and ``mpmath``
may be absent there; ``test_fixture_holds_every_tuple_once`` ties it to the recorded calls of ``reference_decide``."""
import collections
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gcross_table.npz")
PARENT_PAIRS = [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]       # the ordered pairs of distinct values from {0, 1, 2}
THRESHOLDS = (1.0, 1.5, 2.706)
N_MARKER_THRES = 5
TOP_TOT = 40
NO_CALL = 3                                                           # class of './.'

Table = collections.namedtuple("Table", "codes p1 p2 win_off tots triple counts")


@functools.lru_cache(maxsize=None)
def triples(tot):
    """int32 [k, 3]: all (a, h, b) with a + h + b <= tot, in lexicographic order (the order is the contract: sample ``s`` of the
    window of ``tot`` rows carries triple ``s mod k``)"""
    out = np.array([(a, h, b) for a in range(tot + 1) for h in range(tot + 1 - a) for b in range(tot + 1 - a - h)], dtype=np.int32)
    out.flags.writeable = False
    return out


def true_counts(triple, parents):
    """(m1, mh, m2) the kernel must report for ``a`` rows of value p1, ``h`` rows of value 2 and ``b`` rows of value p2: a parent
    that is 2 shares its rows with the heterozygous counter, both ways"""
    triple = np.asarray(triple)
    a, h, b = triple[..., 0], triple[..., 1], triple[..., 2]
    one_is_het, two_is_het = parents[0] == 2, parents[1] == 2
    m1 = a + (h if one_is_het else 0)
    mh = h + (a if one_is_het else 0) + (b if two_is_het else 0)
    m2 = b + (h if two_is_het else 0)
    return np.stack([m1, mh, m2], axis=-1).astype(np.int32)


def build(parents, bar, tots=range(1, TOP_TOT + 1), seed=20261018):
    """``Table``: one window per ``tot`` of exactly ``tot`` rows, ``len(triples(max(tots)))`` samples; sample ``s`` of the window of
    ``tot`` rows holds ``a`` rows of value p1, ``h`` of value 2, ``b`` of value p2 and ``./.`` in the rest for triple
    ``s mod len(triples(tot))``, its rows permuted on their own (so the four waves of the kernel see different shares of each
    count).  ``bar`` (0 / 1) is the separator bit of every code.  ``triple`` int32 [n_win, n_samples, 3] is the intended triple,
    ``counts`` what the kernel must report (``true_counts``: closed form, not a scan of ``codes``)."""
    assert tuple(parents) in PARENT_PAIRS and bar in (0, 1)
    tots = [int(t) for t in tots]
    ns = len(triples(max(tots)))
    rng = np.random.default_rng(seed)
    win_off = np.concatenate(([0], np.cumsum(tots))).astype(np.int64)
    codes = np.empty((int(win_off[-1]), ns), dtype=np.uint8)
    triple = np.empty((len(tots), ns, 3), dtype=np.int32)
    for w, tot in enumerate(tots):
        t = triples(tot)[np.arange(ns) % len(triples(tot))]
        a, h, b = t[:, 0], t[:, 1], t[:, 2]
        row = np.arange(tot)[:, None]
        block = np.where(row < a, parents[0], np.where(row < a + h, 2, np.where(row < a + h + b, parents[1], NO_CALL)))
        codes[win_off[w]:win_off[w + 1]] = rng.permuted(block.astype(np.uint8), axis=0)
        triple[w] = t
    codes |= np.uint8(bar << 3)
    n = len(codes)
    table = Table(codes, np.full(n, parents[0], dtype=np.int8), np.full(n, parents[1], dtype=np.int8), win_off,
                  np.array(tots, dtype=np.int64), triple, true_counts(triple, parents))
    for a in table:
        a.flags.writeable = False
    return table


# ------------------------------------------------------------------------------------------------ the rule at 50 digits
@functools.lru_cache(maxsize=None)
def _mp():
    import mpmath
    ctx = mpmath.mp.clone()
    ctx.dps = 50
    return ctx


@functools.lru_cache(maxsize=None)
def reference_likeli(m, tot):
    """likeliTest(tot, m) as a 50-digit number; None where the reference gives NaN (tot == 0 or m == 0)"""
    assert 0 <= m <= tot, "provided y is greater than n"
    mp = _mp()
    if tot == 0 or m == 0:
        return None
    if m == tot:
        return mp.mpf(1)
    p = mp.mpf(0.99999999)                               # the double the reference's literal is, converted exactly
    ps = mp.mpf(m) / tot
    return m * mp.log(ps / p) + (tot - m) * mp.log((1 - ps) / (1 - p))


@functools.lru_cache(maxsize=None)
def reference_parts(m1, mh, m2, tot):
    """(high, tie, ratio) of one count tuple, before any threshold: ``high`` the first class with the smallest likelihood that is
    not NaN (-1: there is none), ``tie`` more than one ratio equal to 1, ``ratio`` the smallest ratio different from 1 as a 50-digit
    number (None: there is none).  Two likelihoods of one window are equal exactly when their counts are: equality is decided on
    the counts, order on the 50-digit values."""
    ms = (m1, mh, m2)
    like = [reference_likeli(m, tot) for m in ms]
    live = [k for k in range(3) if like[k] is not None]
    if not live:
        return -1, False, None
    high = live[0]
    for k in live[1:]:
        if ms[k] != ms[high] and like[k] < like[high]:
            high = k
    top = like[high]
    if not top > 0:                                      # get_fraction: every ratio is NaN
        return high, False, None
    tie = sum(1 for k in live if ms[k] == ms[high]) > 1
    rest = [like[k] / top for k in live if ms[k] != ms[high]]
    return high, tie, (min(rest) if rest else None)


def reference_decide(m1, mh, m2, tot, lr_thres, n_marker_thres=N_MARKER_THRES):
    """(call, runner-up ratio) by the rule of ``getWindowGenotype`` at 50 digits: call -1 (NA), 0, 1 or 2; the ratio as the double
    nearest to the 50-digit value, NaN where the window is NA by its size or for want of a match, or where no ratio other than 1
    exists (``lr_thres`` stands in for it then).  ``lr_thres`` is taken as the double it is."""
    if tot < n_marker_thres or not (m1 or mh or m2):
        return -1, float("nan")
    mp = _mp()
    high, tie, ratio = reference_parts(int(m1), int(mh), int(m2), int(tot))
    shown = float("nan") if ratio is None else float(ratio)
    if tie:
        return 1, shown
    thres = mp.mpf(float(lr_thres))
    nxt = thres if ratio is None else ratio
    call = -1
    if high == 0 and nxt >= thres:
        call = 0
    elif high == 2 and nxt >= thres:
        call = 2
    if high == 1:
        call = 1
    return call, shown


# ------------------------------------------------------------------------------------------------ the fixture
_fixture = {}
_sorted_keys = []                                        # the search keys of ``lookup``, kept apart from what ``fixture`` returns


def _key(m1, mh, m2, tot):
    return ((np.asarray(tot, dtype=np.int64) * 64 + m1) * 64 + mh) * 64 + m2


def fixture():
    """the arrays of tests/golden/gcross_table.npz (read once, shared, read-only); ``key`` [k, 4] = (tot, m1, mh, m2) in
    lexicographic order"""
    if not _fixture:
        with np.load(GOLDEN) as z:
            _fixture.update({k: z[k] for k in z.files})
        for a in _fixture.values():
            a.flags.writeable = False
    return _fixture


def lookup(counts, tot):
    """index into the fixture of every cell: ``counts`` [..., 3], ``tot`` broadcast against its leading axes"""
    if not _sorted_keys:
        key = fixture()["key"].astype(np.int64)
        _sorted_keys.append(_key(key[:, 1], key[:, 2], key[:, 3], key[:, 0]))
        _sorted_keys[0].flags.writeable = False
    sorted_keys = _sorted_keys[0]
    counts = np.asarray(counts, dtype=np.int64)
    want = _key(counts[..., 0], counts[..., 1], counts[..., 2], np.broadcast_to(tot, counts.shape[:-1]))
    at = np.searchsorted(sorted_keys, want)
    assert np.array_equal(sorted_keys[np.minimum(at, len(sorted_keys) - 1)], want), "a count tuple the fixture does not hold"
    return at


def stored_decide(at, tot, lr_thres, n_marker_thres=N_MARKER_THRES):
    """the rule applied to what the fixture stores of every cell (``high``, ``tie`` and the runner-up ``ratio``, all from the
    50-digit values): the call for any ``lr_thres`` and ``n_marker_thres``, not only the recorded ones"""
    fix = fixture()
    high, tie, ratio = fix["high"][at], fix["tie"][at], fix["ratio"][at]
    nxt = np.where(np.isnan(ratio), lr_thres, ratio)
    call = np.full(high.shape, -1, dtype=np.int8)
    call[(high == 0) & (nxt >= lr_thres)] = 0
    call[(high == 2) & (nxt >= lr_thres)] = 2
    call[high == 1] = 1
    call[tie] = 1
    call[(np.broadcast_to(tot, high.shape) < n_marker_thres) | (high < 0)] = -1
    return call


def golden_calls(counts, tot, lr_thres):
    """the recorded reference call (``n_marker_thres`` 5) of every cell for one of the recorded thresholds"""
    return fixture()["call"][lookup(counts, tot), THRESHOLDS.index(lr_thres)]
