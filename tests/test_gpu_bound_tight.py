"""
The tighter exact-mode bound (-m gpu): two-level sums in the long-tile dense k_fast, and the chain-magnitude reference term of
slab-carry jobs.  The bound decides which totals take the second pass; a bound that is too small is a wrong match count, so
everything here is held against the fp64 oracle (``c_oracle.genotyper``: the reference's chunk loop over the whole SNP axis).

  1. resident queries on 248-row tiles (SNPM_LONG_SCAN_ROWS=1) with parts capped at 1 and 2 (SNPM_DEBUG_MAX_PARTS: long parts,
     several epochs) and uncapped: block shapes of 3, 5 and 7 waves and a width with a pure pad line (the PAD instantiation);
     rows below one tile (247), a ragged last tile with an odd group count (751), exactly one epoch (15 872 = 64 * 248), an
     epoch boundary plus a remainder (16 125) and three epochs (40 000); weights constant 0.1 and 0.999 (the adversarial case
     for a rounding bound: every addition rounds the same way), PL-like, and spanning 1e-6 ... 1e6; with and without skip_hets.
     ninfo equal in every mode, |fast - reference| <= Query.error_bound, exact-mode counts equal, strict-mode bits equal.
  2. the same job through a three-slab Carry on int8 and packed slab buffers: |fast total - reference total| <= the job's bound
     for every accession, the flag list equal to the rule evaluated on the host, flagged totals (also forced ones) with the
     oracle's bits after SlabScorer's second pass.
  3. the finish kernel of the chain term runs again when the totals before the slab changed: a job scored twice onto one carry
     without a reset.
  4. the bound itself, derived and not measured: a one-slab job of 40 000 rows in ONE part is bounded by the reference term
     (computed here from the weights) + wsum * gamma(m) with m = 248 + 64 + 64 + groups + 2 + the carry's own term.
  5. all-integer weights: bound 0, nothing flagged, every mode bit-identical to the oracle.

Every oracle result is computed once per (width, rows, weights, skip_hets) and shared read-only between the cases.
"""
import contextlib
import functools
import os

import numpy as np
import pytest

from oracle import c_oracle
from snpmatch_amd import engine, synth

pytestmark = pytest.mark.gpu

SWITCHES = ("SNPM_LONG_SCAN_ROWS", "SNPM_DEBUG_MAX_PARTS", "SNPM_DEBUG_REEVAL")
CHUNK = 1000
U = 2.0 ** -53
TILE, EPOCH_TILES, REDUCE_GROUP = 248, 64, 64              # LONG_TILE_ROWS, EPOCH_TILES, REDUCE_GROUP of snpm_k_common.hpp
WIDTHS = [600, 1250, 1700, 2600]                           # 3-, 5-, 7-wave blocks; 2600: PAD_WIDTHS[0] of test_gpu_step_floor.py
ROWS = [247, 751, 15872, 16125, 40000]
CAPS = [pytest.param(1, id="one_part"), pytest.param(2, id="two_parts"), pytest.param(0, id="uncapped")]
WEIGHTS = ["const0.1", "const0.999", "pl", "span"]
_CODES = np.array([-1] * 5 + [0] * 60 + [1] * 33 + [2] * 2, dtype=np.int8)      # P(-1, 0, 1, 2) = (0.05, 0.60, 0.33, 0.02)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


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


def long_tiles(cap=0, **more):
    env = {"SNPM_LONG_SCAN_ROWS": 1}
    if cap:
        env["SNPM_DEBUG_MAX_PARTS"] = cap
    env.update(more)
    return context(**env)


@functools.lru_cache(maxsize=None)
def panel_db(n_acc, n):
    rng = np.random.default_rng(n_acc * 11 + n)
    return frozen(_CODES[rng.integers(0, 100, size=(n, n_acc), dtype=np.uint8)])[0]


@functools.lru_cache(maxsize=None)
def weights(kind, n):
    rng = np.random.default_rng(len(kind) * 1000003 + n)
    if kind.startswith("const"):
        wei = np.full((n, 3), float(kind[5:]))
    elif kind == "pl":
        wei = synth.sample_weights(rng, rng.choice(np.array([0, 1, 2], dtype=np.int8), size=n), frac_pl=1.0)
    elif kind == "span":
        wei = 10.0 ** rng.uniform(-6.0, 6.0, size=(n, 3))
    else:
        assert kind == "integer"
        wei = rng.integers(0, 4, size=(n, 3)).astype(np.float64)
    return frozen(np.ascontiguousarray(wei, dtype=np.float64))[0]


@functools.lru_cache(maxsize=None)
def reference(n_acc, n, kind, skip):
    return frozen(*c_oracle.genotyper(panel_db(n_acc, n), None, weights(kind, n), CHUNK, skip))


def predicted_flags(s_fast, bound):
    """the certificate's rule (an integer inside [s - B, s + B], or the interval reaching below zero) in numpy's fp64"""
    lo, hi = s_fast - bound, s_fast + bound
    return np.flatnonzero(~(lo >= 0.0) | (np.floor(lo) != np.floor(hi)))


def gamma(m):
    return m * U / (1.0 - m * U)


# --------------------------------------------------------------------------------------------------- 1. resident queries
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("n_acc", WIDTHS)
def test_resident_query_on_long_tiles_against_oracle(n_acc, cap):
    worst = 0.0
    with long_tiles(cap) as ctx:
        for n in ROWS:
            panel = engine.Panel.from_host(ctx, panel_db(n_acc, n))
            for kind in WEIGHTS:
                q = engine.Query(panel, None, weights(kind, n))
                bound = q.error_bound(CHUNK)
                assert bound > 0.0
                for skip in (False, True):
                    want_s, want_n = reference(n_acc, n, kind, skip)
                    tag = (n_acc, cap, n, kind, skip)
                    s, ninfo = q.run(CHUNK, skip, engine.MODE_FAST)
                    err = float(np.max(np.abs(s - want_s)))
                    worst = max(worst, err / bound)
                    assert np.array_equal(ninfo, want_n), tag
                    assert err <= bound, tag + (err, bound)
                    s, ninfo = q.run(CHUNK, skip, engine.MODE_EXACT)
                    assert np.array_equal(ninfo, want_n), tag
                    assert np.array_equal(s.astype(np.int64), want_s.astype(np.int64)), tag
                    s, ninfo = q.run(CHUNK, skip, engine.MODE_STRICT)
                    assert np.array_equal(ninfo, want_n) and np.array_equal(bits(s), bits(want_s)), tag
                q.free()
            panel.free()
    print("largest |fast - reference| / Query.error_bound: %.4f" % worst)


def test_full_occupancy_seven_wave_blocks_against_oracle():
    """The size from which the host keeps the single-level kernel: 7-wave blocks (1700 accessions) fit four per CU with the
    single-level kernel's registers and three with the two-level one's, so a scan of more than three blocks per CU (here 807
    tiles = 807 parts on a device of 256 CUs) stays on single-level sums.  Same checks as above on that launch; the smaller
    shapes above all run the two-level kernel, which needs fewer blocks than fit."""
    n_acc, n, kind = 1700, 200000, "pl"
    rng = np.random.default_rng(1700)
    db = rng.integers(-1, 3, size=(n, n_acc), dtype=np.int8)
    wei = weights(kind, n)
    with long_tiles(0) as ctx:
        panel = engine.Panel.from_host(ctx, db)
        q = engine.Query(panel, None, wei)
        bound = q.error_bound(CHUNK)
        for skip in (False, True):
            want_s, want_n = c_oracle.genotyper(db, None, wei, CHUNK, skip)
            s, ninfo = q.run(CHUNK, skip, engine.MODE_FAST)
            assert np.array_equal(ninfo, want_n), skip
            assert float(np.max(np.abs(s - want_s))) <= bound, skip
            s, ninfo = q.run(CHUNK, skip, engine.MODE_EXACT)
            assert np.array_equal(ninfo, want_n), skip
            assert np.array_equal(s.astype(np.int64), want_s.astype(np.int64)), skip
        q.free()
        panel.free()


# ------------------------------------------------------------------------------------------------------- 2. slab carries
JOB_ROWS = 40000
SLABS = (16000, 16000, 8000)                    # 64.5 tiles (just past one epoch when the parts are capped), a short last slab
FORMATS = [pytest.param(False, id="int8"), pytest.param(True, id="packed")]


def chunks_after(slabs, k):
    return sum(-(-s // CHUNK) for s in slabs[k + 1:])


def first_pass(ctx, db, wei, slabs, skip, packed, repeat=1):
    """the first pass of SlabScorer.run(MODE_EXACT) by hand; repeat > 1 scores the job again onto the same carry, no reset.
    Returns the fast totals, the counts, the bound after every repetition, the flag list (sorted) and the flag count."""
    starts = np.concatenate([[0], np.cumsum(slabs)])
    panel = engine.Panel(ctx, max(slabs), db.shape[1], packed=packed)
    carry = engine.Carry(ctx, db.shape[1])
    queries = [None] * len(slabs)
    bounds = []
    for _ in range(repeat):
        for k in range(len(slabs)):
            panel.upload_rows(0, db[starts[k]:starts[k + 1]])
            if queries[k] is None:
                queries[k] = engine.Query(panel, None, wei[starts[k]:starts[k + 1]])
            queries[k].run_carry(carry, CHUNK, skip, engine.MODE_EXACT, chunks_after(slabs, k))
        bounds.append(float(carry.error_bound()))
    s_fast, ninfo, flagged = carry.finish()
    n_flagged = int(carry.n_flagged)
    for q in queries:
        q.free()
    carry.free()
    panel.free()
    return s_fast, ninfo, bounds, flagged, n_flagged


def slab_scorer(ctx, db, wei, slabs, skip, packed):
    starts = np.concatenate([[0], np.cumsum(slabs)])
    panel = engine.Panel(ctx, max(slabs), db.shape[1], packed=packed)

    def load(k, p):
        p.upload_rows(0, db[starts[k]:starts[k + 1]])

    return engine.SlabScorer(panel, list(slabs), load, lambda k: wei[starts[k]:starts[k + 1]], chunk=CHUNK, skip_hets=skip)


@pytest.mark.parametrize("cap", [pytest.param(1, id="one_part"), pytest.param(0, id="uncapped")])
@pytest.mark.parametrize("packed", FORMATS)
@pytest.mark.parametrize("n_acc", [1250, 2600])
def test_three_slab_carry_bound_flags_and_reference_bits(n_acc, packed, cap):
    db = panel_db(n_acc, JOB_ROWS)
    worst = 0.0
    for kind in WEIGHTS:
        wei = weights(kind, JOB_ROWS)
        for skip in (False, True):
            want_s, want_n = reference(n_acc, JOB_ROWS, kind, skip)
            tag = (n_acc, packed, cap, kind, skip)
            with long_tiles(cap) as ctx:
                s_fast, ninfo, (bound,), flagged, n_flagged = first_pass(ctx, db, wei, SLABS, skip, packed)
                sc = slab_scorer(ctx, db, wei, SLABS, skip, packed)
                s, ninfo2, info = sc.run(engine.MODE_EXACT)
                sc.free()
            err = np.abs(s_fast - want_s)
            worst = max(worst, float(err.max()) / bound)
            want_flags = predicted_flags(s_fast, bound)
            assert np.array_equal(ninfo, want_n) and np.array_equal(ninfo2, want_n), tag
            assert bound > 0.0 and np.all(err <= bound), tag + (bound, int(np.argmax(err)), float(err.max()))
            assert n_flagged == len(want_flags), tag + (n_flagged, len(want_flags))
            assert info["n_strict_reeval"] == n_flagged, tag
            if n_flagged <= 64:
                assert np.array_equal(flagged, want_flags), tag + (flagged, want_flags)
                assert np.array_equal(bits(s)[want_flags], bits(want_s)[want_flags]), tag
                quiet = np.ones(n_acc, dtype=bool)
                quiet[want_flags] = False
                assert np.array_equal(bits(s)[quiet], bits(s_fast)[quiet]), tag
            else:
                assert np.array_equal(bits(s), bits(want_s)), tag
            assert np.array_equal(s.astype(np.int64), want_s.astype(np.int64)), tag
    print("largest |fast total - reference total| / Carry.error_bound: %.4f" % worst)


@pytest.mark.parametrize("packed", FORMATS)
def test_forced_flags_end_with_reference_bits(packed):
    n_acc, kind = 1250, "const0.999"
    db, wei = panel_db(n_acc, JOB_ROWS), weights(kind, JOB_ROWS)
    want_s, want_n = reference(n_acc, JOB_ROWS, kind, False)
    with long_tiles(1, SNPM_DEBUG_REEVAL=3) as ctx:
        sc = slab_scorer(ctx, db, wei, SLABS, False, packed)
        s, ninfo, info = sc.run(engine.MODE_EXACT)
        sc.free()
    assert info["second_pass"] is True and info["n_strict_reeval"] >= 3
    assert np.array_equal(ninfo, want_n)
    assert np.array_equal(bits(s)[:3], bits(want_s)[:3])
    assert np.array_equal(s.astype(np.int64), want_s.astype(np.int64))


# ------------------------------------------------------------------------------- 3. the chain term follows the totals before
def chain_term(wei, slabs, w_before=0.0):
    """u * sum over the chunks of P2(W_before + prefix of the chunk sums of wmax), nothing rounded up: a lower bound of the device's"""
    wmax = np.abs(wei).max(axis=1)
    starts = np.concatenate([[0], np.cumsum(slabs)])
    run, total = w_before, 0.0
    for k in range(len(slabs)):
        for r0 in range(starts[k], starts[k + 1], CHUNK):
            run += float(wmax[r0:min(r0 + CHUNK, starts[k + 1])].sum())
            total += 2.0 ** np.floor(np.log2(run))
    return total * U


@pytest.mark.parametrize("packed", FORMATS)
def test_second_run_onto_the_same_carry_is_charged_at_the_larger_totals(packed):
    """A job scored twice onto one carry without a reset: the second run's chain additions happen on totals at least twice as
    large, so every one of them is charged at least twice the first run's, i.e. bound(2 runs) - 2 * bound(1 run) is at least the
    first run's chain term (the carry's own term only adds to the difference: 2 W gamma(7) - 2 W gamma(4) > 0).  With a finish
    kernel that did not run again the difference would be those 6 W u alone, less than a chain term of some 15 W u."""
    n_acc, kind = 1250, "const0.999"
    db, wei = panel_db(n_acc, JOB_ROWS), weights(kind, JOB_ROWS)
    with long_tiles(1) as ctx:
        _, _, (b1, b2), _, _ = first_pass(ctx, db, wei, SLABS, False, packed, repeat=2)
    chain1 = chain_term(wei, SLABS)
    w = float(np.abs(wei).max(axis=1).sum())
    print("bound after one run %.6e, after two %.6e, chain term of one run %.6e (%.1f W u)" % (b1, b2, chain1, chain1 / (w * U)))
    assert chain1 > 10.0 * w * U                    # the construction: the chain term stands out of the carry's own term
    assert b2 >= b1 > 0.0
    assert b2 - 2.0 * b1 >= chain1 * (1.0 - 1e-6), (b1, b2, chain1)


# ------------------------------------------------------------------------------------------- 4. the bound, derived
@pytest.mark.parametrize("skip", [pytest.param(False, id="hets"), pytest.param(True, id="skip_hets")])
@pytest.mark.parametrize("n_acc", WIDTHS)
def test_one_part_bound_is_the_two_level_formula(n_acc, skip):
    """40 000 rows in one part = 162 tiles = three epochs, three partial slots, one reduce group.  A term passes through at most 248
    additions of its tile, 64 of its epoch, 64 of its group, one per group and two more: m = 248 + 64 + 64 + 1 + 2 = 379 (it was
    64 * 248 + 64 + 1 + 2 = 15 939).  The job's bound is the reference term (in-chunk gamma(len + 3) and the chain term, from
    the weights) + W gamma(m) + the carry's W gamma(slabs + 1), each rounded up by 1e-7 at most a few times."""
    n, kind = JOB_ROWS, "pl"
    db, wei = panel_db(n_acc, n), weights(kind, n)
    want_s, want_n = reference(n_acc, n, kind, skip)
    with long_tiles(1) as ctx:
        s_fast, ninfo, (bound,), _, _ = first_pass(ctx, db, wei, (n,), skip, False)
    wmax = np.abs(wei).max(axis=1)
    w = float(wmax.sum())
    n_groups = 1
    m = TILE + EPOCH_TILES + REDUCE_GROUP + n_groups + 2
    assert m <= 248 + 64 + 64 + n_groups + 2
    in_chunk = sum(float(wmax[r0:r0 + CHUNK].sum()) * (min(CHUNK, n - r0) + 3) for r0 in range(0, n, CHUNK)) * U
    want = in_chunk + chain_term(wei, (n,)) + w * gamma(m) + w * gamma(2)
    print("bound %.6e  derived %.6e  ratio %.9f  (single-level fast term would add %.3e)" % (bound, want, bound / want, w * gamma(15939 - m)))
    assert want * (1.0 - 1e-6) <= bound <= want * (1.0 + 1e-5), (bound, want)
    assert np.array_equal(ninfo, want_n) and np.all(np.abs(s_fast - want_s) <= bound)


# ------------------------------------------------------------------------------------------------- 5. integer weights
@pytest.mark.parametrize("packed", FORMATS)
def test_integer_weights_are_exact_in_every_mode(packed):
    n_acc, kind = 1700, "integer"
    db, wei = panel_db(n_acc, JOB_ROWS), weights(kind, JOB_ROWS)
    for skip in (False, True):
        want_s, want_n = reference(n_acc, JOB_ROWS, kind, skip)
        for cap in (1, 0):
            with long_tiles(cap) as ctx:
                panel = engine.Panel.from_host(ctx, db, packed=packed)
                q = engine.Query(panel, None, wei)
                assert q.error_bound(CHUNK) == 0.0
                for mode in (engine.MODE_FAST, engine.MODE_EXACT, engine.MODE_STRICT):
                    s, ninfo = q.run(CHUNK, skip, mode)
                    assert np.array_equal(bits(s), bits(want_s)) and np.array_equal(ninfo, want_n), (packed, skip, cap, mode)
                q.free()
                panel.free()
                s_fast, ninfo, (bound,), flagged, n_flagged = first_pass(ctx, db, wei, SLABS, skip, packed)
            assert bound == 0.0 and n_flagged == 0 and len(flagged) == 0
            assert np.array_equal(bits(s_fast), bits(want_s)) and np.array_equal(ninfo, want_n)
