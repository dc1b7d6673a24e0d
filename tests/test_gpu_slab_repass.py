"""
The second pass of a slab-streamed job (-m gpu), pinned at its edges.  A job scored SNP slab after SNP slab in MODE_EXACT
adds the slabs' fast-pass totals and their error bounds up in a ``Carry``; ``Carry.finish`` lists the accessions whose total
the summed bound cannot vouch for, and ``SlabScorer.run`` streams the slabs once more for them: up to 64 through a column-list
carry (compact chunk sums, a chain continued from slab to slab, written back over the fast totals), more than 64 through a
strict pass over every accession.  What the pass owes, and what these tests hold against the fp64 oracle
(``c_oracle.genotyper``: the reference's chunk loop over the whole SNP axis, core/snpmatch.py:218-225):

  1. the bound is sound for EVERY accession, and the flag list is exactly what the fast totals and the bound predict;
  2. every flagged accession ends with the reference's bits, every other total is left as the first pass wrote it;
  3. 64 flagged accessions are patched, 65 re-run everyone -- in a slab job and in one query on a resident panel;
  4. nothing of one run (flag count, column list, bound) reaches the next run or mode, also with caller-owned totals;
  5. slabs of exactly one chunk and of one row.

On int8 and packed panels (a transient slab buffer read through its layout descriptor), with and without ``skip_hets``, with
flagged columns in every 256-thread block of the flag kernel and in the last, partly filled byte of a packed row, with a last
slab shorter than a chunk and with chunks of 7 rows (600 segments per slab in the compact rows).

Two comparisons are device against device, and are meant to be: "an unflagged total is bit-equal to the first pass's" (the
first pass driven by hand through the same public calls) and "a repeated run is bit-equal to the first run".  Everything else
is compared with the oracle or with a host recomputation from values the API returned.
"""
import contextlib
import functools
import os

import numpy as np
import pytest

from oracle import c_oracle
from snpmatch_amd import engine, synth

pytestmark = pytest.mark.gpu

CAP = 64                                    # the sparse tier's cap (REEVAL_CAP): 64 flagged are patched, 65 re-run everyone
SWITCHES = ("SNPM_DEBUG_REEVAL", "SNPM_ACC_MAJOR_MIN_ROWS")

# (n, n_acc, slabs, chunk): 600 + 600 + 86 chunks of 7 rows on a width of 256 + 1; a last slab shorter than one chunk on the
# width of the 1001 Genomes panel (1135 = 4 * 283 + 3: the last byte of a packed row holds three calls)
GEOMETRIES = [
    (9001, 257, (4200, 4200, 601), 7),
    (12345, 1135, (6000, 6000, 345), 1000),
]
FORMATS = [pytest.param(False, id="int8"), pytest.param(True, id="packed")]
SKIPS = [pytest.param(False, id="hets"), pytest.param(True, id="skip_hets")]
GEOMS = [pytest.param(0, id="chunk7"), pytest.param(1, id="short_last_slab")]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def rand_db(rng, n, n_acc):
    return rng.choice(np.array([-1, 0, 1, 2], dtype=np.int8), size=(n, n_acc), p=[0.05, 0.60, 0.33, 0.02])


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


def planted_columns(n_acc):
    """both sides of the first block boundary of the flag kernel (255 | 256), a wave boundary, and the last column"""
    return [3, 64, 255, 256, n_acc - 1]


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def job_data(kind, n, n_acc, chunk, skip, seed):
    """(db, wei, want_s, want_n) of one job, computed once and shared read-only by the cases that differ in the panel format only.
    kind "random": full-PL weights of a code vector that is no panel column (nothing is an exact integer);
    kind "planted": the planted columns are copies of one column and the weights are drawn from its calls (missing -> 0):
    their totals are sums of exp(0) = 1.0, exact integers, which the certificate has to flag by itself."""
    rng = np.random.default_rng(seed)
    db = rand_db(rng, n, n_acc)
    if kind == "planted":
        cols = planted_columns(n_acc)
        db[:, cols] = db[:, [cols[0]]]
        codes = db[:, cols[0]].copy()
        codes[codes < 0] = 0
    else:
        codes = rng.choice(np.array([0, 1, 2], dtype=np.int8), size=n)
    wei = synth.sample_weights(rng, codes, frac_pl=1.0)
    want_s, want_n = c_oracle.genotyper(db, None, wei, chunk, skip)
    return frozen(db, wei, want_s, want_n)


def chunks_after(slabs, chunk, k):
    return sum(-(-s // chunk) for s in slabs[k + 1:])


def first_pass(ctx, db, wei, slabs, chunk, skip, packed):
    """The first pass of SlabScorer.run(MODE_EXACT) driven by hand: every slab uploaded into one slab-sized panel and scored onto a
    carry.  Returns the fast totals, the counts, the job's bound, the flag list (sorted) and the flag count."""
    starts = np.concatenate([[0], np.cumsum(slabs)])
    panel = engine.Panel(ctx, max(slabs), db.shape[1], packed=packed)
    carry = engine.Carry(ctx, db.shape[1])
    queries = []
    for k in range(len(slabs)):
        panel.upload_rows(0, db[starts[k]:starts[k + 1]])
        q = engine.Query(panel, None, wei[starts[k]:starts[k + 1]])
        q.run_carry(carry, chunk, skip, engine.MODE_EXACT, chunks_after(slabs, chunk, k))
        queries.append(q)
    bound = carry.error_bound()
    s_fast, ninfo, flagged = carry.finish()
    n_flagged = int(carry.n_flagged)
    for q in queries:
        q.free()
    carry.free()
    panel.free()
    return s_fast, ninfo, float(bound), flagged, n_flagged


def predicted_flags(s_fast, bound):
    """the certificate's rule (an integer inside [s - B, s + B], or the interval reaching below zero) in numpy's fp64"""
    lo, hi = s_fast - bound, s_fast + bound
    return np.flatnonzero(~(lo >= 0.0) | (np.floor(lo) != np.floor(hi)))


def slab_scorer(ctx, db, wei, slabs, chunk, skip, packed):
    """a panel that holds one slab at a time; load(k) uploads slab k into its first rows"""
    starts = np.concatenate([[0], np.cumsum(slabs)])
    panel = engine.Panel(ctx, max(slabs), db.shape[1], packed=packed)

    def load(k, p):
        p.upload_rows(0, db[starts[k]:starts[k + 1]])

    return engine.SlabScorer(panel, list(slabs), load, lambda k: wei[starts[k]:starts[k + 1]], chunk=chunk, skip_hets=skip)


def others(n_acc, cols):
    keep = np.ones(n_acc, dtype=bool)
    keep[np.asarray(cols, dtype=np.int64)] = False
    return keep


# ------------------------------------------------------------------------------------------- 1. the certificate's contract
@pytest.mark.parametrize("skip", SKIPS)
@pytest.mark.parametrize("packed", FORMATS)
@pytest.mark.parametrize("geom", GEOMS)
def test_first_pass_bound_is_sound_and_flags_are_predicted(geom, packed, skip):
    """The first pass by hand on weights that match no column: counts exact, |fast total - reference total| <= bound for every
    accession, the flag list equal to the host's evaluation of the rule on the returned totals and bound (device and host add
    the same two fp64 operands for the bound), and int(total) right wherever nothing was flagged."""
    n, n_acc, slabs, chunk = GEOMETRIES[geom]
    db, wei, want_s, want_n = job_data("random", n, n_acc, chunk, skip, 100 + geom)
    with context() as ctx:
        s_fast, ninfo, bound, flagged, n_flagged = first_pass(ctx, db, wei, slabs, chunk, skip, packed)
    err = np.abs(s_fast - want_s)
    want_flags = predicted_flags(s_fast, bound)
    print("bound %.3e  max error %.3e  flagged %d  predicted %d" % (bound, err.max(), n_flagged, len(want_flags)))
    assert np.array_equal(ninfo, want_n)
    assert bound > 0.0 and np.all(err <= bound), (bound, int(np.argmax(err)), float(err.max()))
    assert n_flagged == len(want_flags), (n_flagged, want_flags)
    assert np.all(np.diff(flagged) > 0) and np.all(np.isin(flagged, want_flags))
    if n_flagged <= CAP:
        assert np.array_equal(flagged, want_flags), (flagged, want_flags)
    quiet = others(n_acc, want_flags)
    assert np.array_equal(s_fast[quiet].astype(np.int64), want_s[quiet].astype(np.int64))


# ------------------------------------------------------------------------------- 2. scattered flagged columns, nothing else moved
@pytest.mark.parametrize("skip", SKIPS)
@pytest.mark.parametrize("packed", FORMATS)
@pytest.mark.parametrize("geom", GEOMS)
def test_scattered_flagged_columns_get_reference_bits_and_nothing_else_moves(geom, packed, skip):
    """Five exact-integer totals in columns 3, 64, 255, 256 and the last one, no forced re-evaluation: the certificate flags them
    by itself, the second pass gives EVERY flagged accession the reference's bits, and every unflagged total is bit-equal to the
    hand-driven first pass's (device against device, on purpose: the write-back touched nothing else)."""
    n, n_acc, slabs, chunk = GEOMETRIES[geom]
    db, wei, want_s, want_n = job_data("planted", n, n_acc, chunk, skip, 200 + geom)
    planted = planted_columns(n_acc)
    with context() as ctx:
        s_fast, ninfo_fast, bound, flagged, n_flagged = first_pass(ctx, db, wei, slabs, chunk, skip, packed)
        sc = slab_scorer(ctx, db, wei, slabs, chunk, skip, packed)
        s, ninfo, info = sc.run(engine.MODE_EXACT)
        sc.free()
    print("bound %.3e  flagged %s  info %s" % (bound, flagged.tolist(), info))
    assert want_s[planted].tolist() == np.floor(want_s[planted]).tolist()          # the construction: exact integers
    assert info["second_pass"] is True
    assert n_flagged == len(flagged) <= CAP and set(planted) <= set(flagged.tolist())
    assert np.array_equal(flagged, predicted_flags(s_fast, bound))
    assert info["n_strict_reeval"] == len(flagged)
    assert np.array_equal(ninfo, want_n) and np.array_equal(ninfo_fast, want_n)
    assert np.array_equal(bits(s)[flagged], bits(want_s)[flagged]), (flagged, s[flagged], want_s[flagged])
    quiet = others(n_acc, flagged)
    assert np.array_equal(bits(s)[quiet], bits(s_fast)[quiet]), np.flatnonzero(quiet & (bits(s) != bits(s_fast)))
    assert np.array_equal(s[quiet].astype(np.int64), want_s[quiet].astype(np.int64))


# ------------------------------------------------------------------------------------------------------- 3. the cap, exactly
CAP_JOB = (9000, 300, (4000, 4000, 1000), 1000)
CAP_PLANTED = [200, 299]                    # two exact-integer totals: the natural flag set is not empty and not a prefix


@functools.lru_cache(maxsize=None)
def cap_data():
    n, n_acc, slabs, chunk = CAP_JOB
    rng = np.random.default_rng(64065)
    db = rand_db(rng, n, n_acc)
    db[:, CAP_PLANTED] = db[:, [CAP_PLANTED[0]]]
    codes = db[:, CAP_PLANTED[0]].copy()
    codes[codes < 0] = 0
    wei = synth.sample_weights(rng, codes, frac_pl=1.0)
    want_s, want_n = c_oracle.genotyper(db, None, wei, chunk, False)
    return frozen(db, wei, want_s, want_n)


def cap_first_pass(packed):
    """the hand-driven first pass without forced accessions: (s_fast, F0, {64: k64, 65: k65}) with |{0..k-1} u F0| = 64 / 65"""
    n, n_acc, slabs, chunk = CAP_JOB
    db, wei, want_s, want_n = cap_data()
    with context() as ctx:
        s_fast, ninfo, bound, flagged, n_flagged = first_pass(ctx, db, wei, slabs, chunk, False, packed)
    assert n_flagged <= 60, "the natural flag set holds %d accessions: choose another seed for cap_data()" % n_flagged
    f0 = set(flagged.tolist())
    assert len(f0) == n_flagged and f0 == set(predicted_flags(s_fast, bound).tolist())
    assert set(CAP_PLANTED) <= f0
    ks = {}
    for k in range(n_acc + 1):
        ks.setdefault(len(f0 | set(range(k))), k)          # the union grows by at most one per step: every size is met
    return s_fast, f0, {64: ks[64], 65: ks[65]}


@pytest.mark.parametrize("packed", FORMATS)
def test_slab_job_patches_64_and_reruns_everyone_at_65(packed):
    """64 flagged accessions (forced 0..k-1 and the natural set) take the column-list carry: they carry the reference's bits and
    the other 236 are bit-equal to the hand-driven first pass (device against device, on purpose).  One more, and SlabScorer.run
    scores every accession in reference order: all 300 carry the reference's bits."""
    n, n_acc, slabs, chunk = CAP_JOB
    db, wei, want_s, want_n = cap_data()
    s_fast, f0, ks = cap_first_pass(packed)
    print("natural flag set %s  k64 %d  k65 %d" % (sorted(f0), ks[64], ks[65]))
    with context(SNPM_DEBUG_REEVAL=ks[64]) as ctx:
        sc = slab_scorer(ctx, db, wei, slabs, chunk, False, packed)
        s, ninfo, info = sc.run(engine.MODE_EXACT)
        sc.free()
    flagged = np.array(sorted(f0 | set(range(ks[64]))), dtype=np.int64)
    assert len(flagged) == 64
    assert info == {"n_strict_reeval": 64, "second_pass": True}
    assert np.array_equal(ninfo, want_n)
    assert np.array_equal(bits(s)[flagged], bits(want_s)[flagged])
    quiet = others(n_acc, flagged)
    assert quiet.sum() == 236 and np.array_equal(bits(s)[quiet], bits(s_fast)[quiet])
    assert np.array_equal(s[quiet].astype(np.int64), want_s[quiet].astype(np.int64))
    with context(SNPM_DEBUG_REEVAL=ks[65]) as ctx:
        sc = slab_scorer(ctx, db, wei, slabs, chunk, False, packed)
        s, ninfo, info = sc.run(engine.MODE_EXACT)
        sc.free()
    assert info == {"n_strict_reeval": 65, "second_pass": True}
    assert np.array_equal(ninfo, want_n)
    assert np.array_equal(bits(s), bits(want_s)), np.flatnonzero(bits(s) != bits(want_s))


@pytest.mark.parametrize("acc_major", [pytest.param(False, id="row_major_read"), pytest.param(True, id="acc_major_read")])
@pytest.mark.parametrize("packed", FORMATS)
def test_resident_query_switches_tiers_between_64_and_65(packed, acc_major):
    """The same two counts in one query over the whole axis of a resident panel: at 64 the sparse tier (path 1: the accession-major
    copy, built under SNPM_ACC_MAJOR_MIN_ROWS=0; path 2: the strided read of the row-major panel) gives the flagged accessions
    the reference's bits, at 65 the dense tier (path 3) gives them to everyone."""
    n, n_acc, slabs, chunk = CAP_JOB
    db, wei, want_s, want_n = cap_data()
    s_fast, f0, ks = cap_first_pass(packed)
    # the forced accessions and the exact-integer totals are flagged under ANY sound bound; the query's bound is not the job's,
    # so the counts carry over only while nothing else is flagged
    assert f0 == set(CAP_PLANTED), "the natural flag set %s holds more than the planted columns: choose another seed" % sorted(f0)
    env = {"SNPM_ACC_MAJOR_MIN_ROWS": 0} if acc_major else {}
    for count in (64, 65):
        with context(SNPM_DEBUG_REEVAL=ks[count], **env) as ctx:
            panel = engine.Panel.from_host(ctx, db, packed=packed)
            s, ninfo, info = engine.Query(panel, None, wei).run(chunk, False, engine.MODE_EXACT, return_info=True)
        print(count, info)
        flagged = np.array(sorted(f0 | set(range(ks[count]))), dtype=np.int64)
        assert info["n_strict_reeval"] == count == len(flagged)
        assert np.array_equal(ninfo, want_n)
        assert np.array_equal(s.astype(np.int64), want_s.astype(np.int64))
        if count == 64:
            assert info["reeval_path"] == (1 if acc_major else 2)
            assert np.array_equal(bits(s)[flagged], bits(want_s)[flagged])
        else:
            assert info["reeval_path"] == 3
            assert np.array_equal(bits(s), bits(want_s)), np.flatnonzero(bits(s) != bits(want_s))


# ----------------------------------------------------------------------------------------------------- 4. state between runs
@pytest.mark.parametrize("packed", FORMATS)
def test_nothing_leaks_between_runs_modes_and_bound_outputs(packed):
    """One SlabScorer, run after run: exact twice (bit-equal results and equal info: device against device, on purpose, beside the
    oracle's bits for the flagged accessions), strict (the oracle's bits everywhere), exact again (as the first time: neither the
    flag count nor the column list of an earlier run or mode survives in the carry's device block), and once more with the
    totals kept in caller-owned tensors of 257 elements -- the patched values arrive there, the 64 bytes behind them stay."""
    import torch
    n, n_acc, slabs, chunk = GEOMETRIES[0]
    db, wei, want_s, want_n = job_data("planted", n, n_acc, chunk, False, 200)
    planted = planted_columns(n_acc)
    with context() as ctx:
        _, _, bound, flagged, _ = first_pass(ctx, db, wei, slabs, chunk, False, packed)
        sc = slab_scorer(ctx, db, wei, slabs, chunk, False, packed)
        s1, n1, info1 = sc.run(engine.MODE_EXACT)
        s2, n2, info2 = sc.run(engine.MODE_EXACT)
        s3, n3, info3 = sc.run(engine.MODE_STRICT)
        s4, n4, info4 = sc.run(engine.MODE_EXACT)
        # caller-owned totals: [n_acc] and 8 more elements (64 bytes) that belong to the caller
        pad, sent_f, sent_i = 8, -12345.678, 0x5A5A5A5A5A5A5A5A
        d_score = torch.full((n_acc + pad,), sent_f, dtype=torch.float64, device="cuda:0")
        d_ninfo = torch.full((n_acc + pad,), sent_i, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        sc.carry.reset()                    # outputs are bound before the first slab of a job
        sc.carry.bind_outputs(d_score.data_ptr(), d_ninfo.data_ptr())
        s5, n5, info5 = sc.run(engine.MODE_EXACT)
        ctx.synchronize()
        t_score, t_ninfo = d_score.cpu().numpy(), d_ninfo.cpu().numpy()
        sc.carry.reset()
        sc.carry.bind_outputs(None, None)
        sc.free()
    print("bound %.3e  flagged %s  info %s" % (bound, flagged.tolist(), info1))
    assert info1 == {"n_strict_reeval": len(flagged), "second_pass": True} and set(planted) <= set(flagged.tolist())
    assert np.array_equal(bits(s1)[flagged], bits(want_s)[flagged]) and np.array_equal(n1, want_n)
    assert np.array_equal(s1.astype(np.int64), want_s.astype(np.int64))
    assert info2 == info1 and np.array_equal(bits(s2), bits(s1)) and np.array_equal(n2, n1)
    assert info3 == {"n_strict_reeval": 0, "second_pass": False}
    assert np.array_equal(bits(s3), bits(want_s)) and np.array_equal(n3, want_n)
    assert info4 == info1 and np.array_equal(bits(s4), bits(s1)) and np.array_equal(n4, n1)
    assert info5 == info1 and np.array_equal(bits(s5), bits(s1)) and np.array_equal(n5, n1)
    assert np.array_equal(bits(t_score[:n_acc]), bits(s5)) and np.array_equal(t_ninfo[:n_acc], n5)
    assert np.array_equal(bits(t_score[:n_acc])[flagged], bits(want_s)[flagged]) and np.array_equal(t_ninfo[:n_acc], want_n)
    assert np.array_equal(bits(t_score[n_acc:]), bits(np.full(pad, sent_f))), t_score[n_acc:]
    assert np.array_equal(t_ninfo[n_acc:], np.full(pad, sent_i, dtype=np.int64)), t_ninfo[n_acc:]


# ------------------------------------------------------------------------------------------- 5. one-chunk and one-row slabs
@pytest.mark.parametrize("packed", FORMATS)
def test_one_chunk_slabs_and_a_slab_of_one_row(packed):
    """slabs of exactly one chunk and a last slab of a single row, three forced accessions: they carry the oracle's bits over all
    2001 rows, the counts are exact and every other total truncates to the oracle's integer"""
    n, n_acc, slabs, chunk = 2001, 70, (1000, 1000, 1), 1000
    db, wei, want_s, want_n = job_data("random", n, n_acc, chunk, False, 500)
    with context(SNPM_DEBUG_REEVAL=3) as ctx:
        sc = slab_scorer(ctx, db, wei, slabs, chunk, False, packed)
        s, ninfo, info = sc.run(engine.MODE_EXACT)
        bound = sc.carry.error_bound()
        sc.free()
    print("bound %.3e  info %s" % (bound, info))
    assert info["second_pass"] is True and 3 <= info["n_strict_reeval"] <= CAP
    assert np.array_equal(ninfo, want_n)
    assert np.array_equal(bits(s)[:3], bits(want_s)[:3])
    assert np.array_equal(s.astype(np.int64), want_s.astype(np.int64))
