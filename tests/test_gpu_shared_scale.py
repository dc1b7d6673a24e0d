"""
The shared-row scan (snpmatch_amd/csrc/snpm_k_shared.hpp) at the shapes its numbers are quoted on and at the edges of its
fixed-point contraction (-m gpu).  test_gpu_shared.py covers small panels with forced row-tile counts; here:

  A  64 samples of ~194k markers against 1135 x 11M resident (tools/bench_real_panel.py's chip batch) under the AUTOMATIC
     policy: 5 digits, 36 row tiles with filler tiles; every sample against the C oracle on the numpy twin of the batch's
     union, forced re-evaluations carry the reference's bits; coded weights from host memory give the same bits;
  B  64 samples of > 2^18 markers against 10 000 x 1.5M: the automatic 6-digit rule, four groups of 128 matrix rows, two
     passes over groups; against the per-sample pass and the C oracle on accession quads;
  C  hard-call (0 / 1) batches: integer weights quantise exactly, so the certificate flags no pair (the per-sample pass does
     not either); a hard-call sample adds nothing to a mixed batch's pair count;
  D  a NaN / infinite het weight under skip_hets is refused by every pass, as any other non-finite weight is;
  E  a forced row-tile count over a 20M-row union: a tile keeps at most 2^23 rows, or its int32 digit sums wrap.

Reference: one `Genotyper.genotyper` run per sample (core/snpmatch.py:207-233, the chunk loop :218-225).
"""
import math

import numpy as np
import pytest

from oracle import c_oracle
from oracle import snpmatch_oracle as orc
from snpmatch_amd import engine, synth
from test_gpu_shared import LIK_RTOL, chip_samples, make_ctx, rand_db, sample_on

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
TWIN_BLOCK = 50_000


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def frac_bits(digits):
    return 8 * (digits - 1) + 6


def twin_rows(seed, rows, acc0, n_acc):
    """synth.panel_rows in row blocks (host memory: the hash array of a block is 8 B per accession quad and row)"""
    return np.concatenate([synth.panel_rows(seed, rows[r0:r0 + TWIN_BLOCK], acc0, n_acc) for r0 in range(0, len(rows), TWIN_BLOCK)])


def on_device(samples):
    """the concatenated batch in HBM: (tensors to keep alive, score_batch's device= triple)"""
    import torch
    off = np.concatenate([[0], np.cumsum([len(r) for r, _ in samples])]).astype(np.int64)
    d_rows = torch.as_tensor(np.concatenate([r for r, _ in samples]), device="cuda:0")
    d_wei = torch.as_tensor(np.concatenate([w for _, w in samples]), device="cuda:0")
    torch.cuda.synchronize()
    return (d_rows, d_wei), (d_rows.data_ptr(), d_wei.data_ptr(), off)


def oracle_runs(db, samples, skip, chunk=1000):
    return [c_oracle.genotyper(db, rows, wei, chunk, skip) for rows, wei in samples]


def assert_parity(want, got, samples, digits, reeval=0, lik=True, chunk=1000, cols=slice(None)):
    """test_gpu_shared.check_against_oracle on oracle results computed once (want[b] = (score, ninfo) over the accessions
    `cols` of the results), plus the fp64 bits of the accessions 0 .. reeval-1 that SNPM_DEBUG_REEVAL sends through the
    reference-order re-evaluation.  An unflagged score is the fixed-point sum: below the exact sum by at most 2^-F per matched
    SNP; the reference's own fp64 sum is off the exact one by at most (chunk + K) u times itself (K chunks of recursive
    summation of non-negative terms) -- far below the quantisation on small samples, 5e-7 on a 20M-row one."""
    for b, ((rows, _), (ws, wn)) in enumerate(zip(samples, want)):
        gs, gn = got["score"][b][cols], got["ninfo"][b][cols]
        assert np.array_equal(gn, wn), b
        assert np.array_equal(gs.astype(np.int64), ws.astype(np.int64)), b
        n = len(rows)
        ref_order = (chunk + -(-n // chunk) + 3) * U * 1.01 * np.abs(ws)
        assert np.all(np.abs(gs - ws) < 1e-7 + n * 2.0 ** -frac_bits(digits) + ref_order), b
        if reeval:
            assert np.array_equal(bits(gs[:reeval]), bits(ws[:reeval])), b
        if lik:
            wl, wr = orc.calculate_likelihoods(np.array(ws, dtype=np.int64), wn)
            np.testing.assert_allclose(got["lik"][b][cols], wl, rtol=LIK_RTOL, equal_nan=True)
            np.testing.assert_allclose(got["lrt"][b][cols], wr, rtol=LIK_RTOL, equal_nan=True)


def sh_digits(x, digits):
    """numpy model of k_sh_expand's balanced digits of one weight, top digit first: Q' = floor(x 2^F) + sum_{p < D-1} 128 * 256^p,
    digit at byte position p < D-1 = byte p of Q' - 128, top digit = Q' >> 8 (D - 1)"""
    q = int(np.floor(x * 2.0 ** frac_bits(digits))) + sum(128 << (8 * p) for p in range(digits - 1))
    return [q >> (8 * (digits - 1))] + [((q >> (8 * p)) & 255) - 128 for p in range(digits - 2, -1, -1)]


# ---------------------------------------------------------------------------------------------------------------------------
# A: the quoted shape
QUOTED = {}
A_SEED, A_SNP, A_ACC, A_MARKERS, A_PLANTED = 1001, 11_000_000, 1135, 200_000, 417


def quoted_batch():
    """tools/bench_real_panel.py's chip batch: 64 samples on ONE set of 200k markers, each lacking 3 % of it, planted accessions
    (2 % error, 80 % PL weights); sample 0 a perfect PL match of accession 417 (an exact-integer score).  With the numpy twin
    of the union's rows and every sample's rows remapped into it; built once for both formats."""
    if not QUOTED:
        rng = np.random.default_rng(5)
        base = np.sort(rng.choice(A_SNP, size=A_MARKERS, replace=False)).astype(np.int64)
        samples, accs = [], []
        for b in range(64):
            rows = base[rng.random(A_MARKERS) >= 0.03]
            acc = A_PLANTED if b == 0 else (b * 11) % A_ACC
            col = synth.panel_rows(A_SEED, rows, acc // 4 * 4, 4)[:, acc % 4]
            if b == 0:
                codes = col.copy()
                codes[codes < 0] = 0
                wei = synth.sample_weights(rng, codes, frac_pl=1.0)
            else:
                wei = synth.planted_sample(rng, col, 0.02)[1]
            samples.append((rows, wei))
            accs.append(acc)
        union = np.unique(np.concatenate([r for r, _ in samples]))
        QUOTED.update(samples=samples, accs=accs, union=union, twin=twin_rows(A_SEED, union, 0, A_ACC),
                      remapped=[(np.searchsorted(union, r), w) for r, w in samples])
    return QUOTED


def quoted_oracle(skip):
    q = quoted_batch()
    if ("want", skip) not in q:
        q[("want", skip)] = oracle_runs(q["twin"], q["remapped"], skip)
    return q[("want", skip)]


@pytest.mark.parametrize("packed", [False, True])
def test_quoted_shape_64_samples_on_one_marker_set_against_1135_x_11M(packed):
    q = quoted_batch()
    samples = q["samples"]
    assert 193_000 <= min(len(r) for r, _ in samples) and max(len(r) for r, _ in samples) <= 200_000
    ctx = make_ctx(SNPM_DEBUG_REEVAL=2)
    try:
        panel = engine.Panel(ctx, A_SNP, A_ACC, packed=packed)
        panel.fill_synthetic(A_SEED)
        keep, dev = on_device(samples)
        got = engine.score_batch(panel, None, 1000, False, engine.MODE_EXACT, device=dev)
        st = engine.batch_last_stats(ctx)
        assert got["shared_rows"] and st["taken"] and st["digits"] == 5, st
        # 36 row tiles planned for this shape (32 aligned + 4 filler tiles on the CUs the aligned ones leave idle)
        assert st["row_tiles"] > 8 and st["row_tiles"] % 8 != 0, "planned %d row tiles: %s" % (st["row_tiles"], st)
        assert st["union_rows"] == len(q["union"]) and not got["strict_fallback"], (st, got["pairs_reeval"])
        assert got["pairs_reeval"] >= 2 * 64
        assert_parity(quoted_oracle(False), got, samples, 5, reeval=2)
        assert [int(np.nanargmin(got["lik"][b])) for b in range(64)] == q["accs"]
        # the same batch as dictionary codes of exp(-PL / 10) from host memory: the digits come from the table's values, the bits
        # of every result are those of the device-input run
        table = engine.pl_table(7460)
        codes = engine.weight_codes(np.concatenate([w for _, w in samples]), table)
        assert codes is not None
        off = np.cumsum([0] + [len(r) for r, _ in samples])
        coded = [(r, codes[off[b]:off[b + 1]]) for b, (r, _) in enumerate(samples)]
        engine.batch_configure(ctx, shared_rows=1)
        cg = engine.score_batch(panel, coded, 1000, False, engine.MODE_EXACT, table=table)
        assert cg["shared_rows"] and engine.batch_last_stats(ctx)["taken"]
        assert cg["pairs_reeval"] == got["pairs_reeval"]
        for k in ("score", "ninfo", "lik", "lrt"):
            assert np.array_equal(np.ascontiguousarray(cg[k]).view(np.uint64), np.ascontiguousarray(got[k]).view(np.uint64)), k
        engine.batch_configure(ctx, shared_rows=-1)
        if not packed:
            # skip_hets: the het class has neither weight digits nor a count
            sk = engine.score_batch(panel, None, 1000, True, engine.MODE_EXACT, device=dev)
            st = engine.batch_last_stats(ctx)
            assert sk["shared_rows"] and st["taken"] and st["digits"] == 5 and not sk["strict_fallback"], st
            assert_parity(quoted_oracle(True), sk, samples, 5, reeval=2)
        del keep
        panel.free()
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------
# B: the automatic 6-digit rule, several groups and passes, a wide panel
B_SEED, B_SNP, B_ACC, B_MARKERS = 2024, 1_500_000, 10_000, 320_000


def test_six_digits_four_groups_two_passes_against_10000_x_1_5M():
    """the longest sample is above 2^18 rows: 6 digits + the count row = 7 matrix rows per sample, 64 samples = 448 rows = four
    groups of 128 (sample 18 lies across the first two); a 256-MB digit-matrix budget holds two groups (123 MB each): two passes"""
    rng = np.random.default_rng(6)
    base = np.sort(rng.choice(B_SNP, size=B_MARKERS, replace=False)).astype(np.int64)
    samples, accs = [], []
    for b in range(64):
        rows = base[rng.random(B_MARKERS) >= 0.03]
        acc = 417 if b == 0 else (b * 157) % B_ACC
        col = synth.panel_rows(B_SEED, rows, acc // 4 * 4, 4)[:, acc % 4]
        samples.append((rows, synth.planted_sample(rng, col, 0.02)[1]))
        accs.append(acc)
    assert max(len(r) for r, _ in samples) > (1 << 18)
    ctx = make_ctx(SNPM_SHARED_WS_MB=256)
    try:
        panel = engine.Panel(ctx, B_SNP, B_ACC)
        panel.fill_synthetic(B_SEED)
        keep, dev = on_device(samples)
        got = engine.score_batch(panel, None, 1000, False, engine.MODE_EXACT, device=dev)
        st = engine.batch_last_stats(ctx)
        assert got["shared_rows"] and st["taken"] and not got["strict_fallback"], st
        assert st["digits"] == 6 and st["groups"] >= 4 and st["passes"] >= 2, st
        assert [int(np.nanargmin(got["lik"][b])) for b in range(64)] == accs
        # the per-sample pass on the same context
        engine.batch_configure(ctx, shared_rows=0)
        seg = engine.score_batch(panel, None, 1000, False, engine.MODE_EXACT, device=dev)
        engine.batch_configure(ctx, shared_rows=-1)
        assert not seg["shared_rows"]
        assert np.array_equal(seg["ninfo"], got["ninfo"])
        assert np.array_equal(seg["score"].astype(np.int64), got["score"].astype(np.int64))
        np.testing.assert_allclose(seg["lik"], got["lik"], rtol=LIK_RTOL, equal_nan=True)
        del keep
        panel.free()
    finally:
        ctx.close()
    # the C oracle on accession quads of the twin (a score depends on its own column only): both ends of the panel, the edges of
    # the 128-accession wave tiles, every planted accession
    union = np.unique(np.concatenate([r for r, _ in samples]))
    quads = sorted({0, 124, 128, 4996, 9996} | {a // 4 * 4 for a in accs})
    twin = np.concatenate([twin_rows(B_SEED, union, c4, 4) for c4 in quads], axis=1)
    cols = np.concatenate([np.arange(c4, c4 + 4) for c4 in quads])
    remapped = [(np.searchsorted(union, r), w) for r, w in samples]
    assert_parity(oracle_runs(twin, remapped, False), got, samples, 6, lik=False, cols=cols)


# ---------------------------------------------------------------------------------------------------------------------------
# C: hard-call batches
def hard_samples(rng, db, count, n_markers, drop=0.03):
    """GT-only samples (weights 0 / 1, core/parsers.py:132-139) on one marker set, each planted on a random accession"""
    base = np.sort(rng.choice(db.shape[0], size=n_markers, replace=False)).astype(np.int64)
    out = []
    for b in range(count):
        rows = base[rng.random(n_markers) >= drop]
        codes = db[rows, int(rng.integers(0, db.shape[1]))].copy()
        codes[codes < 0] = 0
        out.append((rows, orc.weights_from_gt_codes(codes)))
    return out


def test_hard_call_batches_flag_no_pair():
    """integer weights quantise exactly (Q = 0 or 2^F), the digit sums are exact integers and so is their fp64 form: no
    (sample, accession) pair is unproven, whichever way the batch arrives, and the score is the reference's fp64 bit for bit"""
    rng = np.random.default_rng(15)
    n_snp, n_acc = 100_000, 1135
    db = rand_db(rng, n_snp, n_acc)
    samples = hard_samples(rng, db, 64, 20_000)
    want = oracle_runs(db, samples, False)
    table = engine.pl_table(7460)
    assert table[0] == 1.0 and table[7459] == 0.0
    coded = [(r, np.where(w == 1.0, 0, 7459).astype(np.uint16)) for r, w in samples]
    ctx = make_ctx()
    try:
        panel = engine.Panel.from_host(ctx, db)
        keep, dev = on_device(samples)
        runs = {}
        engine.batch_configure(ctx, shared_rows=1)
        runs["forced, host"] = engine.score_batch(panel, samples, 1000, False, engine.MODE_EXACT)
        runs["coded, host"] = engine.score_batch(panel, coded, 1000, False, engine.MODE_EXACT, table=table)
        engine.batch_configure(ctx, shared_rows=-1)
        runs["automatic, device"] = engine.score_batch(panel, None, 1000, False, engine.MODE_EXACT, device=dev)
        engine.batch_configure(ctx, shared_rows=0)
        seg = engine.score_batch(panel, samples, 1000, False, engine.MODE_EXACT)
        assert not seg["shared_rows"] and seg["pairs_reeval"] == 0 and not seg["strict_fallback"]
        runs["per-sample pass"] = seg
        for name, got in runs.items():
            assert got["shared_rows"] == (name != "per-sample pass"), name
            assert got["pairs_reeval"] == 0 and not got["strict_fallback"], (name, got["pairs_reeval"], got["strict_fallback"])
            for b, (ws, wn) in enumerate(want):
                assert np.array_equal(got["ninfo"][b], wn), (name, b)
                assert np.array_equal(bits(got["score"][b]), bits(ws)), (name, b)
        # mixed: the certificate is per pair, so 32 hard-call samples beside 32 PL ones (every other one a perfect PL match: an
        # exact-integer score that is flagged) add nothing to the PL samples' count
        pl = [(r, sample_on(rng, db, r, 0 if b % 2 else 2)) for b, (r, _) in enumerate(samples[32:])]
        mixed = [s for pair in zip(samples[:32], pl) for s in pair]
        engine.batch_configure(ctx, shared_rows=1, digits=5)
        alone = engine.score_batch(panel, pl, 1000, False, engine.MODE_EXACT)
        got = engine.score_batch(panel, mixed, 1000, False, engine.MODE_EXACT)
        st = engine.batch_last_stats(ctx)
        assert alone["shared_rows"] and got["shared_rows"] and st["taken"] and st["digits"] == 5, st
        assert alone["pairs_reeval"] >= 16 and not alone["strict_fallback"]
        assert got["pairs_reeval"] == alone["pairs_reeval"] and not got["strict_fallback"], (got["pairs_reeval"], alone["pairs_reeval"])
        want_pl = oracle_runs(db, pl, False)
        assert_parity([w for pair in zip(want[:32], want_pl) for w in pair], got, mixed, 5)
        for b in range(0, 64, 2):
            assert np.array_equal(bits(got["score"][b]), bits(want[b // 2][0])), b
        del keep
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------
# D: a non-finite het weight under skip_hets
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_het_weight_is_refused_under_skip_hets(bad):
    """skip_hets ignores the het class, not the het weight's validity: the per-sample pass refuses a non-finite weight in any
    column (the reference's 0 * NaN is NaN), and so must the shared-row pass, which reads the het weight as W[:, 1]"""
    assert orc.weights_from_gt_codes(np.array([2], dtype=np.int8)).tolist() == [[0.0, 1.0, 0.0]]      # column 1 = het
    rng = np.random.default_rng(21)
    n_snp, n_acc = 30_000, 300
    db = rand_db(rng, n_snp, n_acc)
    samples = chip_samples(rng, db, 8, 4000)
    ctx = make_ctx()
    try:
        panel = engine.Panel.from_host(ctx, db)
        keep, dev = on_device(samples)
        ok = engine.score_batch(panel, None, 1000, True, engine.MODE_EXACT, device=dev)         # the automatic policy takes it
        assert ok["shared_rows"], engine.batch_last_stats(ctx)
        rows, wei = samples[3]
        wei = wei.copy()
        wei[len(rows) // 2, 1] = bad
        broken = list(samples)
        broken[3] = (rows, wei)
        keep_b, dev_b = on_device(broken)
        engine.batch_configure(ctx, shared_rows=1)
        with pytest.raises(AssertionError, match="finite"):
            engine.score_batch(panel, broken, 1000, True, engine.MODE_EXACT)
        engine.batch_configure(ctx, shared_rows=-1)
        with pytest.raises(AssertionError, match="finite"):
            engine.score_batch(panel, None, 1000, True, engine.MODE_EXACT, device=dev_b)
        engine.batch_configure(ctx, shared_rows=0)
        with pytest.raises(AssertionError, match="finite"):
            engine.score_batch(panel, broken, 1000, True, engine.MODE_EXACT)
        # the context goes on: the finite batch again, through the shared-row pass
        engine.batch_configure(ctx, shared_rows=-1)
        again = engine.score_batch(panel, None, 1000, True, engine.MODE_EXACT, device=dev)
        assert again["shared_rows"]
        for k in ("score", "ninfo", "lik", "lrt"):
            assert np.array_equal(np.ascontiguousarray(again[k]).view(np.uint64), np.ascontiguousarray(ok[k]).view(np.uint64)), k
        assert_parity(oracle_runs(db, samples, True), again, samples, 5)
        del keep, keep_b
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------
# E: a forced row-tile count over a large union
def test_forced_tile_count_keeps_tiles_within_int32_digit_sums():
    """every class weight x = 0x207F7F7F7F7F 2^-46: under 6 digits each lower digit is +127 and the top one 32, so a tile's int32
    sum of a lower digit over 20M informative rows (2.54e9) would wrap; 2^23 rows (1.07e9) do not.  SNPM_SHARED_TILES=1 asks for
    one tile: the plan takes as many as keep a tile within 2^23 rows"""
    x = 0x207F7F7F7F7F / 2.0 ** 46
    assert sh_digits(x, 6) == [32, 127, 127, 127, 127, 127]
    assert sum(d * 256 ** (5 - j) for j, d in enumerate(sh_digits(x, 6))) == int(x * 2.0 ** 46)
    n_snp, n_acc = 20_000_000, 8
    assert n_snp * 127 > 2 ** 31 - 1 and (1 << 23) * 128 <= 2 ** 31 - 1
    rng = np.random.default_rng(23)
    db = rng.integers(0, 3, size=(n_snp, n_acc), dtype=np.int8)            # codes 0..2 only: every call is informative
    all_rows = np.arange(n_snp, dtype=np.int64)
    sub = np.flatnonzero(rng.random(n_snp) < 0.85).astype(np.int64)       # ~17M rows
    samples = [(all_rows, np.full((n_snp, 3), x)), (sub, synth.planted_sample(rng, db[sub, 5], 0.02)[1])]
    ctx = make_ctx(SNPM_SHARED_TILES=1)
    try:
        panel = engine.Panel.from_host(ctx, db)
        engine.batch_configure(ctx, shared_rows=1, digits=6)
        got = engine.score_batch(panel, samples, 1000, False, engine.MODE_EXACT)
        st = engine.batch_last_stats(ctx)
        assert got["shared_rows"] and st["taken"] and st["digits"] == 6 and st["union_rows"] == n_snp, st
        assert st["row_tiles"] >= math.ceil(n_snp / 2 ** 23), st
        panel.free()
    finally:
        ctx.close()
    assert_parity(oracle_runs(db, samples, False), got, samples, 6)
    assert np.array_equal(got["ninfo"][0], np.full(n_acc, n_snp))
    assert int(np.nanargmin(got["lik"][1])) == 5
