#!/usr/bin/env python3
"""
Time ``engine.pair_counts`` (pairsnp for every pair of a cohort in one device call) at two shapes:

  cohort   384 samples x 1M records on five chromosomes, about 3 % of the calls absent: 384 x 384 x 1M = 1.5e11 byte comparisons
           (every ordered pair; the kernel computes the upper triangle of 32 x 32 tiles and mirrors it)
  pair     2 samples x 5M records: the two-file command, one pair split over the record axis

Reported per shape: the two kernels (``k_pair_transpose``, ``k_pair_count``; HIP events) with the bytes each moves and the byte
comparisons per second, and the whole call (host arrays in, host arrays out: validation and copies included).  Compared with, on
the same inputs on the same machine: for the cohort the numpy twin (tests/pairsnp_twin.py) on the first ``--twin-samples`` samples,
scaled by the number of unordered pairs (the subsample is stated in the output; the device's counts of those samples must equal the
twin's); for the pair the work of the reference's loop -- one comparison of two genotype TEXT arrays per chromosome
(core/snpmatch.py:293-300) -- on the texts the ids stand for.  One JSON line per shape.

    python tools/time_pairsnp.py [--reps 5] [--shape cohort|pair|both]

``--host-only``: only the two comparisons (numpy twin on the subsample, text loop), on a machine without a GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pairsnp_twin  # noqa: E402

TILE, CHUNK, TR_SAMPLES = 32, 4096, 64          # PR_TILE, PR_CHUNK, PR_TR_SAMPLES of csrc/snpm_k_pairs.hpp
TEXTS = np.array(["", "0/0", "1/1", "0/1", "1/0"])


def make_ids(n, ns, n_seg, seed):
    """ids 1..4 with 1 in 33 calls absent; segment sizes in the proportions of TAIR10's chromosomes"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 33, size=(n, ns), dtype=np.uint8)
    ids = np.where(v == 0, 0, (v - 1) % 4 + 1).astype(np.uint8)
    share = np.array([30.4, 19.7, 23.5, 18.6, 27.0][:n_seg])
    sizes = np.floor(share / share.sum() * n).astype(np.int64)
    sizes[-1] = n - sizes[:-1].sum()
    return ids, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def timed(ctx, engine, ids, seg_off, reps):
    out = engine.pair_counts(ctx, ids, seg_off)                       # warm-up: workspaces, code object
    ctx.profile(True)
    ctx.profile_reset()
    calls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        engine.pair_counts(ctx, ids, seg_off)
        calls.append(time.perf_counter() - t0)
    n_t, ms_t = ctx.profile_read("pairs_t")
    n_c, ms_c = ctx.profile_read("pairs_c")
    ctx.profile(False)
    return out, ms_t / max(n_t, 1) / 1e3, ms_c / max(n_c, 1) / 1e3, calls


def report(name, ids, seg_off, out, t_s, c_s, calls, extra):
    n, ns = ids.shape
    pitch = (ns + TR_SAMPLES - 1) // TR_SAMPLES * TR_SAMPLES
    n_pad = int(sum(-(-int(k) // CHUNK) for k in np.diff(seg_off))) * CHUNK
    tiles = -(-ns // TILE)
    tile_pairs = tiles * (tiles + 1) // 2
    cells = (len(seg_off) - 1) * ns * ns
    transpose_bytes = n * ns + pitch * n_pad                         # packed rows read, planes written
    # a block reads the chunk of its two tiles (one on the diagonal); the planes are read tile_pairs-fold, mostly from cache
    count_bytes = n_pad * TILE * (2 * tile_pairs - tiles)
    compares = float(ns) * ns * n
    call_s = float(np.median(calls))
    line = {"shape": name, "samples": ns, "records": n, "segments": len(seg_off) - 1, "reps": len(calls),
            "transpose_ms": round(t_s * 1e3, 3), "transpose_bytes": transpose_bytes,
            "transpose_GBps": round(transpose_bytes / t_s / 1e9, 1) if t_s else None,
            "count_ms": round(c_s * 1e3, 3), "count_bytes_requested": count_bytes,
            "count_GBps_requested": round(count_bytes / c_s / 1e9, 1) if c_s else None,
            "byte_comparisons": compares, "count_comparisons_per_s": round(compares / c_s, 0) if c_s else None,
            "kernels_comparisons_per_s": round(compares / (c_s + t_s), 0) if c_s + t_s else None,
            "call_ms_median": round(call_s * 1e3, 2), "call_ms_min": round(min(calls) * 1e3, 2),
            "call_bytes": n * ns + 8 * cells, "call_comparisons_per_s": round(compares / call_s, 0)}
    line.update(extra)
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shape", default="both", choices=["cohort", "pair", "both"])
    ap.add_argument("--samples", type=int, default=384)
    ap.add_argument("--records", type=int, default=1000000)
    ap.add_argument("--pair-records", type=int, default=5000000)
    ap.add_argument("--twin-samples", type=int, default=6)
    ap.add_argument("--host-only", action="store_true")
    args = ap.parse_args()
    from snpmatch_amd import engine
    ctx = None if args.host_only else engine.default_context()
    ok = True
    if args.shape in ("cohort", "both"):
        ids, seg_off = make_ids(args.records, args.samples, 5, 17)
        k = min(args.twin_samples, args.samples)
        t0 = time.perf_counter()
        want = pairsnp_twin.pair_counts(np.ascontiguousarray(ids[:, :k]), seg_off)
        twin_s = time.perf_counter() - t0
        pairs_all, pairs_sub = args.samples * (args.samples + 1) // 2, k * (k + 1) // 2
        if ctx is None:
            print(json.dumps({"shape": "cohort", "samples": args.samples, "records": args.records, "device": "not measured",
                              "numpy_twin_samples": k, "numpy_twin_pairs": pairs_sub, "numpy_twin_s": round(twin_s, 2),
                              "numpy_twin_scaled_to_all_pairs_s": round(twin_s * pairs_all / pairs_sub, 1)}), flush=True)
            ids = None
    if ctx is not None and args.shape in ("cohort", "both"):
        out, t_s, c_s, calls = timed(ctx, engine, ids, seg_off, args.reps)
        same = bool(np.array_equal(out[0][:, :k, :k], want[0]) and np.array_equal(out[1][:, :k, :k], want[1]))
        ok &= same
        report("cohort", ids, seg_off, out, t_s, c_s, calls, {
            "numpy_twin_samples": k, "numpy_twin_pairs": pairs_sub, "numpy_twin_s": round(twin_s, 2),
            "numpy_twin_scaled_to_all_pairs_s": round(twin_s * pairs_all / pairs_sub, 1), "counts_equal_twin_on_subsample": same})
        del ids, out
    if args.shape in ("pair", "both"):
        ids, seg_off = make_ids(args.pair_records, 2, 5, 18)
        present = np.flatnonzero((ids[:, 0] != 0) & (ids[:, 1] != 0))       # the common rows, as the command hands them over
        ids = np.ascontiguousarray(ids[present])
        seg_off = np.searchsorted(present, seg_off).astype(np.int64)
        gt_a, gt_b = TEXTS[ids[:, 0]], TEXTS[ids[:, 1]]
        t0 = time.perf_counter()
        loop = [int(np.sum(np.array(gt_a[a:b] == gt_b[a:b], dtype=int))) for a, b in zip(seg_off[:-1], seg_off[1:])]
        loop_s = time.perf_counter() - t0
        if ctx is None:
            print(json.dumps({"shape": "pair", "samples": 2, "records": int(len(ids)), "device": "not measured",
                              "text_loop_per_chromosome_s": round(loop_s, 3)}), flush=True)
            return 0
        out, t_s, c_s, calls = timed(ctx, engine, ids, seg_off, args.reps)
        same = out[1][:, 0, 1].tolist() == loop and out[0][:, 0, 1].tolist() == np.diff(seg_off).tolist()
        ok &= same
        report("pair", ids, seg_off, out, t_s, c_s, calls, {"text_loop_per_chromosome_s": round(loop_s, 3), "counts_equal_text_loop": bool(same)})
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
