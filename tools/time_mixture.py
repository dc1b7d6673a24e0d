#!/usr/bin/env python3
"""
Time ``engine.mix_counts`` (the read-count-weighted 2 x 2 table of every ordered pair of accessions of a resident panel against one
sample's allele depths) at the shape of a 1001-Genomes identification: 1135 accessions x 200k matched rows (an unsorted row list, as
``get_positions_idxs`` gives it), on an int8 and on a packed panel of 1M rows.

Panels are the library's synthetic panel (``Panel.fill_synthetic``); the sample's read counts are drawn from a seed, once with a
largest count of 3, of 15 and of 255, so that the call takes ``k_mix_count`` at 2, 4 and 8 bit slices.  Reported per shape, one JSON
line: ``k_win_planes`` and ``k_mix_count`` per number of slices (HIP events), the whole call (host arrays out, validation, bit slices
and copies included), the host fit (``mixture.fit_pairs`` on the table, the default grid) and as the yardstick ``k_f1x_count`` over
the SAME selection in the same run (``engine.f1_counts``) with the ratio of each count kernel to it.  Compared with, on the same
values: the numpy twin (tests/mixture_twin.py) on the first ``--twin-rows`` selected rows, scaled by rows (the subsample is stated in
the output; the device's sums of those rows must equal the twin's).

    python tools/time_mixture.py [--reps 5] [--shape int8|packed|all] [--out profiles/time_mixture.txt]

``--host-only``: only the twin and the fit, on a machine without a GPU.
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

import mixture_twin  # noqa: E402

SEED = 1001
LARGEST = ((2, 3), (4, 15), (8, 255))           # (bit slices, largest count)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shape", default="all", choices=["int8", "packed", "all"])
    ap.add_argument("--panel-rows", type=int, default=1000000)
    ap.add_argument("--rows", type=int, default=200000, help="matched rows: a sorted random subset of the panel's rows, as a row list")
    ap.add_argument("--accessions", type=int, default=1135)
    ap.add_argument("--twin-rows", type=int, default=200)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from snpmatch_amd import engine, synth
    from snpmatch_amd.core import mixture
    ctx = None if args.host_only else engine.default_context()
    rng = np.random.default_rng(SEED)
    rows = np.sort(rng.choice(args.panel_rows, size=args.rows, replace=False)).astype(np.int64)
    reads = {}
    for bits, largest in LARGEST:                # Poisson-like low depth, clipped; the largest count present
        alt = np.minimum(rng.poisson(min(largest, 6) / 2.0, args.rows), largest).astype(np.uint8)
        ref = np.minimum(rng.poisson(min(largest, 6) / 2.0, args.rows), largest).astype(np.uint8)
        alt[-1] = largest
        reads[bits] = (alt, ref)
    classes = rng.choice(np.array([0, 1, 2, 0xFF], dtype=np.uint8), size=args.rows, p=[0.45, 0.35, 0.17, 0.03])
    n_acc, n_rows = args.accessions, args.rows
    ok = True
    for name, packed in (("int8", False), ("packed", True)):
        if args.shape not in ("all", name):
            continue
        # the twin on the first selected rows (they lie in the first stretch of the panel: only that stretch is generated)
        k = min(args.twin_rows, n_rows)
        values = synth.panel_values(SEED, 0, int(rows[k - 1]) + 1, 0, n_acc)
        t0 = time.perf_counter()
        want = mixture_twin.mix_counts(values, reads[4][0][:k], reads[4][1][:k], None, rows[:k])
        twin_s = time.perf_counter() - t0
        line = {"shape": name, "accessions": n_acc, "rows": n_rows, "panel_rows": args.panel_rows, "packed": packed, "numpy_twin_rows": k,
                "numpy_twin_s": round(twin_s, 2), "numpy_twin_scaled_to_all_rows_s": round(twin_s * n_rows / k, 1)}
        table = want
        if ctx is None:
            line["device"] = "not measured"
        else:
            panel = engine.Panel(ctx, args.panel_rows, n_acc, packed=packed)
            panel.fill_synthetic(SEED)
            got = engine.mix_counts(panel, reads[4][0][:k], reads[4][1][:k], rows=rows[:k])      # warm-up: workspaces, code object; and the check
            same = bool(np.array_equal(got, want))
            ok &= same
            for bits, _ in LARGEST:
                engine.mix_counts(panel, *reads[bits], rows=rows)
            engine.f1_counts(panel, classes, rows=rows)
            ctx.profile(True)
            per_bits = {}
            for bits, _ in LARGEST:                                                  # the two scans alternate
                ctx.profile_reset()
                mix_calls, f1_calls = [], []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    table = engine.mix_counts(panel, *reads[bits], rows=rows)
                    mix_calls.append(time.perf_counter() - t0)
                    t0 = time.perf_counter()
                    engine.f1_counts(panel, classes, rows=rows)
                    f1_calls.append(time.perf_counter() - t0)
                n_p, ms_p = ctx.profile_read("win_planes")
                n_c, ms_c = ctx.profile_read("mix_count")
                n_f, ms_f = ctx.profile_read("f1x_count")
                assert n_c == n_f == args.reps * (n_p // (2 * args.reps))
                c_ms, f_ms = ms_c / args.reps, ms_f / args.reps
                per_bits["bits%d" % bits] = {"count_ms": round(c_ms, 3), "f1x_count_ms": round(f_ms, 3), "count_over_f1x_count": round(c_ms / f_ms, 2) if f_ms else None,
                                             "planes_ms": round(ms_p / n_p, 3), "slabs": n_c // args.reps,
                                             "call_ms_median": round(float(np.median(mix_calls)) * 1e3, 2), "call_ms_min": round(min(mix_calls) * 1e3, 2),
                                             "f1_call_ms_median": round(float(np.median(f1_calls)) * 1e3, 2)}
            ctx.profile(False)
            line.update(per_bits)
            line.update({"reps": args.reps, "call_bytes_to_host": 32 * n_acc * n_acc, "sums_equal_twin_on_subsample": same})
            panel.free()
        t0 = time.perf_counter()
        fit = mixture.fit_pairs(table, mixture.ERR, mixture.alpha_grid(mixture.GRID))
        mixture.shortlist(fit)
        line["host_fit_s"] = round(time.perf_counter() - t0, 3)
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
