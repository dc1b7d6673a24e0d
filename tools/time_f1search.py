#!/usr/bin/env python3
"""
Time ``engine.f1_counts`` (the in-silico F1 of every pair of accessions of a resident panel against one sample's hard calls) at the
shape of a 1001-Genomes identification: 1135 accessions x 200k matched rows (an unsorted row list, as ``get_positions_idxs`` gives
it), on an int8 and on a packed panel of 1M rows.

Panels are the library's synthetic panel (``Panel.fill_synthetic``); the sample's classes are drawn from a seed.  Reported per
shape, one JSON line: the two kernels (``k_win_planes``, ``k_f1x_count``; HIP events), the whole call (host arrays out, validation,
masks and copies included), and as the yardstick ``k_kin_count`` over the SAME selection in the same run (``engine.kinship_counts``:
three planes and 10 operations per pair and dword against five planes and 14) with the ratio of the two count kernels.  Compared
with, on the same values: the numpy twin (tests/f1search_twin.py) on the first ``--twin-rows`` selected rows, scaled by rows (the
subsample is stated in the output; the device's counts of those rows must equal the twin's).

    python tools/time_f1search.py [--reps 5] [--shape int8|packed|all] [--out profiles/time_f1search.txt]

``--host-only``: only the twin, on a machine without a GPU.
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

import f1search_twin  # noqa: E402

TILE, PL_COLS, STEP_ROWS = 32, 64, 1024         # F1X_TILE, F1X_PL_COLS, F1X_STEP_WORDS * 64
SEED = 1001


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shape", default="all", choices=["int8", "packed", "all"])
    ap.add_argument("--panel-rows", type=int, default=1000000)
    ap.add_argument("--rows", type=int, default=200000, help="matched rows: a sorted random subset of the panel's rows, as a row list")
    ap.add_argument("--accessions", type=int, default=1135)
    ap.add_argument("--twin-rows", type=int, default=10000)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from snpmatch_amd import engine, synth
    ctx = None if args.host_only else engine.default_context()
    rng = np.random.default_rng(SEED)
    rows = np.sort(rng.choice(args.panel_rows, size=args.rows, replace=False)).astype(np.int64)
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
        want = f1search_twin.f1_counts(values, classes[:k], None, rows[:k])
        twin_s = time.perf_counter() - t0
        line = {"shape": name, "accessions": n_acc, "rows": n_rows, "panel_rows": args.panel_rows, "packed": packed, "numpy_twin_rows": k,
                "numpy_twin_s": round(twin_s, 2), "numpy_twin_scaled_to_all_rows_s": round(twin_s * n_rows / k, 1)}
        if ctx is None:
            line["device"] = "not measured"
        else:
            panel = engine.Panel(ctx, args.panel_rows, n_acc, packed=packed)
            panel.fill_synthetic(SEED)
            got = engine.f1_counts(panel, classes[:k], rows=rows[:k])                # warm-up: workspaces, code object; and the check
            same = all(np.array_equal(g, w) for g, w in zip(got, want))
            ok &= same
            engine.f1_counts(panel, classes, rows=rows)
            engine.kinship_counts(panel, rows=rows)
            ctx.profile(True)
            ctx.profile_reset()
            f1_calls, kin_calls = [], []
            for _ in range(args.reps):                                               # the two scans alternate
                t0 = time.perf_counter()
                engine.f1_counts(panel, classes, rows=rows)
                f1_calls.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                engine.kinship_counts(panel, rows=rows)
                kin_calls.append(time.perf_counter() - t0)
            n_p, ms_p = ctx.profile_read("win_planes")
            n_c, ms_c = ctx.profile_read("f1x_count")
            n_kp, ms_kp = ctx.profile_read("kin_planes")
            n_kc, ms_kc = ctx.profile_read("kin_count")
            ctx.profile(False)
            p_ms, c_ms, kp_ms, kc_ms = (v / args.reps for v in (ms_p, ms_c, ms_kp, ms_kc))
            pair_rows = float(n_acc) * n_acc * n_rows
            tiles = -(-n_acc // TILE)
            tile_pair_rows = float(tiles * (tiles + 1) // 2) * TILE * TILE * (-(-n_rows // STEP_ROWS) * STEP_ROWS)      # what the blocks compute
            line.update({"reps": args.reps, "slabs": n_p // args.reps, "planes_ms": round(p_ms, 3), "count_ms": round(c_ms, 3),
                         "count_pair_rows_per_s": round(pair_rows / (c_ms / 1e3), 0) if c_ms else None,
                         "count_computed_pair_rows_per_s": round(tile_pair_rows / (c_ms / 1e3), 0) if c_ms else None,
                         "call_ms_median": round(float(np.median(f1_calls)) * 1e3, 2), "call_ms_min": round(min(f1_calls) * 1e3, 2),
                         "kin_planes_ms": round(kp_ms, 3), "kin_count_ms": round(kc_ms, 3), "kin_slabs": n_kp // args.reps,
                         "kin_call_ms_median": round(float(np.median(kin_calls)) * 1e3, 2),
                         "count_over_kin_count": round(c_ms / kc_ms, 3) if kc_ms else None,
                         "call_bytes_to_host": 8 * n_acc * n_acc, "counts_equal_twin_on_subsample": bool(same)})
            assert n_c == n_p and n_kc == n_kp
            panel.free()
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
