#!/usr/bin/env python3
"""
Time ``engine.sim_counts`` (the sample simulated from every accession of a resident panel scored against every accession, per group
of selected rows) at the shape of a 1001-Genomes power study: 1135 accessions x 200k selected rows in 4 groups (a ladder of 2k / 20k /
100k / 200k markers, sorted inside each group, as ``power.draw_ladder`` gives it), error rate 0.001, on an int8 and on a packed panel of
1M rows.

Panels are the library's synthetic panel (``Panel.fill_synthetic``).  Reported per shape, one JSON line: the three kernels
(``k_win_planes``, ``k_sim_noise``, ``k_sim_count``; HIP events), the whole call (host arrays out, validation and copies included), and as
the yardstick ``k_f1x_count`` over the SAME selection in the same run (``engine.f1_counts``: 16 operations per pair and dword on half
the square of pairs against about 7 on the full square) with the ratio of the two count kernels.  Compared with, on the same values:
the numpy twin (tests/power_twin.py) on the first ``--twin-rows`` selected rows, scaled by rows (the subsample is stated in the
output; the device's counts of those rows must equal the twin's).

    python tools/time_power.py [--reps 5] [--shape int8|packed|all] [--out profiles/time_power.txt]

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

import power_twin  # noqa: E402

TILE, STEP_ROWS = 32, 1024                      # F1X_TILE, F1X_STEP_WORDS * 64
SEED = 1001


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shape", default="all", choices=["int8", "packed", "all"])
    ap.add_argument("--panel-rows", type=int, default=1000000)
    ap.add_argument("--levels", default="2000,20000,100000,200000", help="the ladder: its last entry is the number of selected rows")
    ap.add_argument("--accessions", type=int, default=1135)
    ap.add_argument("--err-rate", type=float, default=0.001)
    ap.add_argument("--twin-rows", type=int, default=2000)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from snpmatch_amd import engine, synth
    from snpmatch_amd.core import power
    ctx = None if args.host_only else engine.default_context()
    levels = power.parse_levels(args.levels)
    rows, grp_off = power.draw_ladder(args.panel_rows, levels, np.random.default_rng(SEED))
    n_acc, n_rows = args.accessions, len(rows)
    classes = np.random.default_rng(SEED).choice(np.array([0, 1, 2, 0xFF], dtype=np.uint8), size=n_rows, p=[0.45, 0.35, 0.17, 0.03])
    ok = True
    for name, packed in (("int8", False), ("packed", True)):
        if args.shape not in ("all", name):
            continue
        # the twin on the selected rows that come first in the panel, in two groups (only that stretch of the panel is generated)
        k = min(args.twin_rows, n_rows)
        sub = np.sort(rows)[:k]
        values = synth.panel_values(SEED, 0, int(sub[-1]) + 1, 0, n_acc)
        t0 = time.perf_counter()
        want = power_twin.sim_counts(values, [0, k // 2, k], power_twin.err_threshold(args.err_rate), SEED, None, sub)
        twin_s = time.perf_counter() - t0
        line = {"shape": name, "accessions": n_acc, "rows": n_rows, "groups": len(levels), "err_rate": args.err_rate, "panel_rows": args.panel_rows,
                "packed": packed, "numpy_twin_rows": k, "numpy_twin_s": round(twin_s, 2), "numpy_twin_scaled_to_all_rows_s": round(twin_s * n_rows / k, 1)}
        if ctx is None:
            line["device"] = "not measured"
        else:
            panel = engine.Panel(ctx, args.panel_rows, n_acc, packed=packed)
            panel.fill_synthetic(SEED)
            got = engine.sim_counts(panel, [0, k // 2, k], args.err_rate, SEED, rows=sub)       # warm-up: workspaces, code object; and the check
            same = all(np.array_equal(g, w) for g, w in zip(got, want))
            ok &= same
            engine.sim_counts(panel, grp_off, args.err_rate, SEED, rows=rows)
            engine.f1_counts(panel, classes, rows=rows)
            ctx.profile(True)
            ctx.profile_reset()
            sim_calls, f1_calls = [], []
            for _ in range(args.reps):                                               # the two scans alternate
                t0 = time.perf_counter()
                engine.sim_counts(panel, grp_off, args.err_rate, SEED, rows=rows)
                sim_calls.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                engine.f1_counts(panel, classes, rows=rows)
                f1_calls.append(time.perf_counter() - t0)
            n_p, ms_p = ctx.profile_read("win_planes")                               # (of both scans: one launch per slab each)
            n_n, ms_n = ctx.profile_read("sim_noise")
            n_c, ms_c = ctx.profile_read("sim_count")
            n_f, ms_f = ctx.profile_read("f1x_count")
            ctx.profile(False)
            p_ms, n_ms, c_ms, f_ms = ms_p / max(n_p, 1) * (n_c / args.reps), ms_n / args.reps, ms_c / args.reps, ms_f / args.reps
            pair_rows = float(n_acc) * n_acc * n_rows
            tiles = -(-n_acc // TILE)
            tile_pair_rows = float(tiles * tiles) * TILE * TILE * (-(-n_rows // STEP_ROWS) * STEP_ROWS)      # what the blocks compute
            line.update({"reps": args.reps, "slabs": n_c // args.reps, "planes_ms": round(p_ms, 3), "noise_ms": round(n_ms, 3), "count_ms": round(c_ms, 3),
                         "count_pair_rows_per_s": round(pair_rows / (c_ms / 1e3), 0) if c_ms else None,
                         "count_computed_pair_rows_per_s": round(tile_pair_rows / (c_ms / 1e3), 0) if c_ms else None,
                         "call_ms_median": round(float(np.median(sim_calls)) * 1e3, 2), "call_ms_min": round(min(sim_calls) * 1e3, 2),
                         "f1x_count_ms": round(f_ms, 3), "f1x_slabs": n_f // args.reps, "f1x_call_ms_median": round(float(np.median(f1_calls)) * 1e3, 2),
                         "count_over_f1x_count": round(c_ms / f_ms, 3) if f_ms else None,
                         "call_bytes_to_host": 8 * len(levels) * n_acc * n_acc, "counts_equal_twin_on_subsample": bool(same)})
            assert n_n == n_c and n_p == n_c + n_f
            panel.free()
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
