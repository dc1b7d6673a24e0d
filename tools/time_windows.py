#!/usr/bin/env python3
"""
Time ``engine.window_counts`` (per genome window the call counts of every accession and the agreement counts of listed pairs, on
the resident panel) at two shapes:

  int8     1135 accessions x 11M rows, one byte per call
  packed   the same panel, 2 bits per call (split rows: 256 + 32 bytes)

with 399 windows of equal length (TAIR10 at 300 kb has 399), all columns plus 100 random pairs.  Panels are the library's synthetic
panel (``Panel.fill_synthetic``).  Reported per shape, one JSON line: the two kernels (``k_win_planes``, ``k_win_count``; HIP
events, summed over the slabs of a call) with the bytes they move (panel rows at their pitch in and 4 bits per call of the padded
columns out; the plane rows of the columns and of the pairs' members in and 16 bytes per cell out), the whole call (host arrays
out: validation, the slab plan, the per-slab copies and host additions included), and the time of the read-only kernel
``k_calib_read`` (``Panel.stream_read``: every panel byte once, nothing else) over the same rows in the same run as the yardstick
-- that kernel has no HIP events of its own, so it is timed by the host clock around the synchronous call, best of ``--reps``.
Compared with the numpy twin (tests/windows_twin.py) on the first ``--twin-rows`` rows, SCALED by rows (the subsample is stated in
the output; the device's counts of those rows must equal the twin's).

    python tools/time_windows.py [--reps 3] [--shape int8|packed|all] [--out profiles/r11_time_windows.txt]

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

import windows_twin  # noqa: E402

SEED = 1001


def equal_windows(n_rows, n_win):
    return (np.arange(n_win + 1, dtype=np.int64) * n_rows) // n_win


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shape", default="all")
    ap.add_argument("--rows", type=int, default=11000000)
    ap.add_argument("--accessions", type=int, default=1135)
    ap.add_argument("--windows", type=int, default=399)
    ap.add_argument("--pairs", type=int, default=100)
    ap.add_argument("--twin-rows", type=int, default=20000)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from snpmatch_amd import engine, synth
    ctx = None if args.host_only else engine.default_context()
    ws_bytes = int(os.environ.get("SNPM_WIN_WS_MB", "256")) << 20
    ok = True
    for name, packed in (("int8", False), ("packed", True)):
        if args.shape not in ("all", name):
            continue
        n_acc, n_rows, n_win = args.accessions, args.rows, args.windows
        pairs = np.random.default_rng(SEED).integers(0, n_acc, size=(args.pairs, 2))
        sub = min(n_rows, args.twin_rows)
        values = synth.panel_values(SEED, 0, sub, 0, n_acc)
        sub_off = equal_windows(sub, min(n_win, 40))
        t0 = time.perf_counter()
        want = windows_twin.window_counts(values, sub_off, None, pairs)
        twin_s = time.perf_counter() - t0
        line = {"shape": name, "accessions": n_acc, "rows": n_rows, "packed": packed, "windows": n_win, "pairs": len(pairs), "numpy_twin_rows": sub,
                "numpy_twin_s": round(twin_s, 3), "numpy_twin_scaled_to_all_rows_s": round(twin_s * n_rows / sub, 1)}
        if ctx is None:
            line["device"] = "not measured"
        else:
            panel = engine.Panel(ctx, n_rows, n_acc, packed=packed)
            panel.fill_synthetic(SEED)
            got = engine.window_counts(panel, sub_off, None, pairs, range(0, sub))      # warm-up and the check
            same = bool(np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]))
            ok &= same
            win_off = equal_windows(n_rows, n_win)
            engine.window_counts(panel, win_off, None, pairs)
            read_s = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                read_bytes = panel.stream_read()
                read_s.append(time.perf_counter() - t0)
            ctx.profile(True)
            ctx.profile_reset()
            calls = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                engine.window_counts(panel, win_off, None, pairs)
                calls.append(time.perf_counter() - t0)
            launches, planes_ms = ctx.profile_read("win_planes")
            _, count_ms = ctx.profile_read("win_count")
            ctx.profile(False)
            p_s, c_s = planes_ms / args.reps / 1e3, count_ms / args.reps / 1e3
            plan = engine.window_slabs(ws_bytes, n_acc, n_acc + len(pairs), win_off, n_rows)
            cols_pad = -(-n_acc // 64) * 64
            plane_words = sum(s[1] * engine.WIN_STEP_ROWS // 64 for s in plan)      # words per plane row, summed over the slabs
            cells = sum(s[3] for s in plan) * (n_acc + len(pairs))
            line.update({"reps": args.reps, "row_pitch_bytes": int(panel.pitch), "slabs": launches // args.reps, "planned_slabs": len(plan), "workspace_budget_bytes": ws_bytes,
                         "planes_kernel_ms": round(p_s * 1e3, 3), "planes_bytes_read": n_rows * int(panel.pitch), "planes_bytes_written": 4 * cols_pad * plane_words * 8,
                         "count_kernel_ms": round(c_s * 1e3, 3), "count_bytes_read": (4 * n_acc + 6 * len(pairs)) * (n_rows // 8), "count_bytes_written": cells * 16,
                         "calib_read_ms_host_clock": round(min(read_s) * 1e3, 3), "calib_read_GBps": round(read_bytes / min(read_s) / 1e9, 1),
                         "kernels_vs_calib_read": round((p_s + c_s) / min(read_s), 2),
                         "call_ms_median": round(float(np.median(calls)) * 1e3, 2), "call_ms_min": round(min(calls) * 1e3, 2),
                         "call_bytes_to_host": cells * 16, "counts_equal_twin_on_subsample": same})
            panel.free()
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
