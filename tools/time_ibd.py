#!/usr/bin/env python3
"""
Time ``engine.ibd_counts`` (for every pair of accessions of a resident panel the genome windows in which the two are identical, and
the runs they form) at the shape of a 1001-Genomes panel: 1135 accessions x 200k rows (a sorted row list) in 399 windows whose row
counts are proportional to the 300 kb windows of TAIR10, on an int8 and on a packed panel of 1M rows.

Panels are the library's synthetic panel (``Panel.fill_synthetic``).  Reported per shape, one JSON line: the three kernels
(``k_win_planes``, ``k_ibd_count``, ``k_ibd_runs``; HIP events, per repetition), the whole call (host arrays out -- the two bitsets
are 134 MB --, validation, the plan and copies included), and as the yardstick ``k_par_count`` over the SAME selection and windows,
the calls alternating in the same run (``engine.parent_counts``), with the ratio of the two count kernels and the run-to-run spread
of each.  Compared with, on the same values: the numpy twin (tests/ibd_twin.py) on the windows that hold the first ``--twin-rows``
selected rows, scaled by rows (the subsample is stated in the output; the device's results on those windows must equal the twin's).

    python tools/time_ibd.py [--reps 5] [--shape int8|packed|all] [--out profiles/time_ibd.txt]

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

import ibd_twin  # noqa: E402

TAIR10 = (30427671, 19698289, 23459830, 18585056, 26975502)
BIN = 300000
SEED = 1001


def tair10_windows(n_rows, bin_len=BIN):
    """offsets [n_win + 1] of n_rows rows spread evenly over the base pairs of TAIR10, cut into its windows of bin_len"""
    spans = np.array([min(bin_len, length - 1 - lo) for length in TAIR10 for lo in range(0, length - 1, bin_len)], dtype=np.float64)
    edges = np.concatenate([[0.0], np.cumsum(spans)]) / spans.sum()
    off = np.rint(edges * n_rows).astype(np.int64)
    off[0], off[-1] = 0, n_rows
    return off


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shape", default="all", choices=["int8", "packed", "all"])
    ap.add_argument("--panel-rows", type=int, default=1000000)
    ap.add_argument("--rows", type=int, default=200000, help="selected rows: a sorted random subset of the panel's rows, as a row list")
    ap.add_argument("--accessions", type=int, default=1135)
    ap.add_argument("--min-win-sites", type=int, default=20)
    ap.add_argument("--max-diff-ppm", type=int, default=1000)
    ap.add_argument("--min-run", type=int, default=5)
    ap.add_argument("--twin-rows", type=int, default=10000)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from snpmatch_amd import engine, synth
    ctx = None if args.host_only else engine.default_context()
    rng = np.random.default_rng(SEED)
    rows = np.sort(rng.choice(args.panel_rows, size=args.rows, replace=False)).astype(np.int64)
    classes = rng.choice(np.array([0, 1, 2, 0xFF], dtype=np.uint8), size=args.rows, p=[0.45, 0.35, 0.17, 0.03])      # of the yardstick's sample
    win_off = tair10_windows(args.rows)
    n_acc, n_rows, n_win = args.accessions, args.rows, len(win_off) - 1
    params = (args.min_win_sites, args.max_diff_ppm, args.min_run)
    ok = True
    for name, packed in (("int8", False), ("packed", True)):
        if args.shape not in ("all", name):
            continue
        # the twin on the first whole windows (they lie in the first stretch of the panel: only that stretch is generated)
        w_sub = max(1, int(np.searchsorted(win_off, min(args.twin_rows, n_rows), side="right")) - 1)
        k = int(win_off[w_sub])
        values = synth.panel_values(SEED, 0, int(rows[k - 1]) + 1, 0, n_acc)
        t0 = time.perf_counter()
        want = ibd_twin.ibd_counts(values, win_off[:w_sub + 1], *params, rows=rows[:k])
        twin_s = time.perf_counter() - t0
        line = {"shape": name, "accessions": n_acc, "rows": n_rows, "windows": n_win, "min_win_sites": params[0], "max_diff_ppm": params[1],
                "min_run": params[2], "panel_rows": args.panel_rows, "packed": packed, "numpy_twin_rows": k, "numpy_twin_windows": w_sub,
                "numpy_twin_s": round(twin_s, 2), "numpy_twin_scaled_to_all_rows_s": round(twin_s * n_rows / k, 1)}
        if ctx is None:
            line["device"] = "not measured"
        else:
            panel = engine.Panel(ctx, args.panel_rows, n_acc, packed=packed)
            panel.fill_synthetic(SEED)
            got = engine.ibd_counts(panel, win_off[:w_sub + 1], *params, rows=rows[:k])      # warm-up; and the check
            same = all(np.array_equal(got[key], want[key]) for key in want)
            ok &= same
            engine.ibd_counts(panel, win_off, *params, rows=rows)
            engine.parent_counts(panel, classes, win_off, 5, rows=rows)
            ctx.profile(True)
            ibd_calls, par_calls, ibd_ms, runs_ms, par_ms, planes_ms, launches = [], [], [], [], [], [], []
            for _ in range(args.reps):                                               # the two scans alternate
                ctx.profile_reset()
                t0 = time.perf_counter()
                full = engine.ibd_counts(panel, win_off, *params, rows=rows)
                ibd_calls.append(time.perf_counter() - t0)
                n_c, ms_c = ctx.profile_read("ibd_count")
                n_r, ms_r = ctx.profile_read("ibd_runs")
                n_p, ms_p = ctx.profile_read("win_planes")
                ibd_ms.append(ms_c)
                runs_ms.append(ms_r)
                planes_ms.append(ms_p)
                launches.append((n_p, n_c, n_r))
                ctx.profile_reset()
                t0 = time.perf_counter()
                engine.parent_counts(panel, classes, win_off, 5, rows=rows)
                par_calls.append(time.perf_counter() - t0)
                par_ms.append(ctx.profile_read("par_count")[1])
            ctx.profile(False)
            med = lambda v: float(np.median(v))      # noqa: E731
            spread = lambda v: (max(v) - min(v)) / med(v) if med(v) else None      # noqa: E731
            pair_rows = float(n_acc) * n_acc * n_rows
            off_diag = ~np.eye(n_acc, dtype=bool)
            line.update({"reps": args.reps, "slabs": launches[0][0], "count_launches": launches[0][1], "runs_launches": launches[0][2],
                         "planes_ms": round(med(planes_ms), 3), "count_ms": round(med(ibd_ms), 3), "count_ms_all": [round(v, 3) for v in ibd_ms],
                         "runs_ms": round(med(runs_ms), 3),
                         "count_pair_rows_per_s": round(pair_rows / (med(ibd_ms) / 1e3), 0) if med(ibd_ms) else None,
                         "call_ms_median": round(med(ibd_calls) * 1e3, 2), "call_ms_min": round(min(ibd_calls) * 1e3, 2),
                         "par_count_ms": round(med(par_ms), 3), "par_count_ms_all": [round(v, 3) for v in par_ms],
                         "par_call_ms_median": round(med(par_calls) * 1e3, 2),
                         "count_over_par_count": round(med(ibd_ms) / med(par_ms), 3) if med(par_ms) else None,
                         "count_spread": round(spread(ibd_ms), 4), "par_count_spread": round(spread(par_ms), 4),
                         "call_bytes_to_host": 28 * n_acc * n_acc + 8 * n_acc * n_acc * ((n_win + 31) // 32),
                         "windows_used_off_diagonal": int(full["w_used"][off_diag].sum()), "windows_shared_off_diagonal": int(full["w_shared"][off_diag].sum()),
                         "results_equal_twin_on_subsample": bool(same)})
            panel.free()
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
