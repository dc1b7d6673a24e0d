#!/usr/bin/env python3
"""
Time ``engine.parent_counts`` (every pair of accessions of a resident panel scored per genome window as the parents of a recombinant
sample) at the shape of a 1001-Genomes identification: 1135 accessions x 200k matched rows (a sorted row list) in 399 windows whose
row counts are proportional to the 300 kb windows of TAIR10, on an int8 and on a packed panel of 1M rows.

Panels are the library's synthetic panel (``Panel.fill_synthetic``); the sample's classes are drawn from a seed.  Reported per
shape, one JSON line: the two kernels (``k_win_planes``, ``k_par_count``; HIP events, per repetition), the whole call (host arrays
out, validation, the plan and copies included), and as the yardstick ``k_f1x_count`` over the SAME selection, the calls alternating
in the same run (``engine.f1_counts``), with the ratio of the two count kernels and the run-to-run spread of each.  Compared with,
on the same values: the numpy twin (tests/parentsearch_twin.py) on the windows that hold the first ``--twin-rows`` selected rows,
scaled by rows (the subsample is stated in the output; the device's counts of those windows must equal the twin's).

    python tools/time_parentsearch.py [--reps 5] [--shape int8|packed|all] [--out profiles/time_parentsearch.txt]

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

import parentsearch_twin  # noqa: E402

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
    ap.add_argument("--rows", type=int, default=200000, help="matched rows: a sorted random subset of the panel's rows, as a row list")
    ap.add_argument("--accessions", type=int, default=1135)
    ap.add_argument("--min-win-sites", type=int, default=5)
    ap.add_argument("--twin-rows", type=int, default=10000)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from snpmatch_amd import engine, synth
    ctx = None if args.host_only else engine.default_context()
    rng = np.random.default_rng(SEED)
    rows = np.sort(rng.choice(args.panel_rows, size=args.rows, replace=False)).astype(np.int64)
    classes = rng.choice(np.array([0, 1, 2, 0xFF], dtype=np.uint8), size=args.rows, p=[0.45, 0.35, 0.17, 0.03])
    win_off = tair10_windows(args.rows)
    n_acc, n_rows, n_win = args.accessions, args.rows, len(win_off) - 1
    ok = True
    for name, packed in (("int8", False), ("packed", True)):
        if args.shape not in ("all", name):
            continue
        # the twin on the first whole windows (they lie in the first stretch of the panel: only that stretch is generated)
        w_sub = max(1, int(np.searchsorted(win_off, min(args.twin_rows, n_rows), side="right")) - 1)
        k = int(win_off[w_sub])
        values = synth.panel_values(SEED, 0, int(rows[k - 1]) + 1, 0, n_acc)
        t0 = time.perf_counter()
        want = parentsearch_twin.parent_counts(values, classes[:k], win_off[:w_sub + 1], args.min_win_sites, None, rows[:k])
        twin_s = time.perf_counter() - t0
        line = {"shape": name, "accessions": n_acc, "rows": n_rows, "windows": n_win, "min_win_sites": args.min_win_sites,
                "panel_rows": args.panel_rows, "packed": packed, "numpy_twin_rows": k, "numpy_twin_windows": w_sub,
                "numpy_twin_s": round(twin_s, 2), "numpy_twin_scaled_to_all_rows_s": round(twin_s * n_rows / k, 1)}
        if ctx is None:
            line["device"] = "not measured"
        else:
            panel = engine.Panel(ctx, args.panel_rows, n_acc, packed=packed)
            panel.fill_synthetic(SEED)
            got = engine.parent_counts(panel, classes[:k], win_off[:w_sub + 1], args.min_win_sites, rows=rows[:k])      # warm-up; and the check
            same = all(np.array_equal(g, w) for g, w in zip(got, want))
            ok &= same
            engine.parent_counts(panel, classes, win_off, args.min_win_sites, rows=rows)
            engine.f1_counts(panel, classes, rows=rows)
            ctx.profile(True)
            par_calls, f1_calls, par_ms, f1_ms, planes_ms, launches = [], [], [], [], [], []
            for _ in range(args.reps):                                               # the two scans alternate
                ctx.profile_reset()
                t0 = time.perf_counter()
                engine.parent_counts(panel, classes, win_off, args.min_win_sites, rows=rows)
                par_calls.append(time.perf_counter() - t0)
                n_c, ms_c = ctx.profile_read("par_count")
                n_p, ms_p = ctx.profile_read("win_planes")
                par_ms.append(ms_c)
                planes_ms.append(ms_p)
                launches.append((n_p, n_c))
                ctx.profile_reset()
                t0 = time.perf_counter()
                engine.f1_counts(panel, classes, rows=rows)
                f1_calls.append(time.perf_counter() - t0)
                f1_ms.append(ctx.profile_read("f1x_count")[1])
            ctx.profile(False)
            med = lambda v: float(np.median(v))      # noqa: E731
            spread = lambda v: (max(v) - min(v)) / med(v) if med(v) else None      # noqa: E731
            pair_rows = float(n_acc) * n_acc * n_rows
            line.update({"reps": args.reps, "slabs": launches[0][0], "count_launches": launches[0][1], "planes_ms": round(med(planes_ms), 3),
                         "count_ms": round(med(par_ms), 3), "count_ms_all": [round(v, 3) for v in par_ms],
                         "count_pair_rows_per_s": round(pair_rows / (med(par_ms) / 1e3), 0) if med(par_ms) else None,
                         "call_ms_median": round(med(par_calls) * 1e3, 2), "call_ms_min": round(min(par_calls) * 1e3, 2),
                         "f1x_count_ms": round(med(f1_ms), 3), "f1x_count_ms_all": [round(v, 3) for v in f1_ms],
                         "f1x_call_ms_median": round(med(f1_calls) * 1e3, 2),
                         "count_over_f1x_count": round(med(par_ms) / med(f1_ms), 3) if med(f1_ms) else None,
                         "count_spread": round(spread(par_ms), 4), "f1x_count_spread": round(spread(f1_ms), 4),
                         "call_bytes_to_host": 16 * n_acc * n_acc, "counts_equal_twin_on_subsample": bool(same)})
            panel.free()
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
