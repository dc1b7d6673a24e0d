#!/usr/bin/env python3
"""
Time ``engine.site_counts`` (allele counts of every panel row per group of accessions, one streaming pass over the resident panel)
at five shapes:

  int8-g1 / int8-g8      1135 accessions x 11M rows, one byte per call, 1 and 8 groups
  packed-g1 / packed-g8  the same panel, 2 bits per call (split rows: 256 + 32 bytes)
  wide-g1                10 000 accessions x 2M rows (int8), 1 group

Panels are the library's synthetic panel (``Panel.fill_synthetic``); group 0 is all accessions, the others are random halves.
Reported per shape, one JSON line: the kernel (``k_site_counts``; HIP events, summed over the slabs of a call) with the bytes it
moves (panel rows at their pitch in, 16 bytes per row and group out), the whole call (host array out: validation, slab copies to
pageable host memory included), and the kernel's read rate as a fraction of what the read-only kernel ``k_calib_read``
(``Panel.stream_read``: every panel byte once, nothing else) reaches over the same panel in the same run -- that kernel has no HIP
events of its own, so it is timed by the host clock around the synchronous call, best of ``--reps`` (a launch and a
synchronisation on top of milliseconds of reading).  Compared with the numpy twin (tests/sitestats_twin.py) on the first
``--twin-rows`` rows, SCALED by rows (the subsample is stated in the output; the device's counts of those rows must equal the
twin's).

    python tools/time_sitestats.py [--reps 3] [--shape int8-g1|...|all] [--out profiles/r09_time_sitestats.txt]

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

import sitestats_twin  # noqa: E402

SEED = 1001


def groups_of(n_acc, n_groups):
    if n_groups == 1:
        return None
    rng = np.random.default_rng(n_acc + n_groups)
    return [np.arange(n_acc)] + [np.sort(rng.permutation(n_acc)[:n_acc // 2]) for _ in range(n_groups - 1)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shape", default="all")
    ap.add_argument("--rows", type=int, default=11000000)
    ap.add_argument("--accessions", type=int, default=1135)
    ap.add_argument("--wide-rows", type=int, default=2000000)
    ap.add_argument("--wide-accessions", type=int, default=10000)
    ap.add_argument("--twin-rows", type=int, default=20000)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from snpmatch_amd import engine, synth
    ctx = None if args.host_only else engine.default_context()
    ws_bytes = int(os.environ.get("SNPM_SITE_WS_MB", "256")) << 20
    shapes = [("int8-g1", args.accessions, args.rows, False, 1), ("int8-g8", args.accessions, args.rows, False, 8),
              ("packed-g1", args.accessions, args.rows, True, 1), ("packed-g8", args.accessions, args.rows, True, 8),
              ("wide-g1", args.wide_accessions, args.wide_rows, False, 1)]
    ok = True
    panel, panel_key = None, None
    for name, n_acc, n_rows, packed, n_groups in shapes:
        if args.shape not in ("all", name):
            continue
        groups = groups_of(n_acc, n_groups)
        values = synth.panel_values(SEED, 0, min(n_rows, args.twin_rows), 0, n_acc)
        t0 = time.perf_counter()
        want = sitestats_twin.site_counts(values, groups)
        twin_s = time.perf_counter() - t0
        line = {"shape": name, "accessions": n_acc, "rows": n_rows, "packed": packed, "groups": n_groups, "numpy_twin_rows": len(values),
                "numpy_twin_s": round(twin_s, 3), "numpy_twin_scaled_to_all_rows_s": round(twin_s * n_rows / len(values), 1)}
        if ctx is None:
            line["device"] = "not measured"
        else:
            if panel_key != (n_acc, n_rows, packed):
                if panel is not None:
                    panel.free()
                panel = engine.Panel(ctx, n_rows, n_acc, packed=packed)
                panel.fill_synthetic(SEED)
                panel_key = (n_acc, n_rows, packed)
            same = bool(np.array_equal(engine.site_counts(panel, groups, range(0, len(values))), want))      # warm-up and the check
            ok &= same
            engine.site_counts(panel, groups)
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
                engine.site_counts(panel, groups)
                calls.append(time.perf_counter() - t0)
            launches, ms = ctx.profile_read("site_counts")
            ctx.profile(False)
            k_s = ms / args.reps / 1e3
            panel_bytes = n_rows * panel.pitch
            out_bytes = 16 * n_rows * n_groups
            read_rate = read_bytes / min(read_s)
            line.update({"reps": args.reps, "row_pitch_bytes": int(panel.pitch), "slabs": launches // args.reps, "workspace_budget_bytes": ws_bytes,
                         "kernel_ms": round(k_s * 1e3, 3), "kernel_bytes_read": panel_bytes, "kernel_bytes_written": out_bytes,
                         "kernel_read_GBps": round(panel_bytes / k_s / 1e9, 1), "kernel_total_GBps": round((panel_bytes + out_bytes) / k_s / 1e9, 1),
                         "calib_read_ms_host_clock": round(min(read_s) * 1e3, 3), "calib_read_GBps": round(read_rate / 1e9, 1),
                         "kernel_read_rate_vs_calib_read": round(panel_bytes / k_s / read_rate, 3),
                         "kernel_total_rate_vs_calib_read": round((panel_bytes + out_bytes) / k_s / read_rate, 3),
                         "call_ms_median": round(float(np.median(calls)) * 1e3, 2), "call_ms_min": round(min(calls) * 1e3, 2),
                         "call_bytes_to_host": out_bytes, "counts_equal_twin_on_subsample": same})
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(text + "\n")
    if panel is not None:
        panel.free()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
