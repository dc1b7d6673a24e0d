#!/usr/bin/env python3
"""
Time ``engine.ld_band`` (r2 of every panel row with each of the ``band`` rows after it, on the resident panel) at three shapes:

  int8     1135 accessions x 11M rows, one byte per call, band 50
  packed   the same panel, 2 bits per call (split rows: 256 + 32 bytes), band 50
  wide     10 000 accessions x 2M rows (int8), band 50

Panels are the library's synthetic panel (``Panel.fill_synthetic``).  Only r2 is asked for (``counts=False``): the host array is
8 bytes per cell, 4.4 GB at 11M rows and band 50 (the counts would be 36 more per cell).  Reported per shape, one JSON line: the
two kernels (``k_ld_planes``, ``k_ld_band``; HIP events, summed over the slabs of a call) with the bytes they move (panel rows at
their pitch in and 12 bytes per 32 columns and plane row out, halo rows included; those planes in, tile by tile with their halo, and
8 bytes per cell out), the whole call (host array out: validation, slab copies to pageable host memory included), the pairs per
second, and the time of the read-only kernel ``k_calib_read`` (``Panel.stream_read``: every panel byte once, nothing else) over the
same rows in the same run as the yardstick -- that kernel has no HIP events of its own, so it is timed by the host clock around the
synchronous call, best of ``--reps``.  Compared with the numpy twin (tests/ld_twin.py) on the first ``--twin-rows`` rows, SCALED by
rows (the subsample is stated in the output; the device's r2 of those rows must equal the twin's as fp64 bits).

    python tools/time_ld.py [--reps 3] [--shape int8|packed|wide|all] [--band 50] [--out profiles/r10_time_ld.txt]

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

import ld_twin  # noqa: E402

SEED = 1001


def same_bits(a, b):
    nan = np.isnan(b)
    return bool(np.array_equal(np.isnan(a), nan) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shape", default="all")
    ap.add_argument("--band", type=int, default=50)
    ap.add_argument("--rows", type=int, default=11000000)
    ap.add_argument("--accessions", type=int, default=1135)
    ap.add_argument("--wide-rows", type=int, default=2000000)
    ap.add_argument("--wide-accessions", type=int, default=10000)
    ap.add_argument("--twin-rows", type=int, default=2000)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from snpmatch_amd import engine, synth
    ctx = None if args.host_only else engine.default_context()
    ws_bytes = int(os.environ.get("SNPM_LD_WS_MB", "256")) << 20
    shapes = [("int8", args.accessions, args.rows, False), ("packed", args.accessions, args.rows, True), ("wide", args.wide_accessions, args.wide_rows, False)]
    ok = True
    for name, n_acc, n_rows, packed in shapes:
        if args.shape not in ("all", name):
            continue
        band = args.band
        values = synth.panel_values(SEED, 0, min(n_rows, args.twin_rows), 0, n_acc)
        t0 = time.perf_counter()
        want = ld_twin.ld_band(values, band)[1]
        twin_s = time.perf_counter() - t0
        line = {"shape": name, "accessions": n_acc, "rows": n_rows, "packed": packed, "band": band, "numpy_twin_rows": len(values),
                "numpy_twin_s": round(twin_s, 3), "numpy_twin_scaled_to_all_rows_s": round(twin_s * n_rows / len(values), 1)}
        if ctx is None:
            line["device"] = "not measured"
        else:
            panel = engine.Panel(ctx, n_rows, n_acc, packed=packed)
            panel.fill_synthetic(SEED)
            same = same_bits(engine.ld_band(panel, band, None, range(0, len(values)), counts=False)[1], want)      # warm-up and the check
            ok &= same
            engine.ld_band(panel, band, counts=False)
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
                engine.ld_band(panel, band, counts=False)
                calls.append(time.perf_counter() - t0)
            launches, planes_ms = ctx.profile_read("ld_planes")
            _, band_ms = ctx.profile_read("ld_band")
            ctx.profile(False)
            p_s, b_s = planes_ms / args.reps / 1e3, band_ms / args.reps / 1e3
            slabs = launches // args.reps
            words = (n_acc + 31) // 32
            slab_rows = engine.ld_slab_rows(ws_bytes, n_acc, band, n_rows)
            plane_rows = n_rows + (slabs - 1) * band                 # every slab but the last builds its halo again
            tiles = -(-n_rows // 64) * -(-band // 64)
            line.update({"reps": args.reps, "row_pitch_bytes": int(panel.pitch), "slabs": slabs, "slab_rows": slab_rows, "workspace_budget_bytes": ws_bytes,
                         "planes_kernel_ms": round(p_s * 1e3, 3), "planes_bytes_read": plane_rows * int(panel.pitch), "planes_bytes_written": plane_rows * words * 12,
                         "band_kernel_ms": round(b_s * 1e3, 3), "band_bytes_read": tiles * (64 + 127) * words * 12, "band_bytes_written": n_rows * band * 8,
                         "pairs": n_rows * band, "band_kernel_pairs_per_s": round(n_rows * band / b_s, 0),
                         "calib_read_ms_host_clock": round(min(read_s) * 1e3, 3), "calib_read_GBps": round(read_bytes / min(read_s) / 1e9, 1),
                         "kernels_vs_calib_read": round((p_s + b_s) / min(read_s), 2),
                         "call_ms_median": round(float(np.median(calls)) * 1e3, 2), "call_ms_min": round(min(calls) * 1e3, 2),
                         "call_bytes_to_host": n_rows * band * 8, "r2_bits_equal_twin_on_subsample": same})
            panel.free()
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
