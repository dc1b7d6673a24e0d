#!/usr/bin/env python3
"""
Time ``engine.mosaic`` (samples painted as mosaics of the accession columns of a resident panel: the copying-model Viterbi with a
uniform switch cost, every accession a state) at the shape of a 1001-Genomes identification: 1135 accessions x 200k matched rows (a
sorted row list) in 5 chains whose row counts are proportional to the chromosomes of TAIR10, for 1 sample and for a plate of 96, on
an int8 and on a packed panel of 1M rows.

Panels are the library's synthetic panel (``Panel.fill_synthetic``); the samples' classes are drawn from a seed, independent of
the panel -- the adverse case for the forward kernel, whose short route per row (one ballot) needs the best column to match the
sample at that row: here it does at about half of the rows, in a sample that copies accessions at nearly all of them.  Reported per shape and sample count, one JSON line: the three kernels
(``k_win_planes``, ``k_mos_fwd``, ``k_mos_back``; HIP events, summed over the slabs and sample groups of a call, per repetition)
and the whole call (host arrays out, validation, class words, the plan and copies included).  Compared with, on the same values:
the numpy twin (tests/mosaic_twin.py) on the first ``--twin-rows`` selected rows as one chain, scaled by rows (the twin is one
Python step per row and vectorised over the columns, so its time is proportional to the rows; the subsample is stated in the
output; the device's results on it must equal the twin's).

    python tools/time_mosaic.py [--reps 3] [--shape int8|packed|all] [--out profiles/time_mosaic.txt]

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

import mosaic_twin  # noqa: E402

TAIR10 = (30427671, 19698289, 23459830, 18585056, 26975502)
SEED = 1001


def tair10_chains(n_rows):
    """offsets [6] of n_rows rows spread evenly over the base pairs of TAIR10's five chromosomes"""
    off = np.rint(np.concatenate([[0.0], np.cumsum(TAIR10)]) / float(sum(TAIR10)) * n_rows).astype(np.int64)
    off[0], off[-1] = 0, n_rows
    return off


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shape", default="all", choices=["int8", "packed", "all"])
    ap.add_argument("--panel-rows", type=int, default=1000000)
    ap.add_argument("--rows", type=int, default=200000, help="matched rows: a sorted random subset of the panel's rows, as a row list")
    ap.add_argument("--accessions", type=int, default=1135)
    ap.add_argument("--samples", default="1,96", help="sample counts, comma-separated")
    ap.add_argument("--switch-cost", type=int, default=40)
    ap.add_argument("--twin-rows", type=int, default=4000)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from snpmatch_amd import engine, synth
    from snpmatch_amd.core import mosaic
    ctx = None if args.host_only else engine.default_context()
    rng = np.random.default_rng(SEED)
    n_acc, n_rows = args.accessions, args.rows
    counts = [int(v) for v in args.samples.split(",")]
    rows = np.sort(rng.choice(args.panel_rows, size=n_rows, replace=False)).astype(np.int64)
    classes = rng.choice(np.array([0, 1, 2, 0xFF], dtype=np.uint8), size=(max(counts), n_rows), p=[0.45, 0.35, 0.17, 0.03])
    chain_off = tair10_chains(n_rows)
    cost = mosaic.cost_table()
    k = min(args.twin_rows, n_rows)
    ok = True
    for name, packed in (("int8", False), ("packed", True)):
        if args.shape not in ("all", name):
            continue
        # the twin on the first rows as one chain (they lie in the first stretch of the panel: only that stretch is generated)
        values = synth.panel_values(SEED, 0, int(rows[k - 1]) + 1, 0, n_acc)
        t0 = time.perf_counter()
        want = mosaic_twin.mosaic(values, classes[:1, :k], [0, k], cost, args.switch_cost, None, rows[:k], packed)
        twin_s = time.perf_counter() - t0
        base = {"shape": name, "accessions": n_acc, "rows": n_rows, "chains": len(chain_off) - 1, "switch_cost": args.switch_cost,
                "panel_rows": args.panel_rows, "packed": packed, "numpy_twin_rows": k, "numpy_twin_s": round(twin_s, 3),
                "numpy_twin_scaled_to_all_rows_s_per_sample": round(twin_s * n_rows / k, 2)}
        panel = None
        if ctx is not None:
            panel = engine.Panel(ctx, args.panel_rows, n_acc, packed=packed)
            panel.fill_synthetic(SEED)
            got = engine.mosaic(panel, classes[:1, :k], [0, k], cost, args.switch_cost, rows=rows[:k], want_col_cost=True)      # warm-up; and the check
            same = all(np.array_equal(g, w) for g, w in zip(got, want))
            ok &= same
            base["results_equal_twin_on_subsample"] = bool(same)
        for n_samples in counts:
            line = dict(base, samples=n_samples)
            if panel is None:
                line["device"] = "not measured"
            else:
                engine.mosaic(panel, classes[:n_samples], chain_off, cost, args.switch_cost, rows=rows)
                ctx.profile(True)
                calls, ms, launches = [], {"win_planes": [], "mos_fwd": [], "mos_back": []}, None
                for _ in range(args.reps):
                    ctx.profile_reset()
                    t0 = time.perf_counter()
                    engine.mosaic(panel, classes[:n_samples], chain_off, cost, args.switch_cost, rows=rows)
                    calls.append(time.perf_counter() - t0)
                    read = {key: ctx.profile_read(key) for key in ms}
                    launches = [read[key][0] for key in ("win_planes", "mos_fwd", "mos_back")]
                    for key in ms:
                        ms[key].append(read[key][1])
                ctx.profile(False)
                med = lambda v: float(np.median(v))      # noqa: E731
                line.update({"reps": args.reps, "slabs": launches[0], "fwd_launches": launches[1], "back_launches": launches[2],
                             "planes_ms": round(med(ms["win_planes"]), 3), "fwd_ms": round(med(ms["mos_fwd"]), 3), "fwd_ms_all": [round(v, 3) for v in ms["mos_fwd"]],
                             "back_ms": round(med(ms["mos_back"]), 3), "call_ms_median": round(med(calls) * 1e3, 2), "call_ms_min": round(min(calls) * 1e3, 2),
                             "fwd_ns_per_row_of_the_longest_chain": round(med(ms["mos_fwd"]) * 1e6 / launches[1] / float(np.diff(chain_off).max()), 1),
                             "twin_over_call": round(twin_s * n_rows / k * n_samples / med(calls), 1)})
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
