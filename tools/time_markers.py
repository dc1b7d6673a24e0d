#!/usr/bin/env python3
"""
Time ``engine.marker_select`` (a greedy minimal set of SNPs that separates every pair of accessions of a resident panel) at the shape
of a 1001-Genomes panel: 1135 accessions x 200k candidate rows (a sorted row list into a panel of 1M rows), depth 1, on an int8 and
on a packed panel.

Panels are the library's synthetic panel (``Panel.fill_synthetic``).  Reported per shape, one JSON line: the rounds the loop needed,
the four kernels (``k_mk_rowplanes`` once per call; ``k_mk_gain``, ``k_mk_pick``, ``k_mk_update`` summed over the call and per round
that did work -- rounds are enqueued eight at a time, the ones behind the end return at once and are counted as launches only; HIP
events, per repetition), the whole call (validation, uploads, the reads of the state between batches and the results included), and
as the yardstick for ONE pass over bit-planes of the same selection ``k_kin_count`` (``engine.kinship_counts``), the calls
alternating in the same run.  Compared with, on the same values: the numpy twin (tests/markers_twin.py) for ``--twin-rounds`` rounds
on the first ``--twin-rows`` selected rows, scaled by rows and by rounds to the whole loop (both factors are stated in the output;
the device's picks on that subsample must equal the twin's).

    python tools/time_markers.py [--reps 3] [--shape int8|packed|all] [--out profiles/time_markers.txt]

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

import markers_twin  # noqa: E402

SEED = 1001


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shape", default="all", choices=["int8", "packed", "all"])
    ap.add_argument("--panel-rows", type=int, default=1000000)
    ap.add_argument("--rows", type=int, default=200000, help="candidate rows: a sorted random subset of the panel's rows, as a row list")
    ap.add_argument("--accessions", type=int, default=1135)
    ap.add_argument("--depth", type=int, default=1)
    ap.add_argument("--twin-rows", type=int, default=20000)
    ap.add_argument("--twin-rounds", type=int, default=3)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from snpmatch_amd import engine, synth
    ctx = None if args.host_only else engine.default_context()
    rng = np.random.default_rng(SEED)
    rows = np.sort(rng.choice(args.panel_rows, size=args.rows, replace=False)).astype(np.int64)
    n_acc, n_rows, k = args.accessions, args.rows, min(args.twin_rows, args.rows)
    ok = True
    for name, packed in (("int8", False), ("packed", True)):
        if args.shape not in ("all", name):
            continue
        values = synth.panel_values(SEED, 0, int(rows[k - 1]) + 1, 0, n_acc)
        h0, h1 = markers_twin.planes(values, rows=rows[:k])
        t0 = time.perf_counter()
        markers_twin.gains(h0, h1, ~np.eye(n_acc, dtype=bool))                       # what first_gain costs the twin: one more round
        first_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        want = markers_twin.marker_select(values, args.depth, args.twin_rounds, rows=rows[:k], first_gain=False)
        twin_s = time.perf_counter() - t0
        line = {"shape": name, "accessions": n_acc, "rows": n_rows, "depth": args.depth, "panel_rows": args.panel_rows, "packed": packed,
                "numpy_twin_rows": k, "numpy_twin_rounds": args.twin_rounds, "numpy_twin_s": round(twin_s, 2), "numpy_twin_first_gain_s": round(first_s, 2)}
        if ctx is None:
            line["device"] = "not measured"
        else:
            panel = engine.Panel(ctx, args.panel_rows, n_acc, packed=packed)
            panel.fill_synthetic(SEED)
            got = engine.marker_select(panel, args.depth, args.twin_rounds, rows=rows[:k], first_gain=False)      # warm-up; and the check
            same = markers_twin.same(got, want, ("chosen", "gain_at", "remaining", "stop_reason", "need"))
            ok &= same
            engine.marker_select(panel, args.depth, rows=rows)
            engine.kinship_counts(panel, rows=rows)
            ctx.profile(True)
            calls, kin_calls, ms, kin_ms, kin_planes_ms, launches = [], [], {n: [] for n in ("mk_planes", "mk_gain", "mk_pick", "mk_update")}, [], [], None
            for _ in range(args.reps):                                               # the two scans alternate
                ctx.profile_reset()
                t0 = time.perf_counter()
                full = engine.marker_select(panel, args.depth, rows=rows)
                calls.append(time.perf_counter() - t0)
                read = {n: ctx.profile_read(n) for n in ms}
                for n in ms:
                    ms[n].append(read[n][1])
                launches = {n: read[n][0] for n in ms}
                ctx.profile_reset()
                t0 = time.perf_counter()
                engine.kinship_counts(panel, rows=rows)
                kin_calls.append(time.perf_counter() - t0)
                kin_ms.append(ctx.profile_read("kin_count")[1])
                kin_planes_ms.append(ctx.profile_read("kin_planes")[1])
            ctx.profile(False)
            med = lambda v: float(np.median(v))      # noqa: E731
            rounds = full["n_chosen"] + (full["stop_reason"] == 2)                   # a round that finds no gain picks nothing
            scale_rows, scale_rounds = n_rows / k, rounds / max(1, want["n_chosen"])
            line.update({"reps": args.reps, "rounds": int(rounds), "markers": full["n_chosen"], "remaining": full["remaining"], "stop_reason": full["stop_reason"],
                         "unresolved_pairs": int(np.count_nonzero(np.triu(full["need"], 1))), "launches": launches,
                         "planes_ms": round(med(ms["mk_planes"]), 3),
                         "gain_ms_total": round(med(ms["mk_gain"]), 3), "pick_ms_total": round(med(ms["mk_pick"]), 3), "update_ms_total": round(med(ms["mk_update"]), 3),
                         "gain_ms_per_round": round(med(ms["mk_gain"]) / rounds, 4), "pick_ms_per_round": round(med(ms["mk_pick"]) / rounds, 4),
                         "update_ms_per_round": round(med(ms["mk_update"]) / rounds, 4), "gain_ms_total_all": [round(v, 3) for v in ms["mk_gain"]],
                         "call_ms_median": round(med(calls) * 1e3, 2), "call_ms_min": round(min(calls) * 1e3, 2),
                         "kin_count_ms": round(med(kin_ms), 3), "kin_planes_ms": round(med(kin_planes_ms), 3), "kin_count_ms_all": [round(v, 3) for v in kin_ms],
                         "kin_call_ms_median": round(med(kin_calls) * 1e3, 2),
                         "gain_round_over_kin_count": round(med(ms["mk_gain"]) / rounds / med(kin_ms), 4) if med(kin_ms) else None,
                         "numpy_twin_scale_rows": round(scale_rows, 2), "numpy_twin_scale_rounds": round(scale_rounds, 2),
                         "numpy_twin_scaled_to_whole_loop_s": round(twin_s * scale_rows * scale_rounds + first_s * scale_rows, 1),
                         "first_picks": full["chosen"][:5].tolist(), "first_gains": full["gain_at"][:5].tolist(),
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
