#!/usr/bin/env python3
"""
Time ``engine.admix`` (the device primitive of ``snpmatch admixture``) at the shape of a 1001-Genomes panel: 1135 accessions x 200k
selected rows (a sorted row list into a panel of 1M rows), on an int8 and on a packed panel, for K = 3 / 8 / 16.

Panels are the library's synthetic panel (``Panel.fill_synthetic``); Q and F are a random start of the command.  Reported per shape
and K, one JSON line, all legs alternating in the same run (HIP events per repetition, medians):
  ms per iteration of each kernel (``k_adm_rows``, ``k_adm_cols``, ``k_adm_fold``) from a call of one iteration;
  ``k_pca_load`` at k = K over the same selection in the same run: the nearest relative, the same row pass with one FMA per component;
  the fp64 FMA, division and logarithm count per called cell (both kernels form p and pbar: 8 Kp FMAs, Kp = 4 / 8 / 16; a homozygous
    cell takes one division per kernel and one logarithm, a het cell twice that);
  the wall time of a 20-iteration call, parameters resident;
Compared with the numpy twin (tests/admixture_twin.py) per iteration on the first ``--twin-rows`` selected rows, scaled by rows; the
device's iteration on that subsample must agree with the twin's to 1e-9 relative (the bounds proper are what the tests hold).

    python tools/time_admixture.py [--reps 3] [--shape int8|packed|all] [--out profiles/time_admixture.txt]

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

import admixture_twin  # noqa: E402

SEED = 1001
BLOCK = 20


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shape", default="all", choices=["int8", "packed", "all"])
    ap.add_argument("--panel-rows", type=int, default=1000000)
    ap.add_argument("--rows", type=int, default=200000, help="selected rows: a sorted random subset of the panel's rows, as a row list")
    ap.add_argument("--accessions", type=int, default=1135)
    ap.add_argument("--K", type=int, nargs="+", default=[3, 8, 16])
    ap.add_argument("--twin-rows", type=int, default=20000)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from snpmatch_amd import engine, synth
    from snpmatch_amd.core import admixture
    ctx = None if args.host_only else engine.default_context()
    rng = np.random.default_rng(SEED)
    rows = np.sort(rng.choice(args.panel_rows, size=args.rows, replace=False)).astype(np.int64)
    n_acc, n_rows, sub = args.accessions, args.rows, min(args.twin_rows, args.rows)
    values = synth.panel_values(SEED, 0, int(rows[sub - 1]) + 1, 0, n_acc)
    ok = True
    for name, packed in (("int8", False), ("packed", True)):
        if args.shape not in ("all", name):
            continue
        panel = None
        if ctx is not None:
            panel = engine.Panel(ctx, args.panel_rows, n_acc, packed=packed)
            panel.fill_synthetic(SEED)
        for K in args.K:
            Q, F = admixture.random_start(SEED + K, n_acc, n_rows, K)
            t0 = time.perf_counter()
            want = admixture_twin.step(values, Q, F[:sub], None, rows[:sub])
            twin_s = time.perf_counter() - t0
            kp = 4 if K <= 4 else 8 if K <= 8 else 16
            line = {"shape": name, "accessions": n_acc, "rows": n_rows, "K": K, "panel_rows": args.panel_rows, "packed": packed, "numpy_twin_rows": sub,
                    "numpy_twin_iteration_s": round(twin_s, 3), "numpy_twin_iteration_scaled_s": round(twin_s * n_rows / sub, 2),
                    "fma_per_cell": 8 * kp, "div_per_hom_cell": 2, "log_per_hom_cell": 1, "cells": n_acc * n_rows}
            if ctx is None:
                line["device"] = "not measured"
            else:
                got = engine.admix(panel, Q, F[:sub], 1, None, rows[:sub])               # warm-up; and the check
                same = bool(np.allclose(got[0], want[0], rtol=1e-9, atol=0) and np.allclose(got[1], want[1], rtol=1e-9, atol=0) and
                            abs(got[2][0] - want[2]) <= 1e-9 * abs(want[2]))
                ok &= same
                tab = np.ones((n_rows, 4))
                engine.admix(panel, Q, F, 1, None, rows)
                engine.loadings(panel, tab, Q, None, rows)
                names = ("adm_rows", "adm_cols", "adm_fold", "pca_load")
                ms, calls = {n: [] for n in names}, {n: [] for n in ("one", "block", "loadings")}
                ctx.profile(True)
                for _ in range(args.reps):                                               # the legs alternate
                    ctx.profile_reset()
                    t0 = time.perf_counter()
                    engine.admix(panel, Q, F, 1, None, rows)
                    calls["one"].append(time.perf_counter() - t0)
                    for n in names[:3]:
                        ms[n].append(ctx.profile_read(n)[1])
                    ctx.profile_reset()
                    t0 = time.perf_counter()
                    engine.loadings(panel, tab, Q, None, rows)
                    calls["loadings"].append(time.perf_counter() - t0)
                    ms["pca_load"].append(ctx.profile_read("pca_load")[1])
                ctx.profile(False)
                for _ in range(args.reps):                                               # (without the events of the profile)
                    t0 = time.perf_counter()
                    trace = engine.admix(panel, Q, F, BLOCK, None, rows)[2]
                    calls["block"].append(time.perf_counter() - t0)
                med = lambda v: float(np.median(v))      # noqa: E731
                it_ms = med(ms["adm_rows"]) + med(ms["adm_cols"]) + med(ms["adm_fold"])
                line.update({"reps": args.reps, "rows_ms": round(med(ms["adm_rows"]), 3), "cols_ms": round(med(ms["adm_cols"]), 3), "fold_ms": round(med(ms["adm_fold"]), 3),
                             "rows_ms_all": [round(v, 3) for v in ms["adm_rows"]], "cols_ms_all": [round(v, 3) for v in ms["adm_cols"]],
                             "iteration_kernels_ms": round(it_ms, 3), "gfma_per_s": round(8 * kp * n_acc * n_rows / it_ms / 1e6, 1),
                             "pca_load_ms_at_k": round(med(ms["pca_load"]), 3), "rows_over_pca_load": round(med(ms["adm_rows"]) / med(ms["pca_load"]), 2),
                             "one_iteration_call_ms": round(med(calls["one"]) * 1e3, 2), "block_of_20_call_ms": round(med(calls["block"]) * 1e3, 2),
                             "block_of_20_ms_per_iteration": round(med(calls["block"]) * 1e3 / BLOCK, 3), "loglik_rises": bool((np.diff(trace) > 0).all()),
                             "twin_over_device_per_iteration": round(twin_s * n_rows / sub * 1e3 / (med(calls["block"]) * 1e3 / BLOCK), 1),
                             "iteration_close_to_twin_on_subsample": same})
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
