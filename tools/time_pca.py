#!/usr/bin/env python3
"""
Time ``engine.gram`` and ``engine.loadings`` (the two device primitives of ``snpmatch pca``) and the whole analysis at the shape of a
1001-Genomes panel: 1135 accessions x 200k selected rows (a sorted row list into a panel of 1M rows), on an int8 and on a packed
panel.

Panels are the library's synthetic panel (``Panel.fill_synthetic``); the table is the one ``standardise`` makes from the device's own
site counts with the command's defaults (rows that fail keep a zero table, so every shape times all 200k rows).  Reported per shape,
one JSON line, all legs alternating in the same run (HIP events per repetition, medians):
  the Gram kernel ``k_pca_gram`` (+ ``k_pca_fold``) beside ``k_kin_count`` over the same selection, with the FMAs it issues (every
    tile pair in full: tile pairs x 64 x 64 x rows; the matrix needs ncols^2 / 2 x rows) and the rate that makes;
  the planes (``k_win_planes``) beside ``k_kin_planes``;
  the loadings kernel ``k_pca_load`` (k = 10) beside the read-only kernel ``snpm_debug_stream_read`` of the whole panel scaled to the
    bytes of the selected rows;
  the whole ``pca.analyse`` (site counts, standardise, Gram, ``numpy.linalg.eigh``, loadings) with its host part stated.
Compared with, on the same values: the numpy twin (tests/pca_twin.py) of both primitives on the first ``--twin-rows`` selected rows,
scaled by rows; the device's results on that subsample must lie within the summation bound of the twin's.

    python tools/time_pca.py [--reps 3] [--shape int8|packed|all] [--out profiles/time_pca.txt]

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

import pca_twin  # noqa: E402
import sitestats_twin  # noqa: E402

SEED = 1001
TILE = 64


class DeviceGenotype(object):
    """the three scans of ``pca.analyse`` on a resident panel"""

    def __init__(self, engine, panel):
        self.engine, self.panel = engine, panel

    def site_counts(self, acc_ix=None, rows=None):
        return self.engine.site_counts(self.panel, acc_ix, rows)

    def gram(self, tab, acc_ix=None, rows=None):
        return self.engine.gram(self.panel, tab, acc_ix, rows)

    def loadings(self, tab, vec, acc_ix=None, rows=None):
        return self.engine.loadings(self.panel, tab, vec, acc_ix, rows)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shape", default="all", choices=["int8", "packed", "all"])
    ap.add_argument("--panel-rows", type=int, default=1000000)
    ap.add_argument("--rows", type=int, default=200000, help="selected rows: a sorted random subset of the panel's rows, as a row list")
    ap.add_argument("--accessions", type=int, default=1135)
    ap.add_argument("--components", type=int, default=10)
    ap.add_argument("--twin-rows", type=int, default=20000)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from snpmatch_amd import engine, synth
    from snpmatch_amd.core import pca
    ctx = None if args.host_only else engine.default_context()
    rng = np.random.default_rng(SEED)
    rows = np.sort(rng.choice(args.panel_rows, size=args.rows, replace=False)).astype(np.int64)
    n_acc, n_rows, k, sub = args.accessions, args.rows, args.components, min(args.twin_rows, args.rows)
    n_tiles = (n_acc + TILE - 1) // TILE
    fma_issued, fma_needed = n_tiles * (n_tiles + 1) // 2 * TILE * TILE * n_rows, n_acc * n_acc // 2 * n_rows
    ok = True
    for name, packed in (("int8", False), ("packed", True)):
        if args.shape not in ("all", name):
            continue
        values = synth.panel_values(SEED, 0, int(rows[sub - 1]) + 1, 0, n_acc)
        tab_sub = pca.standardise(sitestats_twin.site_counts(values, None, rows[:sub])[0], n_acc)[1]
        t0 = time.perf_counter()
        want_gram = pca_twin.gram(values, tab_sub, None, rows[:sub])
        twin_gram_s = time.perf_counter() - t0
        vec = pca.decompose(want_gram, sub, k)[1]
        t0 = time.perf_counter()
        want_load = pca_twin.loadings(values, tab_sub, vec, None, rows[:sub])
        twin_load_s = time.perf_counter() - t0
        line = {"shape": name, "accessions": n_acc, "rows": n_rows, "components": k, "panel_rows": args.panel_rows, "packed": packed,
                "numpy_twin_rows": sub, "numpy_twin_gram_s": round(twin_gram_s, 3), "numpy_twin_loadings_s": round(twin_load_s, 3),
                "numpy_twin_gram_scaled_s": round(twin_gram_s * n_rows / sub, 2), "numpy_twin_loadings_scaled_s": round(twin_load_s * n_rows / sub, 2),
                "gram_fma_issued": fma_issued, "gram_fma_needed": fma_needed}
        if ctx is None:
            line["device"] = "not measured"
        else:
            panel = engine.Panel(ctx, args.panel_rows, n_acc, packed=packed)
            panel.fill_synthetic(SEED)
            got_gram = engine.gram(panel, tab_sub, rows=rows[:sub])                   # warm-up; and the check
            got_load = engine.loadings(panel, tab_sub, vec, rows=rows[:sub])
            same = bool((np.abs(got_gram - want_gram) <= 2.0 * sub * 2.0 ** -53 * pca_twin.gram_abs(values, tab_sub, None, rows[:sub])).all() and
                        (np.abs(got_load - want_load) <= 2.0 * n_acc * 2.0 ** -53 * pca_twin.loadings_abs(values, tab_sub, vec, None, rows[:sub])).all())
            ok &= same
            holder = DeviceGenotype(engine, panel)
            tab = pca.standardise(engine.site_counts(panel, None, rows)[0], n_acc)[1]
            res = pca.analyse(holder, None, n_acc, rows, 0.05, 0.1, k)
            vec_full = res["vec"]
            engine.kinship_counts(panel, rows=rows)
            bytes_all = panel.stream_read()
            names = ("win_planes", "pca_gram", "pca_fold", "pca_load", "kin_planes", "kin_count")
            ms, calls = {n: [] for n in names}, {n: [] for n in ("gram", "loadings", "kinship", "stream_read", "analyse", "eigh")}
            ctx.profile(True)
            for _ in range(args.reps):                                               # the legs alternate
                ctx.profile_reset()
                t0 = time.perf_counter()
                engine.gram(panel, tab, rows=rows)
                calls["gram"].append(time.perf_counter() - t0)
                for n in ("win_planes", "pca_gram", "pca_fold"):
                    ms[n].append(ctx.profile_read(n)[1])
                ctx.profile_reset()
                t0 = time.perf_counter()
                engine.kinship_counts(panel, rows=rows)
                calls["kinship"].append(time.perf_counter() - t0)
                for n in ("kin_planes", "kin_count"):
                    ms[n].append(ctx.profile_read(n)[1])
                ctx.profile_reset()
                t0 = time.perf_counter()
                engine.loadings(panel, tab, vec_full, rows=rows)
                calls["loadings"].append(time.perf_counter() - t0)
                ms["pca_load"].append(ctx.profile_read("pca_load")[1])
                ctx.synchronize()
                t0 = time.perf_counter()
                panel.stream_read()
                ctx.synchronize()
                calls["stream_read"].append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                res = pca.analyse(holder, None, n_acc, rows, 0.05, 0.1, k)
                calls["analyse"].append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                pca.decompose(res["gram"], res["R"], k)
                calls["eigh"].append(time.perf_counter() - t0)
            ctx.profile(False)
            med = lambda v: float(np.median(v))      # noqa: E731
            row_bytes = bytes_all / args.panel_rows
            read_ms = med(calls["stream_read"]) * 1e3 * n_rows / args.panel_rows
            line.update({"reps": args.reps, "rows_used_by_analyse": int(res["R"]),
                         "gram_ms": round(med(ms["pca_gram"]), 3), "fold_ms": round(med(ms["pca_fold"]), 3), "planes_ms": round(med(ms["win_planes"]), 3),
                         "gram_ms_all": [round(v, 3) for v in ms["pca_gram"]],
                         "gram_tfma_per_s_issued": round(fma_issued / med(ms["pca_gram"]) / 1e9, 2), "gram_tfma_per_s_needed": round(fma_needed / med(ms["pca_gram"]) / 1e9, 2),
                         "kin_count_ms": round(med(ms["kin_count"]), 3), "kin_planes_ms": round(med(ms["kin_planes"]), 3),
                         "gram_over_kin_count": round(med(ms["pca_gram"]) / med(ms["kin_count"]), 2) if med(ms["kin_count"]) else None,
                         "load_ms": round(med(ms["pca_load"]), 3), "load_ms_all": [round(v, 3) for v in ms["pca_load"]],
                         "stream_read_whole_panel_ms": round(med(calls["stream_read"]) * 1e3, 3), "panel_row_bytes": row_bytes,
                         "stream_read_scaled_to_selected_rows_ms": round(read_ms, 3), "load_over_read": round(med(ms["pca_load"]) / read_ms, 2) if read_ms else None,
                         "gram_call_ms": round(med(calls["gram"]) * 1e3, 2), "loadings_call_ms": round(med(calls["loadings"]) * 1e3, 2),
                         "kinship_call_ms": round(med(calls["kinship"]) * 1e3, 2), "analyse_ms": round(med(calls["analyse"]) * 1e3, 1),
                         "eigh_ms": round(med(calls["eigh"]) * 1e3, 1), "eigenvalues": [round(float(x), 4) for x in res["eigenvalues"][:3]],
                         "results_within_bound_of_twin_on_subsample": same})
            panel.free()
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
