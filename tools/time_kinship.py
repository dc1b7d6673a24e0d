#!/usr/bin/env python3
"""
Time ``engine.kinship_counts`` (relatedness counts of every pair of accessions of a resident panel) at three shapes:

  int8     1135 accessions x 1M rows, one byte per call
  packed   the same panel, 2 bits per call
  slabs    10 000 accessions x 200k rows (packed): the bit-planes of all rows exceed the default workspace budget, so the row axis
           is processed in several slabs

Panels are the library's synthetic panel (``Panel.fill_synthetic``).  Reported per shape, one JSON line: the two kernels
(``k_kin_planes``, ``k_kin_count``; HIP events) with the bytes each moves, the whole call (host arrays out, validation and copies
included) and its bytes.  Compared with, on the same values: the numpy twin (tests/kinship_twin.py) on the first ``--twin-rows``
rows, scaled by rows (the subsample is stated in the output; the device's counts of those rows must equal the twin's), and the
reference's own chunk loop (``calc_kinship_mat`` per 1000 rows, summed) on the first ``--ref-rows`` rows, run by a second
interpreter (``--ref-python``, one whose scipy still has ``scipy.mat``) where a reference checkout (``--reference``) exists.

    python tools/time_kinship.py [--reps 3] [--shape int8|packed|slabs|all]

``--host-only``: only the two comparisons, on a machine without a GPU.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import kinship_twin  # noqa: E402

TILE, PL_COLS, STEP_ROWS, CHUNK_ROWS = 32, 64, 1024, 8192         # KN_TILE, KN_PL_COLS, KN_STEP_WORDS * 64, KN_CHUNK_WORDS * 64
SEED = 1001
REF_LOOP = """
import sys, time, types, warnings
warnings.filterwarnings("ignore")
for m in ("allel", "h5py", "hmmlearn", "hmmlearn.hmm"):
    sys.modules[m] = types.ModuleType(m)
sys.path.insert(0, sys.argv[1])
import numpy as np
from snpmatch.core import snp_genotype as ref
snps = np.load(sys.argv[2])
t0 = time.perf_counter()
k_mat = n_mat = 0
for r in range(0, len(snps), ref.chunk_size):
    k, n = ref.calc_kinship_mat(snps[r:r + ref.chunk_size], return_counts=True)
    k_mat, n_mat = k_mat + k, n_mat + n
print(time.perf_counter() - t0)
"""


def host_comparisons(values, n_rows, args, tmp):
    """numpy twin and reference loop on the first rows of the panel, each scaled to n_rows"""
    out = {}
    sub = values[:max(1024, min(args.twin_rows, int(2.5e10 / values.shape[1] ** 2)))]       # (five n_acc x n_acc x rows products on the host)
    t0 = time.perf_counter()
    want = kinship_twin.kinship_counts(sub)
    twin_s = time.perf_counter() - t0
    out.update(numpy_twin_rows=len(sub), numpy_twin_s=round(twin_s, 2), numpy_twin_scaled_to_all_rows_s=round(twin_s * n_rows / len(sub), 1))
    if os.path.isdir(args.reference) and os.path.exists(args.ref_python):
        path = os.path.join(tmp, "ref_rows.npy")
        np.save(path, values[:args.ref_rows])
        r = subprocess.run([args.ref_python, "-c", REF_LOOP, args.reference, path], capture_output=True, text=True)
        if r.returncode == 0:
            ref_s = float(r.stdout.strip().split()[-1])
            out.update(reference_loop_rows=int(min(args.ref_rows, len(values))), reference_loop_s=round(ref_s, 2),
                       reference_loop_scaled_to_all_rows_s=round(ref_s * n_rows / min(args.ref_rows, len(values)), 1))
        else:
            out["reference_loop"] = "failed: " + r.stderr.strip().split("\n")[-1][:200]
        os.remove(path)
    else:
        out["reference_loop"] = "not measured (no reference checkout / second interpreter on this machine)"
    return want, out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shape", default="all", choices=["int8", "packed", "slabs", "all"])
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--accessions", type=int, default=1135)
    ap.add_argument("--slab-rows", type=int, default=200000)
    ap.add_argument("--slab-accessions", type=int, default=10000)
    ap.add_argument("--twin-rows", type=int, default=20000)
    ap.add_argument("--ref-rows", type=int, default=5000)
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--ref-python", default="/opt/conda/bin/python3.9")
    ap.add_argument("--host-only", action="store_true")
    args = ap.parse_args()
    import tempfile
    from snpmatch_amd import engine, synth
    ctx = None if args.host_only else engine.default_context()
    ws_bytes = int(os.environ.get("SNPM_KIN_WS_MB", "512")) << 20
    ok = True
    shapes = [("int8", args.accessions, args.rows, False), ("packed", args.accessions, args.rows, True),
              ("slabs", args.slab_accessions, args.slab_rows, True)]
    with tempfile.TemporaryDirectory() as tmp:
        for name, n_acc, n_rows, packed in shapes:
            if args.shape not in ("all", name):
                continue
            values = synth.panel_values(SEED, 0, min(n_rows, max(args.twin_rows, args.ref_rows)), 0, n_acc)
            want, line = host_comparisons(values, n_rows, args, tmp)
            values = values[:line["numpy_twin_rows"]]
            line = dict({"shape": name, "accessions": n_acc, "rows": n_rows, "packed": packed}, **line)
            if ctx is None:
                line["device"] = "not measured"
                print(json.dumps(line), flush=True)
                continue
            panel = engine.Panel(ctx, n_rows, n_acc, packed=packed)
            panel.fill_synthetic(SEED)
            got = engine.kinship_counts(panel, rows=range(0, len(values)))           # warm-up: workspaces, code object; and the check
            same = all(np.array_equal(g, w) for g, w in zip(got, want))
            ok &= same
            engine.kinship_counts(panel)
            ctx.profile(True)
            ctx.profile_reset()
            calls = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                engine.kinship_counts(panel)
                calls.append(time.perf_counter() - t0)
            n_p, ms_p = ctx.profile_read("kin_planes")
            n_c, ms_c = ctx.profile_read("kin_count")
            ctx.profile(False)
            p_s, c_s = ms_p / args.reps / 1e3, ms_c / args.reps / 1e3
            cols_pad = -(-n_acc // PL_COLS) * PL_COLS
            tiles = -(-n_acc // TILE)
            tile_pairs = tiles * (tiles + 1) // 2
            rows_pad = -(-n_rows // STEP_ROWS) * STEP_ROWS
            plane_bytes = 3 * cols_pad * rows_pad // 8
            panel_bytes = n_rows * (-(-n_acc // 4) if packed else n_acc)                 # the calls the plane kernel reads
            count_bytes = 3 * TILE * (rows_pad // 8) * (2 * tile_pairs - tiles)          # planes as the blocks request them, mostly from cache
            pair_rows = float(n_acc) * n_acc * n_rows
            line.update({"reps": args.reps, "slabs": n_p // args.reps, "workspace_budget_bytes": ws_bytes,
                         "planes_ms": round(p_s * 1e3, 3), "planes_bytes": panel_bytes + plane_bytes,
                         "planes_GBps": round((panel_bytes + plane_bytes) / p_s / 1e9, 1) if p_s else None,
                         "count_ms": round(c_s * 1e3, 3), "count_bytes_requested": count_bytes,
                         "count_GBps_requested": round(count_bytes / c_s / 1e9, 1) if c_s else None,
                         "pair_rows": pair_rows, "count_pair_rows_per_s": round(pair_rows / c_s, 0) if c_s else None,
                         "call_ms_median": round(float(np.median(calls)) * 1e3, 2), "call_ms_min": round(min(calls) * 1e3, 2),
                         "call_bytes_to_host": 12 * n_acc * n_acc, "counts_equal_twin_on_subsample": bool(same)})
            print(json.dumps(line), flush=True)
            panel.free()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
