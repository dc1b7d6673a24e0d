#!/usr/bin/env python3
"""
Time ``engine.cross_calls`` (genotype_cross: counts and decision of every window x sample in one device call) at the shape of
an F2 population on TAIR10: 384 samples x ~100k matched segregating markers x 399 windows of 300 kb.

Reported: the kernel (``k_gcross``, HIP events) and the whole call (host arrays in, host arrays out: copies included), each with
the bytes it moves, and the numpy twin (tests/gcross_twin.py) on the same inputs on the same machine, whose calls and counts the
device's must equal.  One JSON line.

    python tools/time_gcross.py [--samples 384] [--markers 100000] [--reps 20]
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

import gcross_twin  # noqa: E402
from snpmatch_amd import engine  # noqa: E402
from snpmatch_amd.core import genomes  # noqa: E402


def make_inputs(n_samples, n_markers, bin_len, seed=7):
    """markers spread over TAIR10 in proportion to chromosome length; F2-like blocks per (window, sample) with 3 % errors, 10 % no-calls"""
    rng = np.random.default_rng(seed)
    genome = genomes.Genome("athaliana_tair10")
    table = genome.window_table(bin_len)
    span = np.array([min(e, int(genome.chrlen[c])) - s + 1 for c, s, e in table], dtype=np.float64)
    sizes = rng.multinomial(n_markers, span / span.sum())
    win_off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    n = int(win_off[-1])
    p1 = rng.integers(0, 2, size=n).astype(np.int8)
    p2 = (1 - p1).astype(np.int8)
    window = np.repeat(np.arange(len(table)), sizes)
    state = rng.choice(3, size=(len(table), n_samples), p=[0.25, 0.5, 0.25])[window]
    value = np.where(state == 0, p1[:, None], np.where(state == 1, 2, p2[:, None]))
    noise = rng.random((n, n_samples), dtype=np.float32)
    cls = np.where(noise < 0.03, rng.integers(0, 3, size=(n, n_samples)), value)
    cls = np.where(noise > 0.90, 3, cls)
    return cls.astype(np.uint8), p1, p2, win_off


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--samples", type=int, default=384)
    ap.add_argument("--markers", type=int, default=100000)
    ap.add_argument("--bin", type=int, default=300000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lr_thres", type=float, default=1.5)
    args = ap.parse_args()
    codes, p1, p2, win_off = make_inputs(args.samples, args.markers, args.bin)
    n, ns, n_win = codes.shape[0], codes.shape[1], len(win_off) - 1

    t0 = time.perf_counter()
    want_geno, want_counts, lr_next = gcross_twin.cross_calls(codes, p1, p2, win_off, args.lr_thres)
    twin_s = time.perf_counter() - t0
    edge = gcross_twin.knife_edge_cells(lr_next, args.lr_thres)

    ctx = engine.default_context()
    geno, counts = engine.cross_calls(ctx, codes, p1, p2, win_off, args.lr_thres, return_counts=True)      # warm-up: workspaces
    same_counts = bool(np.array_equal(counts, want_counts))
    differing = int(np.count_nonzero(geno != want_geno))
    ctx.profile(True)
    ctx.profile_reset()
    calls = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        engine.cross_calls(ctx, codes, p1, p2, win_off, args.lr_thres)
        calls.append(time.perf_counter() - t0)
    launches, kernel_ms = ctx.profile_read("gcross")
    ctx.profile(False)
    kernel_s = kernel_ms / 1e3 / max(launches, 1)
    pitch = (ns + 255) // 256 * 256
    kernel_bytes = n * pitch + 2 * n + 8 * (n_win + 1) + n_win * ns          # rows as the kernel strides them, parents, bounds, calls
    call_bytes = n * ns + 2 * n + 8 * (n_win + 1) + n_win * ns               # what crosses the host-device link per call
    call_s = float(np.median(calls))
    print(json.dumps({
        "samples": ns, "markers": n, "windows": n_win, "reps": args.reps,
        "kernel_ms": round(kernel_s * 1e3, 4), "kernel_bytes": kernel_bytes, "kernel_GBps": round(kernel_bytes / kernel_s / 1e9, 1) if kernel_s else None,
        "call_ms_median": round(call_s * 1e3, 3), "call_ms_min": round(min(calls) * 1e3, 3), "call_bytes": call_bytes,
        "call_GBps": round(call_bytes / call_s / 1e9, 2),
        "numpy_twin_ms": round(twin_s * 1e3, 1), "counts_equal_twin": same_counts, "calls_differing_from_twin": differing,
        "twin_cells_on_the_threshold": edge,
    }))
    return 0 if same_counts and differing <= edge else 1


if __name__ == "__main__":
    sys.exit(main())
