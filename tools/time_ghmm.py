#!/usr/bin/env python3
"""
Time ``engine.cross_hmm`` (genotype_cross_hmm: the Viterbi path of every chromosome x sample in one device call) at the shape
of an F2 population on TAIR10: 384 samples x ~100k matched segregating markers on the five chromosomes (1920 chains).

Reported: the kernel (``k_ghmm``, HIP events) and the whole call (host arrays in, host arrays out: validation and copies
included), each with the bytes it moves, and the numpy twin (tests/ghmm_twin.py) on the same inputs on the same machine, whose
states the device's must equal.  One JSON line.

    python tools/time_ghmm.py [--samples 384] [--markers 100000] [--reps 10]

``--reference-probe PATH``: instead, time ONE probe of the unmodified reference loop (``IdentifyAncestryF2individual(...)
.viterbi(...)`` of the toolkit checked out at PATH, which needs no GPU) on a stated subsample of the same inputs -- the first
``--probe-markers`` markers of chromosome 1 of ``--probe-samples`` samples -- and compare its states with the twin's.
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

import ghmm_twin  # noqa: E402
from snpmatch_amd.core import genomes, infer  # noqa: E402

RATE, BASE_ERROR = 3.5, 0.036
CLASS_TEXT = np.array(["0/0", "1/1", "0/1", "./."])


def make_inputs(n_samples, n_markers, seed=11):
    """markers spread over TAIR10 in proportion to chromosome length; F2-like blocks per (chromosome, sample) with 3 % errors,
    10 % no-calls, DP 0-8 (depth ranks of rint(DP / 2)); homozygous parents"""
    rng = np.random.default_rng(seed)
    genome = genomes.Genome("athaliana_tair10")
    length = genome.chrlen.astype(np.float64)
    sizes = rng.multinomial(n_markers, length / length.sum())
    chain_off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    n = int(chain_off[-1])
    p1 = rng.integers(0, 2, size=n).astype(np.int8)
    p2 = (1 - p1).astype(np.int8)
    cls = np.empty((n, n_samples), dtype=np.uint8)
    for c in range(len(sizes)):
        a, b = int(chain_off[c]), int(chain_off[c + 1])
        cuts = np.sort(rng.integers(0, max(b - a, 1), size=(2, n_samples)), axis=0)
        row = np.arange(b - a)[:, None]
        block = (row >= cuts[0][None, :]).astype(np.int64) + (row >= cuts[1][None, :])
        state = (block + rng.integers(0, 3, size=n_samples)[None, :]) % 3
        cls[a:b] = np.where(state == 0, p1[a:b, None], np.where(state == 1, 2, p2[a:b, None]))
    noise = rng.random((n, n_samples), dtype=np.float32)
    cls = np.where(noise < 0.03, rng.integers(0, 3, size=(n, n_samples)), cls)
    cls = np.where(noise > 0.90, 3, cls).astype(np.uint8)
    halved = rng.integers(0, 9, size=(n, n_samples)) / 2
    levels, rank = np.unique(np.rint(halved), return_inverse=True)
    rank = np.asarray(rank).reshape(halved.shape).astype(np.uint16)
    logT = np.stack([infer.log_transition(infer._transition_frame(genome.chrlen[c] / 1000000, int(sizes[c]), RATE).values)
                     for c in range(len(sizes))])
    _, logI, logE = infer.emission_tables(levels, BASE_ERROR)
    return {"codes": cls, "rank": rank, "halved": halved, "p1": p1, "p2": p2, "pair": infer.pair_index(p1, p2), "chain_off": chain_off,
            "logT": logT, "logI": logI, "logE": logE, "chrlen": genome.chrlen}


def reference_probe(path, inp, n_markers, n_samples):
    """the reference's own loop on the first markers of chromosome 1 (a chain of its own: its transition matrix is the one of
    that many markers); the twin on the same sub-chain must give the same states"""
    import types
    for name in ("allel", "h5py", "hmmlearn", "hmmlearn.hmm"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["hmmlearn"].hmm = sys.modules["hmmlearn.hmm"]
    for name in [m for m in sys.modules if m == "snpmatch" or m.startswith("snpmatch.")]:
        del sys.modules[name]                                        # the toolkit's package name is this repository's alias package
    sys.path.insert(0, path)
    import logging
    logging.disable(logging.CRITICAL)
    from snpmatch.core import infer as ref_infer
    from snpmatch.core import parsers as ref_parsers
    m = min(n_markers, int(inp["chain_off"][1]))
    p1, p2 = inp["p1"][:m], inp["p2"][:m]
    got = np.empty((m, n_samples), dtype=np.int8)
    t0 = time.perf_counter()
    for s in range(n_samples):
        model = ref_infer.IdentifyAncestryF2individual(chromosome_size=inp["chrlen"][0] / 1000000, snps_p1=p1, snps_p2=p2, recomb_rate=RATE,
                                                       base_error=BASE_ERROR, sample_depth=inp["halved"][:m, s])
        got[:, s] = np.array(model.viterbi(ref_parsers.parseGT(CLASS_TEXT[inp["codes"][:m, s]]))[0], dtype=int)
    took = time.perf_counter() - t0
    logT = infer.log_transition(infer._transition_frame(inp["chrlen"][0] / 1000000, m, RATE).values)[None]
    want, _ = ghmm_twin.cross_hmm(inp["codes"][:m, :n_samples], inp["rank"][:m, :n_samples], inp["pair"][:m], [0, m], logT, inp["logI"], inp["logE"])
    print(json.dumps({"reference_probe_markers": m, "reference_probe_samples": n_samples, "reference_probe_s": round(took, 2),
                      "us_per_marker_step": round(took / (m * n_samples) * 1e6, 1), "states_equal_twin": bool(np.array_equal(got, want))}))
    return 0 if np.array_equal(got, want) else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--samples", type=int, default=384)
    ap.add_argument("--markers", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--reference-probe", default=None)
    ap.add_argument("--probe-markers", type=int, default=2000)
    ap.add_argument("--probe-samples", type=int, default=4)
    args = ap.parse_args()
    inp = make_inputs(args.samples, args.markers)
    if args.reference_probe:
        return reference_probe(args.reference_probe, inp, args.probe_markers, args.probe_samples)
    step = (inp["codes"], inp["rank"], inp["pair"], inp["chain_off"], inp["logT"], inp["logI"], inp["logE"])
    n, ns = inp["codes"].shape
    n_chain = len(inp["chain_off"]) - 1

    t0 = time.perf_counter()
    want, _ = ghmm_twin.cross_hmm(*step)
    twin_s = time.perf_counter() - t0

    from snpmatch_amd import engine
    ctx = engine.default_context()
    state = engine.cross_hmm(ctx, *step)                              # warm-up: workspaces
    differing = int(np.count_nonzero(state != want))
    ctx.profile(True)
    ctx.profile_reset()
    calls = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        engine.cross_hmm(ctx, *step)
        calls.append(time.perf_counter() - t0)
    launches, kernel_ms = ctx.profile_read("ghmm")
    ctx.profile(False)
    kernel_s = kernel_ms / 1e3 / max(launches, 1)
    pitch = (ns + 63) // 64 * 64
    tables = 8 * (9 * n_chain + 2 * inp["logI"].size)
    # the kernel reads codes (1 B), depth ranks (2 B) and its own backpointers (1 B) and writes backpointers and states (1 B each)
    kernel_bytes = n * pitch * 6 + n + 8 * (n_chain + 1) + tables
    call_bytes = n * ns * 4 + n + 8 * (n_chain + 1) + tables                 # codes + ranks in, states out
    call_s = float(np.median(calls))
    print(json.dumps({
        "samples": ns, "markers": n, "chains": n_chain * ns, "depth_levels": int(inp["logI"].shape[1]), "reps": args.reps,
        "kernel_ms": round(kernel_s * 1e3, 3), "kernel_bytes": kernel_bytes, "kernel_GBps": round(kernel_bytes / kernel_s / 1e9, 1) if kernel_s else None,
        "kernel_ns_per_marker_step_of_a_wave": round(kernel_s * 1e9 / max(int(np.diff(inp["chain_off"]).max()), 1), 1),
        "call_ms_median": round(call_s * 1e3, 2), "call_ms_min": round(min(calls) * 1e3, 2), "call_bytes": call_bytes,
        "call_GBps": round(call_bytes / call_s / 1e9, 2),
        "numpy_twin_s": round(twin_s, 2), "states_differing_from_twin": differing,
    }))
    return 0 if differing == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
