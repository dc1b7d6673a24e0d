#!/usr/bin/env python3
"""
How many totals of the configs[3] job does the exact-mode certificate send to the second pass?  bench.py answers for ONE seed
(10050: its `checks.strict_reevaluations`); the flag probability of an accession is 2 * B (B = the job's bound, the fractional
part of a PL-weighted total is as good as uniform), so the count of one seed is a draw from a Poisson law of a mean near 0.5 ... 2.
This tool runs the first pass of the same job -- Panel.fill_synthetic(seed), Context.sample_synthetic, run_carry per slab,
Carry.error_bound, Carry.finish -- once for each of several seeds and prints B, the flagged count per seed and the build id of
the library that ran, so that two builds can be compared independently of the draw (SNPMATCH_HIP_LIB=... selects a build).

    python tools/flag_rate.py                            # 10 000 x 50M int8, seeds 10050-10059, slabs as bench.py cuts them
    python tools/flag_rate.py --n-snp 3000000 --slabs 3  # a rehearsal

One pass per seed, no timing loop; the last line is one JSON record.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n-acc", type=int, default=10000)
    ap.add_argument("--n-snp", type=int, default=50_000_000)
    ap.add_argument("--chunk", type=int, default=1000)
    ap.add_argument("--slab-gb", type=float, default=205.0, help="largest resident SNP slab (10^9 bytes), as bench.py")
    ap.add_argument("--slabs", type=int, default=0, help="this many equal slabs (default: as few as fit --slab-gb)")
    ap.add_argument("--seed0", type=int, default=10050)
    ap.add_argument("--seeds", type=int, default=10)
    ap.add_argument("--planted", type=int, default=417)
    ap.add_argument("--packed", action="store_true")
    args = ap.parse_args()

    import torch
    from snpmatch_amd import _lib, engine

    dev = torch.device("cuda:0")
    ctx = engine.Context(0)
    n_acc, n_snp, chunk = args.n_acc, args.n_snp, args.chunk
    planted = args.planted if n_acc > args.planted else n_acc - 1
    pitch = ctx.row_pitch(n_acc, args.packed)
    if args.slabs > 0:
        rows_per_slab = -(-(-(-n_snp // args.slabs)) // chunk) * chunk
    else:
        rows_per_slab = max(chunk, int(args.slab_gb * 1e9 / pitch) // chunk * chunk)
    rows_per_slab = min(rows_per_slab, n_snp)
    slabs = [min(rows_per_slab, n_snp - r0) for r0 in range(0, n_snp, rows_per_slab)]
    starts = [sum(slabs[:k]) for k in range(len(slabs))]
    print("build_id %s  %d accessions x %d SNPs%s  slabs %s" % (_lib.build_id(), n_acc, n_snp, " packed" if args.packed else "", slabs))

    panel = engine.Panel(ctx, rows_per_slab, n_acc, packed=args.packed)
    wei_dev = torch.empty((n_snp, 3), dtype=torch.float64, device=dev)
    carry = engine.Carry(ctx, n_acc)
    rows = []
    for seed in range(args.seed0, args.seed0 + args.seeds):
        ctx.sample_synthetic(seed, 0, n_snp, planted, wei_dev.data_ptr(), err=0.02, frac_pl=0.8)
        queries = [engine.Query.from_device(panel, None, wei_dev[starts[k]:].data_ptr(), slabs[k]) for k in range(len(slabs))]
        carry.reset()
        for k in range(len(slabs)):
            panel.fill_synthetic(seed, snp0=starts[k], acc0=0, row0=0, nrows=slabs[k])
            queries[k].run_carry(carry, chunk, False, engine.MODE_EXACT, sum(-(-s // chunk) for s in slabs[k + 1:]))
        bound = carry.error_bound()
        _, _, flagged = carry.finish(want_results=False)
        for q in queries:
            q.free()
        rows.append({"seed": seed, "B": bound, "flagged": int(carry.n_flagged), "expected": 2.0 * bound * n_acc})
        print("seed %d  B %.6e  flagged %d %s  (2 B n_acc = %.2f)" % (seed, bound, carry.n_flagged, flagged.tolist(), 2.0 * bound * n_acc),
              flush=True)
    carry.free()
    panel.free()
    ctx.close()
    total = sum(r["flagged"] for r in rows)
    print(json.dumps({"build_id": _lib.build_id(), "n_acc": n_acc, "n_snp": n_snp, "slabs": slabs, "packed": args.packed,
                      "B_mean": sum(r["B"] for r in rows) / len(rows), "flagged_total": total, "per_seed": rows}))


if __name__ == "__main__":
    main()
