"""Child process of tests/test_gpu_mixture.py: a context created under the SNPM_MIX_WS_MB of the environment runs
``engine.mix_counts`` over all rows as a range and over a row list, and writes the two tables and the launches per kernel.
``in.npz``: snps, packed, alt, ref, rows, alt_rows, ref_rows (the counts of the row list)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from snpmatch_amd import engine  # noqa: E402

KERNELS = ("win_planes", "mix_count")


def main(src, dst):
    z = np.load(src)
    ctx = engine.Context(0)
    panel = engine.Panel.from_host(ctx, z["snps"], packed=bool(z["packed"]))
    ctx.profile(True)
    out, launches = {}, []
    for name, alt, ref, rows in (("range", z["alt"], z["ref"], None), ("list", z["alt_rows"], z["ref_rows"], z["rows"])):
        ctx.profile_reset()
        out[name] = engine.mix_counts(panel, alt, ref, rows=rows)
        launches.append([ctx.profile_read(k)[0] for k in KERNELS])
    out["launches"] = np.array(launches)
    panel.free()
    ctx.close()
    np.savez(dst, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
