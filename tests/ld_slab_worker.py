"""Child process of tests/test_gpu_ld.py: a context created under the SNPM_LD_WS_MB of the environment runs ``engine.ld_band`` over
all rows of a panel, as a range and as a row list, and writes the results and the launches per kernel.  ``in.npz``: snps, rows,
band."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from snpmatch_amd import engine  # noqa: E402


def main(src, dst):
    z = np.load(src)
    ctx = engine.Context(0)
    panel = engine.Panel.from_host(ctx, z["snps"], packed=True)
    ctx.profile(True)
    ctx.profile_reset()
    counts_range, r2_range = engine.ld_band(panel, int(z["band"]))
    launches = [ctx.profile_read("ld_planes")[0], ctx.profile_read("ld_band")[0]]
    ctx.profile_reset()
    counts_list, r2_list = engine.ld_band(panel, int(z["band"]), None, z["rows"])
    launches += [ctx.profile_read("ld_planes")[0], ctx.profile_read("ld_band")[0]]
    panel.free()
    ctx.close()
    np.savez(dst, counts_range=counts_range, r2_range=r2_range, counts_list=counts_list, r2_list=r2_list, launches=np.array(launches))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
