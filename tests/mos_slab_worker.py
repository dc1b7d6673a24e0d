"""Child process of tests/test_gpu_mosaic.py: a context created under the SNPM_MOS_WS_MB of the environment runs ``engine.mosaic``
over a row list of a panel and writes the results and the launches per kernel.  ``in.npz``: snps, rows, classes, chain_off, cost, S."""
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
    state, chain_cost, col_cost = engine.mosaic(panel, z["classes"], z["chain_off"], z["cost"], int(z["S"]), None, z["rows"], want_col_cost=True)
    launches = [ctx.profile_read(k)[0] for k in ("win_planes", "mos_fwd", "mos_back")]
    panel.free()
    ctx.close()
    np.savez(dst, state=state, chain_cost=chain_cost, col_cost=col_cost, launches=np.array(launches))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
