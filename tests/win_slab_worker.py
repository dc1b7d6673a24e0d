"""Child process of tests/test_gpu_windows.py: a context created under the SNPM_WIN_WS_MB of the environment runs
``engine.window_counts`` over all rows of a panel, as a range and as a row list, and writes the results and the launches per kernel.
``in.npz``: snps, rows, win_off, pairs."""
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
    acc_range, pair_range = engine.window_counts(panel, z["win_off"], None, z["pairs"])
    launches = [ctx.profile_read("win_planes")[0], ctx.profile_read("win_count")[0]]
    ctx.profile_reset()
    acc_list, pair_list = engine.window_counts(panel, z["win_off"], None, z["pairs"], z["rows"])
    launches += [ctx.profile_read("win_planes")[0], ctx.profile_read("win_count")[0]]
    panel.free()
    ctx.close()
    np.savez(dst, acc_range=acc_range, pair_range=pair_range, acc_list=acc_list, pair_list=pair_list, launches=np.array(launches))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
