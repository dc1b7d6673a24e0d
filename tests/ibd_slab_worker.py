"""Child process of tests/test_gpu_ibd.py: a context created under the SNPM_IBD_WS_MB / SNPM_IBD_BITS_MB of the environment runs
``engine.ibd_counts`` and writes the results and the launches per kernel.  ``in.npz``: mode, snps, win_off and
  mode "slabs":  rows, wide -- the scan over all rows as a range and as the row list, then the window set ``wide``
  mode "refuse": small -- the call that must be refused (its message is written), then the window set ``small`` that fits."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from snpmatch_amd import engine  # noqa: E402

KERNELS = ("win_planes", "ibd_count", "ibd_runs")


def main(src, dst):
    z = np.load(src)
    ctx = engine.Context(0)
    panel = engine.Panel.from_host(ctx, z["snps"], packed=bool(z["packed"]))
    args = [int(v) for v in z["params"]]
    out = {}
    if str(z["mode"]) == "slabs":
        ctx.profile(True)
        launches = []
        for name, win_off, rows in (("range", z["win_off"], None), ("list", z["win_off"], z["rows"]), ("wide", z["wide"], None)):
            ctx.profile_reset()
            got = engine.ibd_counts(panel, win_off, *args, rows=rows)
            launches.append([ctx.profile_read(k)[0] for k in KERNELS])
            out.update({name + "_" + k: v for k, v in got.items()})
        out["launches"] = np.array(launches)
    else:
        try:
            engine.ibd_counts(panel, z["win_off"], *args)
            out["message"] = np.array("")
        except AssertionError as err:
            out["message"] = np.array(str(err))
        out.update(engine.ibd_counts(panel, z["small"], *args))
    panel.free()
    ctx.close()
    np.savez(dst, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
