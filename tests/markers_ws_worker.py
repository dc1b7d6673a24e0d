"""Child process of tests/test_gpu_markers.py: a context created under the SNPM_MK_WS_MB of the environment runs
``engine.marker_select`` over all rows of ``snps`` (``in.npz``), which must be refused -- the message is written -- and then over the
first ``fit`` rows with five markers at most, which fit the budget: those results are written."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from snpmatch_amd import engine  # noqa: E402


def main(src, dst):
    z = np.load(src)
    ctx = engine.Context(0)
    panel = engine.Panel.from_host(ctx, z["snps"], packed=False)
    out = {}
    try:
        engine.marker_select(panel)
        out["message"] = np.array("")
    except AssertionError as err:
        out["message"] = np.array(str(err))
    got = engine.marker_select(panel, max_markers=5, rows=range(0, int(z["fit"])))
    out.update({k: np.asarray(v) for k, v in got.items()})
    panel.free()
    ctx.close()
    np.savez(dst, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
