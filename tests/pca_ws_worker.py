"""Child process of tests/test_gpu_pca.py: a context created under the SNPM_PCA_WS_MB of the environment runs ``engine.gram`` and
``engine.loadings`` over all rows of ``snps`` (``in.npz``) with the integer table and vec and with the real ones; the four results and
the launches of win_planes / pca_gram / pca_fold (of one ``gram`` call) and pca_load (of one ``loadings`` call) are written."""
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
    ctx.profile(True)
    ctx.profile_reset()
    out["gram_int"] = engine.gram(panel, z["tab_int"])
    out["load_int"] = engine.loadings(panel, z["tab_int"], z["vec_int"])
    out["launches"] = np.array([ctx.profile_read(name)[0] for name in ("win_planes", "pca_gram", "pca_fold", "pca_load")])
    ctx.profile(False)
    out["gram_real"] = engine.gram(panel, z["tab_real"])
    out["load_real"] = engine.loadings(panel, z["tab_real"], z["vec_real"])
    panel.free()
    ctx.close()
    np.savez(dst, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
