"""The grids ndt_align_pairs builds (every small target from one k1_small_multi launch) and the grids single handles build for
the same clouds (k1_small), saved to one .npz for tests/test_gpu_pairs.py to compare bit for bit.  The small form's switches
(NDT_K1_SMALL_LIST, NDT_K1_LDS_CAP, NDT_K1_SMALL_FINISH) are read once per process: one run per regime.
   pairs_grids_check.py OUT.npz"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from toyslam_amd import clouds, ndt  # noqa: E402

KEYS = ("idx", "n", "mean", "cov", "icov", "evals", "min_b", "max_b", "div_b", "n_valid")


def small_clouds():
    """Clouds of a handful of points up to the small form's 49 152, scenes and crowds: a crowd's voxels hold thousands of
    points, so its buckets overflow the wave lists at NDT_K1_SMALL_LIST=8 and, the largest, at the default capacity too."""
    rng = np.random.default_rng(47)
    cl = [clouds.target_surfaces(n, seed=n, extent=e) for n, e in ((6, 100.0), (700, 20.0), (5000, 60.0), (16000, 100.0), (49152, 100.0))]
    cl.append(clouds.target_uniform(12000, seed=3))
    for n_ctr, n in ((20, 24000), (2, 40000)):
        ctr = clouds.target_uniform(n_ctr, seed=n_ctr)
        cl.append((ctr[rng.integers(0, n_ctr, n)] + rng.normal(0, 0.05, (n, 3))).astype(np.float32))
    return cl


def with_non_finite(cl):
    rng = np.random.default_rng(48)
    out = []
    for c in cl:
        c = c.copy()
        bad = rng.choice(len(c), max(1, len(c) // 50), replace=False)
        c[bad[0::2], 0] = np.nan
        c[bad[1::2], 2] = np.inf
        out.append(c)
    return out


def main():
    out = {}
    base = small_clouds()
    for form, cl, dense in (("dense", base, True), ("nonfinite", with_non_finite(base), False)):
        g = ndt.NormalDistributionsTransform()
        g.setMaximumIterations(1)
        g.alignPairs(cl, [(c, c) for c in range(len(cl))], is_dense=dense)
        ref = ndt.NormalDistributionsTransform()
        for c in range(len(cl)):
            ref.setInputTarget(cl[c], is_dense=dense)
            for who, grid in (("pairs", g.pairsGrid(c)), ("single", ref.grid())):
                for k in KEYS:
                    out["%s%d_%s_%s" % (form, c, who, k)] = np.asarray(grid[k])
    out["n_clouds"] = np.asarray(len(base))
    np.savez(sys.argv[1], **out)
    print("pairs grids of %d clouds x 2 saved" % len(base))


if __name__ == "__main__":
    main()
