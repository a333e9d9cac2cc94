"""Child process of tests/test_gpu_pose_cov.py: NDT_K2_MAX_BLOCKS is read once per process, so the strided walk of
k_grad_outer needs a process of its own.  It only COMPUTES -- what the GPU returns, as hex floats in a JSON file -- and the
parent does the comparing.

    python tests/pose_cov_child.py capped out.json     (run with NDT_K2_MAX_BLOCKS=3)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import score_poses_cases as spc  # noqa: E402

CAPPED_SIZES = (768, 769, 2000)   # three blocks of 256: from 769 points a thread walks several


def hexes(v):
    return [float(x).hex() for x in np.asarray(v, dtype=np.float64).ravel()]


def main(mode, out_path):
    from oracle import pyoracle as po
    from toyslam_amd import ndt
    if mode != "capped":
        raise SystemExit("unknown mode " + mode)
    d = np.load(os.path.join(ROOT, "tests", "golden", "pair_0p1.npz"))
    t, s = d["target"], d["source"]
    with open(os.path.join(ROOT, "tests", "golden", "oracle_golden.json")) as f:
        T = spc.golden_T(json.load(f))
    out = {}
    for method in spc.METHODS:
        g = ndt.NormalDistributionsTransform()
        g.setNeighborhoodSearchMethod(getattr(po, method))
        g.setInputTarget(t)
        for n in CAPPED_SIZES:
            g.setInputSource(s[:n])
            cov, I = g.poseCovariance(T, info=True)
            launches, blocks = g.poseCovarianceLaunches()
            out["%s/%d" % (method, n)] = dict(B=hexes(I["B"]), g=hexes(I["g"]), A=hexes(I["A"]), cov=hexes(cov), n_found=I["n_found"],
                                              launches=launches, blocks=blocks, plan_blocks=g.evalPlan(n)["launch_blocks"])
    with open(out_path, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
