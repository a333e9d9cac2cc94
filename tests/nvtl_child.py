"""Child process of tests/test_gpu_nvtl.py: the two development switches that are read once per process (NDT_K2_MAX_BLOCKS,
NDT_SCORE_POSES_CHUNK) need a process of their own.  It only COMPUTES -- what the GPU returns, as hex floats in a JSON file --
and the parent does the comparing.

    python tests/nvtl_child.py capped  out.json     (run with NDT_K2_MAX_BLOCKS=3)
    python tests/nvtl_child.py chunked out.json     (run with NDT_SCORE_POSES_CHUNK=2)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import score_poses_cases as spc  # noqa: E402

CAPPED_SIZES = (769, 1537)   # three blocks of 256: from 769 points a thread walks several
POSES = (spc.I_IDENTITY, spc.I_GOLDEN, 2, 3, spc.I_FAR)   # the five poses of both modes


def hexes(v):
    return [float(x).hex() for x in v]


def main(mode, out_path):
    from oracle import pyoracle as po
    from toyslam_amd import ndt
    d = np.load(os.path.join(ROOT, "tests", "golden", "pair_0p1.npz"))
    t, s = d["target"], d["source"]
    with open(os.path.join(ROOT, "tests", "golden", "oracle_golden.json")) as f:
        golden = json.load(f)
    all_poses = spc.poses(golden)
    P = [all_poses[k] for k in POSES]
    out = {}
    if mode == "capped":
        for method in spc.METHODS:
            g = ndt.NormalDistributionsTransform()
            g.setNeighborhoodSearchMethod(getattr(po, method))
            g.setInputTarget(t)
            for n in CAPPED_SIZES:
                c = s[:n]
                g.setInputSource(c)
                v, nf = g.nvtlPoses(P, counts=True)
                launches, blocks = g.nvtlLaunches()
                single = [g.calculateNVTL(spc.moved(po, c, T)) for T in P]
                points = [g.sourcePointNVTL(T) for T in P]
                out["%s/%d" % (method, n)] = dict(
                    poses=hexes(v), found=[int(x) for x in nf], launches=launches, blocks=blocks,
                    single=hexes([x[0] for x in single]), single_found=[x[1] for x in single],
                    reduced=hexes([x[1] for x in points]), per_point=[hexes(x[0]) for x in points],
                    plan_blocks=g.evalPlan(n)["launch_blocks"])
    elif mode == "chunked":
        g = ndt.NormalDistributionsTransform()
        g.setInputTarget(t)
        g.setInputSource(s)
        v, nf = g.nvtlPoses(P, counts=True)
        out = dict(poses=hexes(v), found=[int(x) for x in nf], launches=g.nvtlLaunches()[0], blocks=g.nvtlLaunches()[1],
                   plan_blocks=g.evalPlan(len(s))["launch_blocks"])
    else:
        raise SystemExit("unknown mode " + mode)
    with open(out_path, "w") as f:
        json.dump(out, f)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
