"""Child process of tests/test_gpu_gicp_lockstep.py: the development switches that are read once per process
(NDT_GICP_LOCKSTEP_MEMBERS, NDT_GICP_MAX_BLOCKS, NDT_GICP_NO_FUSE) need a process of their own.  It only COMPUTES -- five
consecutive pairs through gicp_align_pairs_lockstep and through gicp_align_pairs_clouds under the same switches, as hex
floats in a JSON file -- and the parent does the comparing.

    python tests/gicp_lockstep_child.py out.json
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gicp_lockstep_cases as lc  # noqa: E402


def main(out_path):
    from toyslam_amd import gicp, ndt
    up = ndt.NormalDistributionsTransform()
    dcs = [up.uploadCloud(c) for c in lc.noisy_subsets(lc.CHILD_SIZES, seed=29)]
    guesses = lc.child_guesses()
    g = gicp.GeneralizedIterativeClosestPoint()
    lock = g.alignPairsLockstep(dcs, None, guesses, 1.0)
    diag = g.diagLockstep()
    seq = g.alignPairsClouds(dcs, None, guesses, 1.0)
    plan = [g.plan(n) for n in lc.CHILD_SIZES]
    with open(out_path, "w") as f:
        json.dump(dict(lockstep=lc.to_json(lock), sequential=lc.to_json(seq), diag=diag, plan=plan), f)


if __name__ == "__main__":
    main(sys.argv[1])
