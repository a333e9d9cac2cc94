"""Child of tests/test_gpu_plane.py, started with NDT_PLANE_MAX_BLOCKS set: the count kernel's blocks stride over the tiles of
small clouds, in both merge forms (NDT_PLANE_MERGE is read at every call).  Models, states and counts against the numpy
restatement; the last line is a JSON verdict."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import plane_cases as pc  # noqa: E402
from toyslam_amd import ndt  # noqa: E402


def main():
    cap = int(os.environ["NDT_PLANE_MAX_BLOCKS"])
    g = ndt.NormalDistributionsTransform()
    done, seen, strided = 0, 0, 0
    picks = [(n, sp) for n, sp in pc.shape_cases() if n >= 1023 or sp["H"] in (1, 257, 513)]
    picks += [(len(xyz), sp, xyz) for xyz, sp in pc.gpu_cases().values()]
    for pick in picks:
        n, sp = pick[0], pick[1]
        xyz = pick[2] if len(pick) > 2 else pc.shape_cloud(n)
        co, st, cn, tri, aux = pc.counts(xyz, sp)
        dc = g.uploadCloud(xyz)
        s = ndt.plane_spec(sp["T"], sp["H"], seed=sp["seed"], axis=sp["axis"], eps_angle=sp["eps"])
        plan = ndt.host_plane_plan(n, sp["H"])
        assert plan["tile_blocks"] == min(plan["tiles"], max(1, cap // plan["hyp_blocks"])), plan
        strided += plan["tile_blocks"] < plan["tiles"]
        for form in ("atomic", "rows"):
            os.environ["NDT_PLANE_MERGE"] = form
            got_co, got_st, got_cn = g.planeCounts(dc, s)
            d = g.planeDiag()
            assert d["count_blocks"] == plan["tile_blocks"] * plan["hyp_blocks"], (d, plan)
            seen = max(seen, plan["tile_blocks"])
            assert np.array_equal(got_st, st) and np.array_equal(got_cn, cn), (n, sp, form)
            assert (np.abs(got_co - co) <= 1e-12 * np.maximum(np.abs(co), 1.0)).all(), (n, sp, form)
            res, inl, oth = g.segmentPlane(dc, s)
            ref = pc.segment(xyz, sp)
            assert (res["best"], res["best_count"], res["n_inliers"], res["n_finite"]) == (ref["best"], ref["best_count"], ref["n_inliers"], ref["n_finite"])
            assert np.array_equal(inl.numpy()[:, :3].view(np.uint32), xyz[ref["inliers"]].view(np.uint32)), (n, sp, form)
            assert np.array_equal(oth.numpy()[:, :3].view(np.uint32), xyz[ref["others"]].view(np.uint32)), (n, sp, form)
        done += 1
    print(json.dumps(dict(ok=True, cases=done, max_tile_blocks_seen=seen, strided=int(strided))))


if __name__ == "__main__":
    main()
