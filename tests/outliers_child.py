"""Child of tests/test_gpu_outliers.py, started with NDT_OUTLIER_MAX_BLOCKS set: the value kernel's blocks stride over the
passes of small clouds.  Values, statistics and kept sets against the numpy reference; the last line is a JSON verdict."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import outlier_cases as oc  # noqa: E402
from toyslam_amd import ndt  # noqa: E402


def main():
    cap = int(os.environ["NDT_OUTLIER_MAX_BLOCKS"])
    g = ndt.NormalDistributionsTransform()
    cases = oc.gpu_cases()
    done, seen = 0, 0
    picks = [("surface", oc.stat(8)), ("surface", oc.stat(65)), ("surface", oc.rad(0.3, 3)), ("non-finite rows", oc.stat(8)),
             ("non-finite rows", oc.rad(0.3, 3)), ("far points", oc.stat(8)), ("plan n=17", oc.stat(2)), ("plan n=9", oc.rad(0.7, 1)),
             ("|F| = 8 + 0", oc.stat(8)), ("100 km from the origin", oc.rad(0.05, 1))]
    for name, spec in picks:
        xyz = cases[name][0]
        ref = oc.reference(xyz, **spec)
        kw = dict(radius=spec["radius"], min_neighbors=spec["min_neighbors"]) if spec["method"] == oc.RADIUS else dict(mean_k=spec["mean_k"], stddev_mul=spec["stddev_mul"])
        dc = g.uploadCloud(xyz)
        values, st = g.neighborValues(dc, **kw)
        d = g.outlierDiag()
        assert d["value_blocks"] == min(cap, g.outlierPlan(len(xyz))[0]), (name, d)
        seen = max(seen, d["value_blocks"])
        fin = ~np.isnan(ref["values"])
        assert np.array_equal(np.isnan(values), ~fin), name
        assert (np.abs(values[fin] - ref["values"][fin]) <= 1e-12 * np.abs(ref["values"][fin])).all(), (name, spec)
        assert st["n_finite"] == ref["n_finite"] and st["n_valid"] == ref["n_valid"]
        assert abs(st["mean"] - ref["mean"]) <= 1e-11 * abs(ref["mean"]) and abs(st["stddev"] - ref["stddev"]) <= 1e-9 * abs(ref["stddev"])
        got, st2, idx = g.removeOutliers(dc, indices=True, **kw)
        assert np.array_equal(idx, np.flatnonzero(ref["keep"])), (name, spec)
        assert np.array_equal(got.numpy()[:, :3].view(np.uint32), xyz[ref["keep"]].view(np.uint32)), (name, spec)
        done += 1
    print(json.dumps(dict(ok=True, cases=done, max_blocks_seen=seen)))


if __name__ == "__main__":
    main()
