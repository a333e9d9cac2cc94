"""Child of tests/test_gpu_normals.py, started with NDT_NORMAL_MAX_BLOCKS set: the kernel's blocks stride over the passes of
small clouds.  argv[1]: an .npz the parent wrote under the default switch -- per pick its records and counts.  Every pick's
records, counts and stats must be those bits, the kept set of a selection the same indices, and the comparison rules of
tests/normal_cases.py must hold against the numpy reference; the last line is a JSON verdict."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import normal_cases as nc  # noqa: E402
from toyslam_amd import ndt  # noqa: E402

PICKS = (("size n=65", nc.spec(k=8)), ("size n=65", nc.spec(radius=1.2)), ("size n=513", nc.spec(k=8)), ("size n=513", nc.spec(radius=1.2)),
         ("non-finite rows", nc.spec(k=8)), ("non-finite rows", nc.spec(radius=1.2)), ("size n=9", nc.spec(k=8)), ("an integer lattice", nc.spec(k=7)),
         ("100 km from the origin", nc.spec(radius=0.1)), ("a blob and far points", nc.spec(k=8)), ("size n=7", nc.spec(radius=1.2)))


def main():
    cap = int(os.environ["NDT_NORMAL_MAX_BLOCKS"])
    parent = np.load(sys.argv[1])
    g = ndt.NormalDistributionsTransform()
    cases = nc.gpu_cases()
    done, seen = 0, 0
    flt = g.normalFilter(curvature=(0.0, 0.02))
    for j, (name, sp) in enumerate(PICKS):
        xyz = cases[name][0]
        directions = dict((nc.tag_of(s), d) for s, d in cases[name][1])[nc.tag_of(sp)]
        dc = g.uploadCloud(xyz)
        rec, cnt, st = g.estimateNormals(dc, **nc.kw_of(sp))
        d = g.normalDiag()
        assert g.normalPlan(len(xyz))[0] == min(cap, -(-len(xyz) // 8)) and d["blocks"] == g.normalPlan(len(xyz))[0] and d["launches"] == 1, (name, d)
        seen = max(seen, d["blocks"])
        assert rec.tobytes() == parent["rec%d" % j].tobytes() and cnt.tobytes() == parent["cnt%d" % j].tobytes(), (name, nc.tag_of(sp))
        assert [st[k] for k in ("n_finite", "n_valid", "n_collinear", "max_neighbors")] == list(parent["st%d" % j]), (name, st)
        bad = nc.compare(rec, cnt, nc.reference(xyz, sp), sp, xyz, directions)
        assert not bad, (name, nc.tag_of(sp), bad)
        _, _, idx = g.selectByNormals(dc, g.normalSpec(**nc.kw_of(sp)), flt, indices=True)
        assert np.array_equal(idx, parent["idx%d" % j]) and np.array_equal(idx, np.flatnonzero(nc.keep_by(nc.keep_filter(nc.KEEP_CURVATURE, (0.0, 0.02)), rec)))
        done += 1
    print(json.dumps(dict(ok=True, cases=done, max_blocks_seen=seen)))


if __name__ == "__main__":
    main()
