"""Child of tests/test_gpu_clusters.py, started with NDT_CLUSTER_MAX_BLOCKS set: the link kernel's blocks stride over the
passes of small clouds.  Labels, roots, tables, indices and kept sets against the numpy reference, exactly; the last line is a
JSON verdict."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import cluster_cases as cc  # noqa: E402
from toyslam_amd import ndt  # noqa: E402


def main():
    cap = int(os.environ["NDT_CLUSTER_MAX_BLOCKS"])
    g = ndt.NormalDistributionsTransform()
    cases = cc.gpu_cases()
    done, seen = 0, 0
    picks = [("components over many cells", cc.spec(0.5, 10)), ("chain, shuffled", cc.spec(0.5)), ("non-finite rows", cc.spec(0.5, 5)),
             ("far points", cc.spec(0.5)), ("plan n=17", cc.spec(0.7)), ("plan n=9", cc.spec(0.7, 2)), ("plan n=65", cc.spec(0.3, 1, 3)),
             ("equal sizes", cc.spec(0.8, 3, 5)), ("100 km from the origin", cc.spec(0.05)), ("duplicate pairs", cc.spec(1e-6, 2, 2))]
    for name, sp in picks:
        xyz = cases[name][0]
        ref = cc.reference(xyz, **sp)
        dc = g.uploadCloud(xyz)
        labels, table, indices, summary, roots = g.clusterCloud(dc, roots=True, **sp)
        d = g.diagClusters()
        assert g.clusterPlan(len(xyz))[0] == min(cap, -(-len(xyz) // 8)) and d["link_blocks"] == g.clusterPlan(len(xyz))[0], (name, d)
        seen = max(seen, d["link_blocks"])
        assert summary == ref["summary"], (name, summary, ref["summary"])
        assert np.array_equal(labels, ref["labels"]) and np.array_equal(roots, ref["roots"]) and np.array_equal(indices, ref["indices"]), name
        for f in ("root", "size", "first", "box_min", "box_max"):
            assert np.array_equal(table[f], ref["table"][f]), (name, f)
        got, s2, idx = g.extractClusters(dc, indices=True, **sp)
        assert s2 == summary and np.array_equal(idx, np.flatnonzero(ref["keep"])), (name, sp)
        assert np.array_equal(got.numpy()[:, :3].view(np.uint32), xyz[ref["keep"]].view(np.uint32)), (name, sp)
        done += 1
    print(json.dumps(dict(ok=True, cases=done, max_blocks_seen=seen)))


if __name__ == "__main__":
    main()
