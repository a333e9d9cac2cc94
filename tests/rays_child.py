"""Child of tests/test_gpu_clear_rays.py, started with NDT_RAYS_MAX_BLOCKS set: a few blocks walk scans of a few thousand rays
in several passes.  Cells, miss counts, hit flags and the totals against tests/ray_cases.py, one cloud and several in one call,
then a clearing; the last line is a JSON verdict."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import ray_cases as rc  # noqa: E402
from toyslam_amd import ndt  # noqa: E402

F = np.float32


def main():
    cap = int(os.environ["NDT_RAYS_MAX_BLOCKS"])
    rng = np.random.default_rng(cap)
    res = 0.7
    leaf = float(F(res))
    g = ndt.NormalDistributionsTransform()
    g.setResolution(res)
    cloud = (rng.uniform(-9, 9, (2500, 3)) * [1, 1, 0.3]).astype(F)
    g.targetAccumulate(cloud)
    vox = np.floor(cloud * (F(1.0) / F(res))).astype(np.int64)
    done, seen, max_passes = 0, 0, 0
    scans, origins = [], []
    for n in (2, 700, 769, 3000, 4099):
        blocks, passes = ndt.host_ray_plan(n)
        assert blocks == min(cap, (n + 255) // 256) and blocks * 256 * (passes - 1) < n <= blocks * 256 * passes, (n, blocks, passes)
        origin = rc.off_faces(rng, rng.uniform(-1, 1, 3), leaf)
        scan = rc.clear_points(rc.off_faces(rng, rng.uniform(-8.5, 8.5, (n, 3)) * [1, 1, 0.3], leaf), origin, res, margin=leaf)
        scan[1::97] = np.nan
        ref = rc.call_counts(vox, [(scan, origin)], res, leaf, min_clearance=rc.CLEAR)
        up = g.uploadCloud(scan)
        got = g.targetRayCounts(up, None, origin)
        d = g.targetClearRaysDiag()
        assert np.array_equal(got["cells"], ref["cells"]) and np.array_equal(got["miss"], ref["miss"]) and np.array_equal(got["hit"], ref["hit"]), n
        assert (d["rays_cast"], d["rays_skipped"], d["cells_visited"], d["launches"]) == (ref["cast"], ref["skipped"], ref["visited"], 1), (n, d)
        seen, max_passes = max(seen, blocks), max(max_passes, passes)
        scans.append(up)
        origins.append(origin)
        done += 1
    # ... all of them in one launch: the misses summed over the clouds
    host = [np.zeros((max(len(s), 1), 4), F) for s in scans]
    parts = []
    for s, h, o in zip(scans, host, origins):
        assert g._L.ndt_cloud_download(g._h, s._c, h.ctypes.data, 16) == 0
        parts.append((h[:len(s), :3], o))
    ref = rc.call_counts(vox, parts, res, leaf, min_clearance=rc.CLEAR)
    got = g.targetRayCounts(scans, None, origins)
    d = g.targetClearRaysDiag()
    assert np.array_equal(got["miss"], ref["miss"]) and np.array_equal(got["hit"], ref["hit"])
    assert (d["rays_cast"], d["rays_skipped"], d["cells_visited"], d["launches"]) == (ref["cast"], ref["skipped"], ref["visited"], 1), d
    before = g.targetAccumulated()["voxels"]
    gone = int(((ref["miss"] >= 2) & ~ref["hit"]).sum())
    assert g.targetClearRays(scans, None, origins)["voxels"] == before - gone and 0 < gone < before
    d = g.targetClearRaysDiag()
    assert d["removed_voxels"] == gone and d["launches"] == 6, d
    print(json.dumps(dict(ok=True, cases=done, max_blocks_seen=seen, max_passes=max_passes)))


if __name__ == "__main__":
    main()
