"""Child of tests/test_gpu_deskew.py, started with NDT_DESKEW_MAX_BLOCKS set: a few blocks walk clouds of a few thousand
points in several passes each.  Records, counts and boxes against the numpy restatement; the last line is a JSON verdict."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import cloud_box_cases as cbc  # noqa: E402
import deskew_cases as dc  # noqa: E402
from toyslam_amd import _lib, ndt  # noqa: E402

F = np.float32


def raw(g, cloud):
    n = len(cloud)
    out = np.zeros((max(n, 1), 4), dtype=F)
    assert g._L.ndt_cloud_download(g._h, cloud._c, out.ctypes.data, 16) == 0
    return out[:n].view(np.uint32).copy()


def main():
    cap = int(os.environ["NDT_DESKEW_MAX_BLOCKS"])
    g = ndt.NormalDistributionsTransform()
    m = dc.make_motion([0.02, -0.01, 0.3], [1.0, 0.05, -0.02], 1.7e9, 1.7e9 + 0.1, 1.7e9 + 0.03)
    cm = dc.to_ctypes(m, _lib.DeskewMotion)
    done, seen, max_ppb = 0, 0, 0
    clouds, motions, times_all, singles = [], [], [], []
    for n in (2, 700, 769, 3000, 4099, 6145):
        blocks, ppb = ndt.host_deskew_plan(n)
        assert blocks == min(cap, (n + 255) // 256) and (blocks - 1) * ppb < n <= blocks * ppb, (n, blocks, ppb)
        rec = dc.build_records(n, seed=n, offset=(1e5, 0, -1e5) if n == 4099 else (0, 0, 0), odd_every=7 if n > 7 else 0)
        times = dc.build_times(n, m, seed=n, untimed_every=11 if n > 11 else 0, at_ref_every=13 if n > 13 else 0)
        cloud = g.uploadCloud(rec)
        rec_u = raw(g, cloud)
        out, nu = g.deskewCloud(cloud, cm, times)
        d = g.deskewDiag()
        assert d == dict(launches=1, blocks=blocks, clouds=1), (n, d)
        got = raw(g, out)
        assert dc.expected_records(rec_u, times, m, got) == nu, n
        dc.check_moved(got.view(F)[:, :3], rec_u.view(F), times, m, n)
        boxes, route = out.bounds()
        ref = cbc.reference_boxes(got.view(F)[:, :3])
        assert cbc.same_boxes(boxes, ref) and route == "deskew", (n, cbc.boxes_text(boxes, ref))
        seen, max_ppb = max(seen, blocks), max(max_ppb, ppb)
        clouds.append(cloud)
        motions.append(cm)
        times_all.append(times)
        singles.append((got, nu, boxes))
        done += 1
    outs, nus = g.deskewClouds(clouds, motions, times_all)     # ... and all of them in one launch
    d = g.deskewDiag()
    assert d["launches"] == 1 and d["clouds"] == len(clouds) and d["blocks"] == sum(ndt.host_deskew_plan(len(c))[0] for c in clouds), d
    for out, nu, (got, nu1, boxes) in zip(outs, nus, singles):
        assert np.array_equal(raw(g, out), got) and nu == nu1 and np.array_equal(out.bounds()[0], boxes)
    print(json.dumps(dict(ok=True, cases=done, max_blocks_seen=seen, max_ppb=max_ppb)))


if __name__ == "__main__":
    main()
