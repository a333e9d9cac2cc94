"""CPU: the inputs of tests/test_gpu_cloud_ops_shared.py (tests/cloud_ops_cases.py) are what that test needs them to be, and
the one plan rule behind the four named plans (ndt_cloud_ops.hpp range_plan) tiles a cloud as each of them did."""
import numpy as np
import pytest

import cloud_box_cases as cb
import cloud_ops_cases as cc
from toyslam_amd import ndt


def test_the_clouds_pass_their_own_checks(built_lib):
    single, many = cc.checked()
    assert tuple(single) == cc.SIZES and tuple(len(r) for r in many) == cc.LIST
    for rec in list(single.values()) + many:
        assert rec.dtype == np.float32 and rec.shape[1] == 4 and not rec.flags.writeable
        ref = cb.reference_boxes(rec)
        finite = np.isfinite(rec[:, :3]).all(1)
        # the last row owns a box value, and the two boxes differ wherever the cloud is large enough to hold owners of both
        less = cb.reference_boxes(rec[:-1]) if len(rec) > 1 else cb.EMPTY_BOXES
        assert (less != ref).any()
        if len(rec) >= 63:
            assert not finite.all() and (ref[0] != ref[1]).any()


def test_a_row_with_a_zero_coordinate_would_not_survive_the_identity(built_lib):
    """why the clouds hold no -0.0: p + 0.0 is +0.0"""
    q, _ = ndt.host_deskew_point(cc.identity_motion(), np.array([-0.0, 1.0, 2.0], np.float32), cc.TIME)
    assert cc.bits(q)[0] == 0 and cc.bits(np.float32(-0.0)) == 0x80000000


@pytest.mark.parametrize("n", (0, 1, 255, 256, 257, 4096, 4097, 262144, 262145, 1048577, 2 ** 31 - 1))
def test_the_named_plans_follow_one_rule(built_lib, n):
    """blocks * per covers n, (blocks - 1) * per does not, per is the floor until the cap binds"""
    for (blocks, per), floor, cap in ((ndt.NormalDistributionsTransform.selectPlan(n), 256, 1024), (ndt.host_deskew_plan(n), 256, 1024)):
        assert per == max(floor, -(-n // cap)) and blocks == -(-n // per) and blocks <= cap
        assert blocks * per >= n > (blocks - 1) * per or n == 0 == blocks


def test_the_shared_host_pieces_under_sanitizers(tmp_path):
    """tests/cloud_ops_host_check.cpp: a stand-alone program over ndt_cloud_ops.hip's host code (plan, row fold, member table,
    preamble, environment cap), host side built with -fsanitize=address,undefined; it makes no device call."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    exe = str(tmp_path / "cloud_ops_host_check")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I" + os.path.join(root, "include"),
                           "-I" + os.path.join(root, "toyslam_amd", "csrc"), os.path.join(root, "tests", "cloud_ops_host_check.cpp"),
                           "-x", "hip", os.path.join(root, "toyslam_amd", "csrc", "ndt_cloud_ops.hip"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "cloud_ops_host_check: ok" in out.stdout, out.stderr[-2000:]
