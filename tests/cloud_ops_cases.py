"""Shared by the cloud-operation tests (no GPU): clouds on which a keep-everything selection and a deskew under the identity
motion must both return the input -- so that the two users of the shared box fold (ndt_cloud_ops.hpp TwoBox: k_select_place,
k_deskew) can be held to each other and to the boxes of an upload.

The clouds are cloud_box_cases.build_cloud's: every one of the 12 box values is owned by one row, the last row (a point of
the last block of every plan) among the owners; owners of box [0] carry a NaN, some variants an infinity or FLT_MAX.  What
the comparison needs of them is checked here, on the CPU, by checked(), before anything touches the GPU:
  no coordinate is +0.0 or -0.0  (the deskew's identity is p + 0.0, which turns -0.0 into +0.0);
  ndt_host_deskew_point -- the function the kernel calls -- under IDENTITY at the test's time returns every row bit for bit
  (rows with a coordinate that is not finite go through as they are; a finite time, so no row is untimed)."""
import functools

import numpy as np

import cloud_box_cases as cb

SIZES = (1, 63, 64, 65, 255, 256, 257, 513)  # wave, block and two-block edges of the 256-thread plans
LIST = (63, 257, 513)                        # the sizes of the list form's three clouds
TIME = 0.5


def identity_motion():
    from toyslam_amd import ndt
    return ndt.host_deskew_motion(np.eye(4, dtype=np.float32), 0.0, 1.0, 0.0)


def records(n, seed):
    """(n, 4) float32: the fourth word is garbage (NaN, inf, huge) that both operations must copy as it is"""
    hot = cb.spread_hot(n, must=[n - 1])
    nan_rows = [r for r in (n // 3, n // 2 + 1) if 0 <= r < n and r not in hot]
    rec, owners = cb.build_cloud(n, hot, floats=4, variant=cb.VARIANTS[seed % 4], seed=seed, nan_rows=nan_rows)  # (not "far")
    assert n - 1 in owners.values()
    return rec


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def checked():
    """-> ({n: records}, [records of the list]), read-only, after the CPU checks of the module's docstring"""
    from toyslam_amd import ndt
    m = identity_motion()
    assert m.angle == 0.0 and tuple(m.tau_ref) == (0.0, 0.0, 0.0)
    single = {n: records(n, i) for i, n in enumerate(SIZES)}
    many = [records(n, 40 + i) for i, n in enumerate(LIST)]
    for rec in list(single.values()) + many:
        assert not (rec[:, :3] == 0).any()
        for row in rec:
            q, untimed = ndt.host_deskew_point(m, row[:3], TIME)
            assert not untimed and np.array_equal(bits(q), bits(row[:3])), row
        rec.setflags(write=False)
    return single, many
