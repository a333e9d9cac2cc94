"""The two users of the one box fold (ndt_cloud_ops.hpp TwoBox: k_select_place, k_deskew) against each other and against the
upload path: a selection that keeps everything and a deskew under the identity motion both return their input, so

    records of selectCloud(c)  ==  records of deskewCloud(c, IDENTITY)  ==  the records of c        bit for bit, all four words,
    bounds() of either         ==  bounds() of an upload of those rows                              all 12 floats, bit for bit,

for the single calls at the wave, block and two-block edges of the 256-thread plans and for the list forms over three such
clouds.  What the inputs must be for this to hold (no +-0.0 coordinate, the host's deskew_point returns every row as it is) is
checked on the CPU by cloud_ops_cases.checked() before the handle is made; tests/test_cloud_ops_cases.py runs it without a GPU."""
import numpy as np
import pytest

import cloud_ops_cases as cc


@pytest.fixture(scope="module")
def env(built_lib):
    single, many = cc.checked()  # (CPU checks first)
    assert built_lib.ndt_device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    from toyslam_amd import ndt
    return ndt.NormalDistributionsTransform(), cc.identity_motion(), single, many


def words(g, dc):
    """all four words of every record"""
    from toyslam_amd import _lib
    out = np.zeros((max(len(dc), 1), 4), dtype=np.float32)
    _lib.check(g._L.ndt_cloud_download(g._h, dc._c, out.ctypes.data, 16))
    return cc.bits(out[:len(dc)])


def same_as_input(g, rec, dc, selected, deskewed, untimed, what):
    """dc: the resident input (its fourth word is whatever the upload made of the caller's)"""
    assert untimed == 0 and len(selected) == len(deskewed) == len(rec), what
    resident = words(g, dc)
    assert np.array_equal(resident[:, :3], cc.bits(rec[:, :3])), what
    assert np.array_equal(words(g, selected), resident), what
    assert np.array_equal(words(g, deskewed), resident), what
    (sb, sr), (db, dr), (ub, _) = selected.bounds(), deskewed.bounds(), g.uploadCloud(rec).bounds()
    print(what, "box words that differ: select / deskew", int((cc.bits(sb) != cc.bits(db)).sum()), "select / upload",
          int((cc.bits(sb) != cc.bits(ub)).sum()))
    assert (sr, dr) == ("select", "deskew"), what
    assert np.array_equal(cc.bits(sb), cc.bits(db)) and np.array_equal(cc.bits(sb), cc.bits(ub)), what


@pytest.mark.gpu
@pytest.mark.parametrize("n", cc.SIZES)
def test_keep_everything_and_identity_deskew_agree(env, n):
    g, identity, single, _ = env
    rec = single[n]
    dc = g.uploadCloud(rec)
    deskewed, untimed = g.deskewCloud(dc, identity, np.full(n, cc.TIME))
    same_as_input(g, rec, dc, g.selectCloud(dc), deskewed, untimed, "n = %d" % n)


@pytest.mark.gpu
def test_the_list_forms_agree(env):
    g, identity, _, many = env
    dcs = [g.uploadCloud(rec) for rec in many]
    selected = g.selectClouds(dcs)
    deskewed, untimed = g.deskewClouds(dcs, [identity] * len(dcs), [np.full(len(rec), cc.TIME) for rec in many])
    assert g.selectDiag()["launches"] == 2 and g.deskewDiag()["launches"] == 1
    for k, rec in enumerate(many):
        same_as_input(g, rec, dcs[k], selected[k], deskewed[k], untimed[k], "list entry %d (n = %d)" % (k, len(rec)))
