"""CPU: the host upload's repack + bounding-box pass (host_repack_bbox, one point per step, and host_repack_bbox_avx2, two),
run as they are through ndt_host_repack_bbox, against the numpy reference of tests/cloud_box_cases.py -- boxes by value,
repacked records (x, y, z, 1.0f) bit for bit -- and the self-checks of that file's reference and cloud builder.
No GPU is used."""
import ctypes as C
import mmap

import numpy as np
import pytest

import cloud_box_cases as cb
from cloud_box_cases import EMPTY_BOXES, F32, FLT_MAX, boxes_text, build_cloud, reference_boxes, same_boxes, spread_hot

SIZES = [0, 1, 2, 3, 4, 5, 255, 256, 257, 20480]
STRIDES = [12, 16, 20, 32]


@pytest.fixture(scope="module")
def ndt(built_lib):
    from toyslam_amd import ndt as m
    return m


@pytest.fixture(scope="module")
def forms(ndt):
    """the forms this CPU runs: (name, avx2 flag)"""
    return [("scalar", 0)] + ([("avx2", 1)] if _has_avx2(ndt) else [])


def _has_avx2(ndt):
    from toyslam_amd import _lib
    try:
        ndt.host_repack_bbox(np.zeros(3, F32), 1, 12, avx2=True)
    except _lib.NdtError:
        return False
    return True


class EndOfAllocation:
    """`nbytes` bytes that end exactly where an allocation ends: the page behind them cannot be read, so a load that leaves
    the last record ends the process instead of passing unseen"""

    def __init__(self, nbytes):
        self.libc = C.CDLL(None, use_errno=True)
        self.libc.mmap.restype = C.c_void_p
        self.libc.mmap.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_long]
        self.libc.mprotect.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
        self.libc.munmap.argtypes = [C.c_void_p, C.c_size_t]
        page = mmap.PAGESIZE
        self.size = (nbytes + page - 1) // page * page + page
        self.base = self.libc.mmap(None, self.size, mmap.PROT_READ | mmap.PROT_WRITE, mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS, -1, 0)
        assert self.base not in (None, C.c_void_p(-1).value), "mmap failed"
        assert self.libc.mprotect(self.base + self.size - page, page, 0) == 0  # PROT_NONE
        self.addr = self.base + self.size - page - nbytes
        self.bytes = np.ctypeslib.as_array((C.c_ubyte * max(nbytes, 1)).from_address(self.addr))[:nbytes]

    def close(self):
        self.bytes = None
        self.libc.munmap(self.base, self.size)


def run_form(ndt, rec, n, stride, avx2):
    """the records placed so that the buffer ends with the last record (12-byte records: with its z)"""
    nbytes = n * stride
    mem = EndOfAllocation(nbytes)
    try:
        mem.bytes[:] = np.ascontiguousarray(rec).view(np.uint8).reshape(-1)[:nbytes]
        return ndt.host_repack_bbox(mem.bytes, n, stride, avx2=avx2)
    finally:
        mem.close()


def check(ndt, forms, rec, stride):
    n = len(rec)
    ref = reference_boxes(rec) if n else EMPTY_BOXES
    want = np.c_[rec[:, :3], np.ones(n, F32)].astype(F32)
    for name, avx2 in forms:
        out, boxes = run_form(ndt, rec, n, stride, avx2)
        assert same_boxes(boxes, ref), (name, boxes_text(boxes, ref))
        assert out.shape == (n, 4) and np.array_equal(out.view(np.uint32), want.view(np.uint32)), name  # bit for bit, NaN payloads too


# ---- the reference and the builder themselves
def test_reference_follows_the_definition():
    big = F32(1e6)
    b = reference_boxes(np.array([[np.nan, big, big]], F32))  # y and z to box [0], nothing to box [1]
    assert b[0, 0, 0] == FLT_MAX and b[0, 1, 0] == -FLT_MAX and (b[0, :, 1:] == big).all() and same_boxes(b[1:].repeat(2, 0), EMPTY_BOXES[1:].repeat(2, 0))
    assert same_boxes(reference_boxes(np.zeros((0, 3), F32)), EMPTY_BOXES)
    assert (EMPTY_BOXES[:, 0] == FLT_MAX).all() and (EMPTY_BOXES[:, 1] == -FLT_MAX).all()
    b = reference_boxes(np.array([[1, -np.inf, 3], [2, 5, np.inf], [-7, 0, 0.5]], F32))
    assert same_boxes(b, np.array([[[-7, -np.inf, 0.5], [2, 5, np.inf]], [[-7, 0, 0.5], [-7, 0, 0.5]]], F32))
    assert same_boxes(np.array([[[-0.0] * 3] * 2] * 2, F32), np.zeros((2, 2, 3), F32))  # the sign of zero stays invisible
    assert not same_boxes(np.full((2, 2, 3), np.nan, F32), np.full((2, 2, 3), np.nan, F32))
    assert same_boxes(reference_boxes(np.full((9, 4), np.nan, F32)), EMPTY_BOXES)


@pytest.mark.parametrize("variant", cb.VARIANTS)
def test_builder_gives_every_value_one_owner(variant):
    rec, owners = build_cloud(300, spread_hot(300, must=[255, 256, 299, 298]), floats=5, variant=variant, seed=3, nan_rows=[7, 100])
    ref = cb.check_owners(rec, owners)
    assert len(owners) == 12 and sorted(owners) == sorted(cb.SLOTS)
    assert (ref[0, 0] < ref[1, 0]).all() and (ref[0, 1] > ref[1, 1]).all()  # box [0] lies beyond box [1] on every side
    for (v, m, k), row in owners.items():
        assert np.isfinite(rec[row, :3]).all() == (v == 1)  # box [0]'s owners give nothing to box [1]
    if variant == "denormal":
        assert 0 < ref[1, 1, 2] < ref[0, 1, 2] < np.finfo(F32).tiny
    if variant == "fltmax":
        assert ref[0, 0, 0] == -FLT_MAX and ref[0, 1, 0] == FLT_MAX
    if variant == "inf":
        assert ref[0, 1, 1] == np.inf and ref[0, 0, 2] == -np.inf and np.isfinite(ref[1]).all()
    if variant == "far":
        assert np.abs(ref[1]).min() > 9e4
    assert not np.isfinite(rec[:, 3:]).all()  # garbage behind z
    with pytest.raises(AssertionError):  # an owner that owns nothing is found out
        broken = rec.copy()
        broken[owners[(1, 1, 0)], 0] = 0
        cb.check_owners(broken, owners)


def test_small_clouds_still_have_owners_in_either_box():
    for n in range(1, 6):
        rec, owners = build_cloud(n, spread_hot(n), variant="plain")
        assert len(owners) == n and (n < 2 or {v for v, _, _ in owners} == {0, 1})


# ---- the two host forms
@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("n", SIZES)
def test_host_forms_against_the_reference(ndt, forms, n, stride):
    """owners on the first, the last, the last even and the last odd row (the AVX2 form's pair loop ends at the last even
    count; 12-byte records take a narrow load for the very last one)"""
    last_even, last_odd = (n - 1) // 2 * 2, (n - 2) // 2 * 2 + 1
    for j, variant in enumerate(cb.VARIANTS):
        must = [[n - 1, 0, last_even, last_odd], [last_odd, last_even, n - 3, 0], [0, n - 2, n - 1, n - 4]][j % 3]
        rec, _ = build_cloud(n, spread_hot(n, must=must), floats=max(3, stride // 4), variant=variant, seed=stride + j)
        check(ndt, forms, np.ascontiguousarray(rec[:, :stride // 4]), stride)


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("n", [1, 2, 5, 256, 257])
def test_all_nan_clouds_have_empty_boxes(ndt, forms, n, stride):
    rec = np.full((n, stride // 4), np.nan, F32)
    check(ndt, forms, rec, stride)
    rec[:, 0] = 3.0  # x alone: box [0] has an x, box [1] stays empty
    check(ndt, forms, rec, stride)
    assert same_boxes(reference_boxes(rec)[1:].repeat(2, 0), EMPTY_BOXES[1:].repeat(2, 0))


@pytest.mark.parametrize("stride", [12, 16])
def test_every_row_in_turn_owns_the_far_corner(ndt, forms, stride):
    """one finite outlier moved through every row of a cloud of 9 (pairs, the odd row, the narrow last load)"""
    base, _ = build_cloud(9, [], floats=stride // 4, seed=5)
    for row in range(9):
        rec = base.copy()
        rec[row, :3] = [500.0, -600.0, 700.0]
        check(ndt, forms, rec, stride)


def test_bad_arguments_are_refused(ndt, forms):
    from toyslam_amd import _lib
    lib = _lib.lib()
    rec = np.zeros((4, 4), F32)
    out, b = np.zeros((5, 4), F32), np.zeros(12, F32)
    fp = C.POINTER(C.c_float)
    aligned = out.ctypes.data + (-out.ctypes.data) % 16
    for stride in (8, 14):
        assert lib.ndt_host_repack_bbox(rec.ctypes.data, 4, stride, 0, aligned, b.ctypes.data_as(fp)) == _lib.NDT_ERR_INVALID
    assert lib.ndt_host_repack_bbox(rec.ctypes.data, 4, 16, 0, aligned + 4, b.ctypes.data_as(fp)) == _lib.NDT_ERR_INVALID
    assert lib.ndt_host_repack_bbox(None, 4, 16, 0, aligned, b.ctypes.data_as(fp)) == _lib.NDT_ERR_INVALID
    assert lib.ndt_host_repack_bbox(rec.ctypes.data, 4, 16, 0, aligned, None) == _lib.NDT_ERR_INVALID
    assert lib.ndt_host_repack_bbox(None, 0, 16, 0, None, b.ctypes.data_as(fp)) == _lib.NDT_OK
    assert same_boxes(b.reshape(2, 2, 3), EMPTY_BOXES)
    if len(forms) == 1:  # a CPU without AVX2 refuses the two-point form
        assert lib.ndt_host_repack_bbox(rec.ctypes.data, 4, 16, 1, aligned, b.ctypes.data_as(fp)) == _lib.NDT_ERR_INVALID
