"""CPU: export and import of the accumulating target (ndt_target_accumulate_export / _import / _save / _load) -- the entries
are declared, exported, in SIGNATURES and wrapped; every device-free refusal comes with its code and a word of its message on
a handle that never asks for a device (blobs crafted in numpy: each header field wrong in turn, a payload bit flipped,
truncated and over-long buffers); the checksum agrees with a pure-Python restatement; the zero-row blob imports without a
device; TilePager's tile arithmetic gives back exactly a tile's cells; and the header parser survives mutated blobs under
ASan + UBSan (tests/acc_blob_fuzz.cpp, a stand-alone CPU program)."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ("ndt_target_accumulate_export", "ndt_target_accumulate_import", "ndt_target_accumulate_save", "ndt_target_accumulate_load",
       "ndt_diag_target_export", "ndt_host_acc_blob_info", "ndt_host_acc_blob_checksum")
METHODS = ("targetAccumulateExport", "targetAccumulateImport", "targetAccumulateSave", "targetAccumulateLoad", "targetExportDiag")
FUNCTIONS = ("acc_blob_info", "acc_blob_checksum", "acc_blob_rows")
LIM = 1 << 20
RESOLUTIONS = (1.0, 0.5, 0.3, 0.1)
MASK = (1 << 64) - 1


@pytest.fixture(scope="module")
def mods(built_lib):
    from toyslam_amd import _lib, ndt
    return built_lib, _lib, ndt


def last_error(L):
    return L.ndt_last_error().decode()


def fnv(words, h=0xcbf29ce484222325):
    """the issue's checksum, restated: per 8-byte word h = (h ^ w) * 0x100000001b3 mod 2^64"""
    for w in words:
        h = ((h ^ int(w)) * 0x100000001b3) & MASK
    return h


def make_blob(ndt, rows, resolution=1.0, lo=None, hi=None, n_voxels=None, magic=b"NDTACC1\0", version=1, row_bytes=104, word5=0,
              checksum=None):
    """a blob from a structured array of rows, every header field open to a wrong value; the checksum is right unless given"""
    rows = np.asarray(rows, dtype=ndt.ACC_ROW_DTYPE)
    cells = np.c_[rows["i"], rows["j"], rows["k"]].reshape(-1, 3)
    if lo is None:
        lo = cells.min(axis=0) if len(rows) else (0, 0, 0)
    if hi is None:
        hi = cells.max(axis=0) if len(rows) else (0, 0, 0)
    head = struct.pack("<8sIIfIQ3i3i", magic, version, row_bytes, resolution, word5, len(rows) if n_voxels is None else n_voxels,
                       *[int(v) for v in lo], *[int(v) for v in hi])
    assert len(head) == 56
    body = head + rows.tobytes()
    if checksum is None:
        checksum = fnv(np.frombuffer(body[:len(body) // 8 * 8], dtype="<u8"))
    return head + struct.pack("<Q", checksum) + rows.tobytes()


def two_rows(ndt):
    rows = np.zeros(2, dtype=ndt.ACC_ROW_DTYPE)
    rows["i"], rows["j"], rows["k"], rows["count"] = [3, -2], [0, 5], [-7, 4], [2, 9]   # ascending key: k is the high part
    rows["d"] = np.arange(18, dtype=np.float64).reshape(2, 9) + 0.5
    rows["f"] = [[1, 2, 3], [4, 5, 6]]
    return rows


def test_entries_are_declared_exported_and_wrapped(mods):
    L, _lib, ndt = mods
    with open(os.path.join(ROOT, "include", "ndt_mi355.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None
        assert re.search(r"\b%s\(" % name, header), name + " is not declared in include/ndt_mi355.h"
    for method in METHODS:
        assert callable(getattr(ndt.NormalDistributionsTransform, method))
    for fn in FUNCTIONS:
        assert callable(getattr(ndt, fn))
    assert ndt.ACC_ROW_DTYPE.itemsize == 104
    assert [ndt.ACC_ROW_DTYPE.fields[k][1] for k in ("i", "j", "k", "count", "d", "f", "pad")] == [0, 4, 8, 12, 16, 88, 100]
    from toyslam_amd import tiles
    assert callable(tiles.TilePager)


@pytest.mark.parametrize("n_words", [0, 1, 7, 300])
def test_checksum_agrees_with_its_restatement(mods, n_words):
    L, _lib, ndt = mods
    words = np.random.default_rng(n_words).integers(0, 1 << 63, n_words, dtype=np.uint64) * np.uint64(2) + np.uint64(n_words % 2)
    assert ndt.acc_blob_checksum(words.astype("<u8").tobytes()) == fnv(words)
    if n_words == 0:
        assert ndt.acc_blob_checksum(b"") == 0xcbf29ce484222325
    out = C.c_uint64(0)
    assert L.ndt_host_acc_blob_checksum(words.ctypes.data, 8 * n_words + 3, C.byref(out)) == _lib.NDT_ERR_INVALID
    assert "multiple of 8" in last_error(L)


def test_blob_info_of_a_hand_made_blob(mods):
    L, _lib, ndt = mods
    rows = two_rows(ndt)
    blob = make_blob(ndt, rows, resolution=0.5)
    assert len(blob) == 64 + 2 * 104
    info = ndt.acc_blob_info(blob)
    assert info["resolution"] == 0.5 and info["n_voxels"] == 2
    assert info["lo"].tolist() == [-2, 0, -7] and info["hi"].tolist() == [3, 5, 4]
    back = ndt.acc_blob_rows(blob)
    assert back.tobytes() == rows.tobytes() and back["count"].tolist() == [2, 9]
    # the checksum field is the hash of bytes [0, 56) followed by the rows
    assert struct.unpack_from("<Q", blob, 56)[0] == ndt.acc_blob_checksum(blob[:56] + blob[64:])
    keys = [ndt.host_acc_pack_cell(r["i"], r["j"], r["k"]) for r in rows]
    assert keys[0] < keys[1]
    empty = make_blob(ndt, rows[:0], resolution=0.25)
    assert len(empty) == 64 and ndt.acc_blob_info(empty)["n_voxels"] == 0


def test_device_free_refusals(mods):
    L, _lib, ndt = mods
    rows = two_rows(ndt)
    good = make_blob(ndt, rows)
    g = ndt.NormalDistributionsTransform()   # no device is asked for
    g.setResolution(1.0)

    def refused(blob, word, nbytes=None):
        b = np.frombuffer(bytes(blob), dtype=np.uint8)
        nbytes = len(b) if nbytes is None else nbytes
        assert L.ndt_target_accumulate_import(g._h, b.ctypes.data, nbytes) == _lib.NDT_ERR_INVALID, word
        assert word in last_error(L), (word, last_error(L))
        assert L.ndt_host_acc_blob_info(b.ctypes.data, nbytes, None, None, None, None) == _lib.NDT_ERR_INVALID, word
        assert word in last_error(L), (word, last_error(L))
        assert g.targetAccumulated() == dict(points=0, voxels=0, updates=0)

    assert L.ndt_target_accumulate_import(None, good, len(good)) == _lib.NDT_ERR_INVALID
    assert "null handle" in last_error(L)
    assert L.ndt_target_accumulate_import(g._h, None, 64) == _lib.NDT_ERR_INVALID
    assert "null blob" in last_error(L)
    refused(good[:63], "shorter")
    refused(good, "shorter", nbytes=0)
    refused(make_blob(ndt, rows, magic=b"NDTACC2\0"), "magic")
    refused(make_blob(ndt, rows, magic=b"ndtacc1\0"), "magic")
    refused(make_blob(ndt, rows, version=2), "version")
    refused(make_blob(ndt, rows, version=0), "version")
    refused(make_blob(ndt, rows, row_bytes=96), "row_bytes")
    refused(make_blob(ndt, rows, n_voxels=3), "64 + 104")
    refused(make_blob(ndt, rows, n_voxels=1), "64 + 104")
    refused(make_blob(ndt, rows, n_voxels=(1 << 64) - 1), "64 + 104")
    refused(good[:-1], "64 + 104")                                # truncated
    refused(good[:64 + 104], "64 + 104")                          # a whole row short
    refused(good + b"\0", "64 + 104")                             # over-long
    refused(good + bytes(104), "64 + 104")
    refused(make_blob(ndt, rows, checksum=0), "checksum")
    for bit in (64 * 8, 64 * 8 + 77, len(good) * 8 - 1, 16 * 8 + 3, 20 * 8, 57 * 8):   # payload, resolution, the spare word, the sum
        flipped = bytearray(good)
        flipped[bit // 8] ^= 1 << (bit % 8)
        refused(flipped, "checksum")
    for res in (0.0, -1.0, float("nan"), float("inf")):
        refused(make_blob(ndt, rows, resolution=res), "finite and positive")
    refused(make_blob(ndt, rows, lo=(4, 0, -7)), "lo > hi")
    refused(make_blob(ndt, rows, lo=(-2, 0, -LIM - 1)), "outside [-2^20, 2^20)")
    refused(make_blob(ndt, rows, hi=(3, LIM, 4)), "outside [-2^20, 2^20)")
    # a well-formed blob of another resolution than the handle's: refused without a device as well
    other = make_blob(ndt, rows, resolution=0.5)
    assert ndt.acc_blob_info(other)["resolution"] == 0.5
    b = np.frombuffer(other, dtype=np.uint8)
    assert L.ndt_target_accumulate_import(g._h, b.ctypes.data, len(b)) == _lib.NDT_ERR_INVALID
    assert "resolution" in last_error(L)
    with pytest.raises(_lib.NdtError) as e:
        g.targetAccumulateImport(other)
    assert e.value.status == _lib.NDT_ERR_INVALID
    assert g.targetAccumulated() == dict(points=0, voxels=0, updates=0)


def test_zero_row_blob_imports_without_a_device(mods, tmp_path):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    g.setResolution(0.5)
    empty = make_blob(ndt, np.zeros(0, ndt.ACC_ROW_DTYPE), resolution=0.5)
    assert g.targetAccumulateImport(empty) == dict(points=0, voxels=0, updates=0)
    path = tmp_path / "empty.ndtacc"
    path.write_bytes(empty)
    assert g.targetAccumulateLoad(path) == dict(points=0, voxels=0, updates=0)
    with pytest.raises(_lib.NdtError) as e:
        g.grid()
    assert e.value.status == _lib.NDT_ERR_NO_INPUT                # still no target


def test_export_save_load_without_a_target_or_a_file(mods, tmp_path):
    L, _lib, ndt = mods
    g = ndt.NormalDistributionsTransform()
    n = C.c_size_t(7)
    f3 = lambda *v: (C.c_float * 3)(*v)   # noqa: E731
    assert L.ndt_target_accumulate_export(None, None, None, None, 0, C.byref(n)) == _lib.NDT_ERR_INVALID
    assert "null handle" in last_error(L)
    assert L.ndt_diag_target_export(None, None, None, None) == _lib.NDT_ERR_INVALID
    for a, b in ((None, f3(1, 1, 1)), (f3(0, 0, 0), None)):
        assert L.ndt_target_accumulate_export(g._h, a, b, None, 0, C.byref(n)) == _lib.NDT_ERR_INVALID
        assert "one bound" in last_error(L)
    assert L.ndt_target_accumulate_export(g._h, f3(0, float("nan"), 0), f3(1, 1, 1), None, 0, C.byref(n)) == _lib.NDT_ERR_INVALID
    assert "NaN" in last_error(L)
    assert L.ndt_target_accumulate_export(g._h, f3(0, 2, 0), f3(1, 1, 1), None, 0, C.byref(n)) == _lib.NDT_ERR_INVALID
    assert "min > max" in last_error(L)
    for a, b in ((None, None), (f3(0, 0, 0), f3(1, 1, 1))):
        assert L.ndt_target_accumulate_export(g._h, a, b, None, 0, C.byref(n)) == _lib.NDT_ERR_NO_INPUT
        assert "no accumulated target" in last_error(L)
    assert n.value == 7                                           # nothing written
    with pytest.raises(_lib.NdtError) as e:
        g.targetAccumulateExport()
    assert e.value.status == _lib.NDT_ERR_NO_INPUT
    with pytest.raises(ValueError):
        g.targetAccumulateExport([0, 0, 0], None)
    target = tmp_path / "map.ndtacc"
    with pytest.raises(_lib.NdtError) as e:
        g.targetAccumulateSave(target)
    assert e.value.status == _lib.NDT_ERR_NO_INPUT and not target.exists() and list(tmp_path.iterdir()) == []
    assert L.ndt_target_accumulate_save(g._h, None, None, None) == _lib.NDT_ERR_INVALID
    assert "null path" in last_error(L)
    assert L.ndt_target_accumulate_load(g._h, None) == _lib.NDT_ERR_INVALID
    assert "null path" in last_error(L)
    missing = tmp_path / "nowhere" / "map.ndtacc"
    with pytest.raises(_lib.NdtError) as e:
        g.targetAccumulateLoad(missing)
    assert e.value.status == _lib.NDT_ERR_INVALID and str(missing) in str(e.value) and "No such file" in str(e.value)
    with pytest.raises(_lib.NdtError) as e:
        g.targetAccumulateLoad(tmp_path)                          # a directory
    assert e.value.status == _lib.NDT_ERR_INVALID and str(tmp_path) in str(e.value)
    garbage = tmp_path / "garbage.ndtacc"
    garbage.write_bytes(b"not a blob at all" * 9)
    with pytest.raises(_lib.NdtError) as e:
        g.targetAccumulateLoad(garbage)
    assert e.value.status == _lib.NDT_ERR_INVALID and "magic" in str(e.value)
    assert g.targetExportDiag() == dict(voxels=0, points=0, launches=0)
    assert g.targetAccumulated() == dict(points=0, voxels=0, updates=0)


@pytest.mark.parametrize("resolution", RESOLUTIONS)
def test_tile_arithmetic(mods, resolution):
    """cells -> tile -> box -> crop_cell_range gives back exactly the tile's cells: at the ends of the lattice, across zero"""
    L, _lib, ndt = mods
    from toyslam_amd import tiles
    g = ndt.NormalDistributionsTransform()
    g.setResolution(resolution)
    for S in (1, 8, 10, 1 << 10):
        pager = tiles.TilePager.__new__(tiles.TilePager)
        pager.handle, pager.tile_cells, pager.radius, pager.tile = g, S, 1, None
        cells = np.array([-LIM, -LIM + 1, -LIM + S - 1, -LIM + S, -2 * S, -S - 1, -S, -S + 1, -1, 0, 1, S - 1, S, S + 1, 12345, LIM - S - 1, LIM - S,
                          LIM - 2, LIM - 1], np.int64)
        t = tiles.tile_of_cell(cells, S)
        assert np.array_equal(t, cells // S)
        lo, hi = tiles.tile_cell_range(t, S)
        assert (lo <= cells).all() and (cells <= hi).all() and (hi - lo <= S - 1).all()
        inner = (lo > -LIM) & (hi < LIM - 1)
        assert np.array_equal((hi - lo)[inner], np.full(int(inner.sum()), S - 1)) and np.array_equal(lo[inner] % S, np.zeros(int(inner.sum())))
        assert tiles.tile_of_cell(-1, S) == -1 and tiles.tile_of_cell(0, S) == 0   # across zero: floor, not truncation
        mn, mx = tiles.cell_box(resolution, lo, hi)
        assert mn.dtype == np.float32 and mx.dtype == np.float32
        back_lo, back_hi = ndt.crop_cell_range(resolution, mn, mx)
        assert np.array_equal(back_lo, lo) and np.array_equal(back_hi, hi)
        # three axes at once through the pager, and a position goes to the tile of its cell
        for k in range(0, len(cells) - 2, 3):
            c3 = cells[k:k + 3]
            tile = tuple(int(v) for v in tiles.tile_of_cell(c3, S))
            assert pager.tile_at(ndt.crop_cell_centre(resolution, c3)) == tile
            bmn, bmx = pager.tile_box(tile)
            got_lo, got_hi = ndt.crop_cell_range(resolution, bmn, bmx)
            want_lo, want_hi = tiles.tile_cell_range(tile, S)
            assert np.array_equal(got_lo, want_lo) and np.array_equal(got_hi, want_hi)
            wmn, wmx = pager.window_box(tile)
            wlo, whi = ndt.crop_cell_range(resolution, wmn, wmx)
            assert np.array_equal(wlo, np.clip((np.array(tile) - 1) * S, -LIM, LIM - 1))
            assert np.array_equal(whi, np.clip((np.array(tile) + 2) * S - 1, -LIM, LIM - 1))
            assert tile in pager.window(tile) and len(pager.window(tile)) <= 27
        assert pager.window_cells() == (3 * S) ** 3


def test_blob_parser_survives_mutated_blobs_under_sanitizers(tmp_path):
    """tests/acc_blob_fuzz.cpp: 5000 mutated blobs through the header parser and the checksum, built with ASan + UBSan (a
    stand-alone CPU program): accepted or refused, never a crash or an out-of-bounds access."""
    csrc = os.path.join(ROOT, "toyslam_amd", "csrc")
    exe = str(tmp_path / "acc_blob_fuzz")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + csrc,
                           os.path.join(ROOT, "tests", "acc_blob_fuzz.cpp"), os.path.join(csrc, "ndt_acc_blob.cpp"), "-o", exe])
    out = subprocess.run([exe, "5000"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "no crash" in out.stdout
    accepted, refused = (int(v) for v in re.search(r"(\d+) accepted, (\d+) refused", out.stdout).groups())
    assert accepted > 0 and refused > 0 and accepted + refused == 5000
