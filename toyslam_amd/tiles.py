"""TilePager: the accumulated target of a handle kept to a window of tiles around the vehicle, the rest paged to disk.

A crop (targetAccumulateCrop) is final: what leaves the window is lost.  The pager saves every tile that leaves the window
(targetAccumulateSave with the tile's box) before it crops, and loads every entering tile that has a file
(targetAccumulateLoad) afterwards -- voxels cross bit for bit, so the window holds what a target that was never cropped
holds in the same cells.  Tiles are cubes of `tile_cells` cells on the absolute lattice: tile t covers the cells
[t * S, (t + 1) * S - 1] on every axis.  The window is the cube of tiles within `radius_tiles` of the vehicle's tile.  The
pager allocates nothing on the device and keeps no state but the current tile and the directory.

What the caller owes: between two move_to calls, points are accumulated only into cells of the current window (a sensor
range of radius_tiles * tile_cells cells, less the way the vehicle goes between two calls).  A voxel accumulated outside the
window is dropped by the next crop, and a tile that comes back while the target already holds one of its cells is refused
by the import ("cell already in the target"): a cell must never exist on both sides."""
import itertools
import os

import numpy as np

from . import ndt as _ndt


def tile_of_cell(cell, tile_cells):
    """the tile of a cell, per axis: floor(cell / S)"""
    return np.floor_divide(np.asarray(cell, dtype=np.int64), int(tile_cells))


def tile_cell_range(tile, tile_cells):
    """(lo, hi): the cells of a tile, clipped to the lattice [-2^20, 2^20)"""
    t = np.asarray(tile, dtype=np.int64)
    lo, hi = t * int(tile_cells), (t + 1) * int(tile_cells) - 1
    return np.clip(lo, -_ndt.ACC_CELL_LIMIT, _ndt.ACC_CELL_LIMIT - 1), np.clip(hi, -_ndt.ACC_CELL_LIMIT, _ndt.ACC_CELL_LIMIT - 1)


def cell_box(resolution, lo, hi):
    """(min_xyz, max_xyz) that crop_cell_range turns back into exactly the cells [lo, hi]: the centres of the corner cells"""
    return _ndt.crop_cell_centre(resolution, lo), _ndt.crop_cell_centre(resolution, hi)


class TilePager:
    def __init__(self, handle, directory, tile_cells, radius_tiles):
        if int(tile_cells) < 1 or int(radius_tiles) < 0:
            raise ValueError("tile_cells must be >= 1 and radius_tiles >= 0")
        self.handle, self.directory = handle, os.fspath(directory)
        self.tile_cells, self.radius = int(tile_cells), int(radius_tiles)
        self.tile = None   # the vehicle's tile; None before the first move_to
        os.makedirs(self.directory, exist_ok=True)

    # ---- arithmetic
    def tile_at(self, xyz):
        """the tile of a position: the tile of the cell the target bins it into"""
        p = np.asarray(xyz, dtype=np.float32).reshape(3)
        cell, _ = _ndt.crop_cell_range(self.handle.getResolution(), p, p)
        return tuple(int(v) for v in tile_of_cell(cell, self.tile_cells))

    def window(self, tile):
        """the tiles within radius_tiles of `tile`, as a set"""
        r = range(-self.radius, self.radius + 1)
        limit = -(-_ndt.ACC_CELL_LIMIT // self.tile_cells)
        out = set()
        for d in itertools.product(r, r, r):
            t = tuple(tile[k] + d[k] for k in range(3))
            if all(-limit <= v < limit for v in t):   # a tile with a cell on the lattice
                out.add(t)
        return out

    def tile_box(self, tile):
        return cell_box(self.handle.getResolution(), *tile_cell_range(tile, self.tile_cells))

    def window_box(self, tile):
        lo, _ = tile_cell_range(tuple(v - self.radius for v in tile), self.tile_cells)
        _, hi = tile_cell_range(tuple(v + self.radius for v in tile), self.tile_cells)
        return cell_box(self.handle.getResolution(), lo, hi)

    def window_cells(self):
        """how many cells a window has at the most"""
        return ((2 * self.radius + 1) * self.tile_cells) ** 3

    def path(self, tile):
        return os.path.join(self.directory, "tile_%d_%d_%d.ndtacc" % tuple(tile))

    # ---- paging
    def _save(self, tile):
        """the tile's voxels to its file, overwriting it"""
        mn, mx = self.tile_box(tile)
        self.handle.targetAccumulateSave(self.path(tile), mn, mx)

    def move_to(self, xyz):
        """The vehicle is at xyz.  Nothing happens while its tile stays; otherwise the tiles that leave the window are saved,
        the target is cropped to the new window and the entering tiles that have a file are loaded."""
        tile = self.tile_at(xyz)
        if tile == self.tile:
            return False
        old = self.window(self.tile) if self.tile is not None else None
        new = self.window(tile)
        if self.handle.targetAccumulated()["updates"] > 0:
            if old is not None:
                for t in sorted(old - new):
                    self._save(t)
            self.handle.targetAccumulateCrop(*self.window_box(tile))
        for t in sorted(new - old if old is not None else new):
            if os.path.exists(self.path(t)):
                self.handle.targetAccumulateLoad(self.path(t))
        self.tile = tile
        return True

    def flush(self):
        """every tile of the window to its file"""
        if self.tile is None or self.handle.targetAccumulated()["updates"] == 0:
            return
        for t in sorted(self.window(self.tile)):
            self._save(t)
