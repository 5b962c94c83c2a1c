"""Minimal OpenVDB (.vdb, file version >= 222, FloatGrid Tree_float_5_4_3) reader -> dense numpy volume (read_vdb_dense) or the list of
its 8^3 leaves as bricks (read_vdb_bricks, what SetVolumeBricks takes).

Replaces `Texture3D::FromVDB` (src/Texture3D.cpp:12-82), which uses OpenVDB v10.0.0 (absent submodule):
dense-ify the grid over `file_bbox`, fill active tiles, require max == 1 (:74).
Handles what the reference's cloud files use: no zip/blosc, optional active-mask compression.
Format notes: SURVEY.md App. E.
"""
import struct
import zlib

import numpy as np


class _R:
    def __init__(self, data):
        self.d, self.p = data, 0

    def take(self, n):
        b = self.d[self.p:self.p + n]
        self.p += n
        return b

    def u8(self):
        return self.take(1)[0]

    def i8(self):
        return struct.unpack("<b", self.take(1))[0]

    def u32(self):
        return struct.unpack("<I", self.take(4))[0]

    def i32(self):
        return struct.unpack("<i", self.take(4))[0]

    def i64(self):
        return struct.unpack("<q", self.take(8))[0]

    def f32(self):
        return struct.unpack("<f", self.take(4))[0]

    def string(self):
        return self.take(self.u32()).decode("latin1")

    def meta(self):
        out = {}
        for _ in range(self.u32()):
            name, typ = self.string(), self.string()
            size = self.u32()
            payload = self.take(size)
            if typ == "vec3i":
                out[name] = struct.unpack("<3i", payload)
            elif typ == "int64":
                out[name] = struct.unpack("<q", payload)[0]
            elif typ == "string":
                out[name] = payload.decode("latin1")
            else:
                out[name] = payload
        return out


def _mask(r, nbits):
    return np.unpackbits(np.frombuffer(r.take(nbits // 8), np.uint8), bitorder="little").astype(bool)


def _values(r, count, mask, flags, background):
    """'compressed value array' (SURVEY App. E item 5)."""
    meta = r.i8()
    inactive0, inactive1 = background, -background if meta != 0 else background
    if meta in (2, 4, 5):
        inactive0 = r.f32()
        if meta == 5:
            inactive1 = r.f32()
    if meta == 1:
        inactive0 = -background
    sel = None
    if meta in (3, 4, 5):
        sel = _mask(r, count)
    n = int(mask.sum()) if (flags & 2) and meta != 6 else count
    if flags & 1:
        nbytes = r.i64()
        raw = zlib.decompress(r.take(nbytes)) if nbytes > 0 else r.take(-nbytes)
    else:
        raw = r.take(4 * n)
    vals = np.frombuffer(raw, "<f4", count=n)
    if n == count:
        return vals.copy()
    out = np.full(count, inactive0, np.float32)
    if sel is not None:
        out[sel] = inactive1
    out[mask] = vals
    return out


def _grid_header(r):
    """reads the file header and the first grid's metadata: (version, grid name, grid type, grid / block / end positions, flags, metadata)"""
    magic = r.i64()
    assert magic == 0x56444220, "not a VDB file"
    version = r.u32()
    r.u32()
    r.u32()                 # library major / minor
    r.u8()                  # has grid offsets
    r.take(36)              # uuid
    r.meta()
    n_grids = r.u32()
    assert n_grids >= 1
    name, gtype = r.string(), r.string()
    r.string()              # instance parent
    grid_pos, block_pos, end_pos = r.i64(), r.i64(), r.i64()
    assert "Tree_float_5_4_3" in gtype, gtype
    r.p = grid_pos
    flags = r.u32()
    gmeta = r.meta()
    return version, name, gtype, grid_pos, block_pos, end_pos, flags, gmeta


def vdb_bbox(path):
    """the file's active-voxel bounding box: (min xyz, max xyz), inclusive integer index coordinates"""
    with open(path, "rb") as f:
        gmeta = _grid_header(_R(f.read()))[7]
    return tuple(int(v) for v in gmeta["file_bbox_min"]), tuple(int(v) for v in gmeta["file_bbox_max"])


def union_bbox(paths):
    """the smallest bbox holding every file's bbox: densify all frames of a sequence over it (read_vdb_dense(path, bbox)) and they share
    one grid -- what a renderer whose volume is replaced frame by frame (NrcHpmRenderer.SetVolume) needs"""
    boxes = [vdb_bbox(p) for p in paths]
    if not boxes:
        raise ValueError("union_bbox: no files")
    return (tuple(int(min(b[0][k] for b in boxes)) for k in range(3)), tuple(int(max(b[1][k] for b in boxes)) for k in range(3)))


def _read_tree(path):
    """parses the first grid: (version, name, flags, grid metadata, tiles [(origin, dim, value)] -- the active ones --, leaves [(origin, value
    mask, values)] in file order); origins are integer index coordinates, a leaf's 512 values are ordered n = x<<6 | y<<3 | z"""
    with open(path, "rb") as f:
        r = _R(f.read())
    version, name, gtype, grid_pos, block_pos, end_pos, flags, gmeta = _grid_header(r)
    r.string()              # transform type (UniformScaleMap etc.); payload skipped by seeking via topology parse below
    # transform payload length depends on the map type; topology starts right after it.  All maps used by the
    # WDAS cloud files are UniformScaleMap = 5 x vec3d
    r.take(120)
    assert r.u32() == 1     # buffer count
    background = r.f32()
    n_tiles, n_children = r.u32(), r.u32()
    tiles = []
    origins = []            # leaf origins in topology order
    for _ in range(n_tiles):
        o = np.array([r.i32(), r.i32(), r.i32()])
        v, act = r.f32(), r.u8()
        if act:
            tiles.append((o, 4096, v))
    for _ in range(n_children):
        o5 = np.array([r.i32(), r.i32(), r.i32()])
        cm5, vm5 = _mask(r, 32768), _mask(r, 32768)
        vals5 = _values(r, 32768, vm5, flags, background)
        for n in np.nonzero(vm5 & ~cm5)[0]:
            tiles.append((o5 + 128 * np.array([n >> 10, (n >> 5) & 31, n & 31]), 128, vals5[n]))
        for n in np.nonzero(cm5)[0]:
            o4 = o5 + 128 * np.array([n >> 10, (n >> 5) & 31, n & 31])
            cm4, vm4 = _mask(r, 4096), _mask(r, 4096)
            vals4 = _values(r, 4096, vm4, flags, background)
            for k in np.nonzero(vm4 & ~cm4)[0]:
                tiles.append((o4 + 8 * np.array([k >> 8, (k >> 4) & 15, k & 15]), 8, vals4[k]))
            for k in np.nonzero(cm4)[0]:
                origins.append(o4 + 8 * np.array([k >> 8, (k >> 4) & 15, k & 15]))
                _mask(r, 512)
    assert r.p == block_pos, (r.p, block_pos)
    leaves = []
    for o3 in origins:
        vm = _mask(r, 512)
        leaves.append((o3, vm, _values(r, 512, vm, flags, background)))
    assert r.p == end_pos, (r.p, end_pos)
    return version, name, flags, gmeta, tiles, leaves


def read_vdb_dense(path, bbox=None):
    """Returns (volume float32 indexed [x][y][z], info dict).  The volume covers the file's bbox, or `bbox` = (min xyz, max xyz)
    (inclusive integer index coordinates) when given: data outside it is cropped, voxels inside it but outside the file's bbox are zero."""
    version, name, flags, gmeta, tiles, leaves = _read_tree(path)
    fmin, fmax = np.array(gmeta["file_bbox_min"]), np.array(gmeta["file_bbox_max"])
    if bbox is None:
        bmin, bmax = fmin, fmax
    else:
        bmin, bmax = np.array(bbox[0], np.int64), np.array(bbox[1], np.int64)
        if bmin.shape != (3,) or bmax.shape != (3,) or (bmax < bmin).any():
            raise ValueError("read_vdb_dense: bbox must be ((x0, y0, z0), (x1, y1, z1)) with x1 >= x0 ...")
    ext = bmax - bmin + 1
    vol = np.zeros(tuple(ext), np.float32)
    active_voxels = 0
    for o, dim, value in tiles:
        lo = np.maximum(o - bmin, 0)
        hi = np.minimum(o - bmin + dim, ext)
        if (hi > lo).all():
            vol[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = value
        active_voxels += dim ** 3
    for o3, vm, vals in leaves:
        active_voxels += int(vm.sum())
        blk = np.where(vm, vals, 0.0).astype(np.float32).reshape(8, 8, 8)   # n = x<<6 | y<<3 | z
        lo = o3 - bmin
        if (lo >= 0).all() and (lo + 8 <= ext).all():
            sub = vol[lo[0]:lo[0] + 8, lo[1]:lo[1] + 8, lo[2]:lo[2] + 8]
            sub[vm.reshape(8, 8, 8)] = blk[vm.reshape(8, 8, 8)]
        else:
            for n in np.nonzero(vm)[0]:
                p = lo + np.array([n >> 6, (n >> 3) & 7, n & 7])
                if (p >= 0).all() and (p < ext).all():
                    vol[tuple(p)] = vals[n]
    info = dict(version=version, name=name, bbox_min=tuple(fmin), bbox_max=tuple(fmax), extent=tuple(int(e) for e in ext),
                dense_bbox_min=tuple(int(v) for v in bmin), dense_bbox_max=tuple(int(v) for v in bmax),
                file_voxel_count=gmeta.get("file_voxel_count"), active_voxels=active_voxels, flags=flags)
    return vol, info


def aligned_bbox(bbox):
    """bbox with its minimum snapped down to multiples of 8 (the maximum stays): over such a bbox the file's 8^3 leaves fall on the
    aligned cells of the grid, which read_vdb_bricks and SetVolumeBricks need"""
    return tuple(int(v) // 8 * 8 for v in bbox[0]), tuple(int(v) for v in bbox[1])


def read_vdb_bricks(path, bbox):
    """The file as the brick list of SetVolumeBricks, without building the dense array: (origins int32 [n][3], bricks float32
    [n][8][8][8]).  The coordinates and axes are those of the dense path -- scene.bricks_to_volume(origins, bricks, (ez, ey, ex)) equals
    read_vdb_dense(path, bbox)[0].transpose(2, 1, 0), the [nz][ny][nx] order quantize_density makes: origin = leaf origin - bbox minimum
    as (x, y, z), a brick is [dz][dy][dx] (the leaf's n = x<<6 | y<<3 | z transposed).  Inactive voxels are 0, active tiles are expanded
    into constant bricks, everything outside bbox is cropped, and bricks left without a non-zero voxel are dropped.
    bbox = (min xyz, max xyz), inclusive, its minimum a multiple of 8 in every axis (aligned_bbox), else ValueError."""
    bmin, bmax = np.array(bbox[0], np.int64), np.array(bbox[1], np.int64)
    if bmin.shape != (3,) or bmax.shape != (3,) or (bmax < bmin).any():
        raise ValueError("read_vdb_bricks: bbox must be ((x0, y0, z0), (x1, y1, z1)) with x1 >= x0 ...")
    if (bmin % 8 != 0).any():
        raise ValueError("read_vdb_bricks: the bbox minimum %s must be a multiple of 8 in every axis (aligned_bbox)" % (tuple(int(v) for v in bmin),))
    tiles, leaves = _read_tree(path)[4:]
    ext = bmax - bmin + 1
    origins, bricks = [], []

    def emit(lo, blk):      # blk [x][y][z] at grid position lo (a multiple of 8)
        if (lo < 0).any() or (lo >= ext).any():
            return
        keep = np.minimum(ext - lo, 8)
        if (keep < 8).any():
            blk = blk.copy()
            blk[keep[0]:, :, :] = 0.0
            blk[:, keep[1]:, :] = 0.0
            blk[:, :, keep[2]:] = 0.0
        if blk.any():
            origins.append(lo)
            bricks.append(blk.transpose(2, 1, 0))

    for o, dim, value in tiles:
        if value == 0.0:
            continue
        lo, hi = np.maximum(o - bmin, 0), np.minimum(o - bmin + dim, ext)
        blk = np.full((8, 8, 8), value, np.float32)
        for x in range(int(lo[0]), int(hi[0]), 8):
            for y in range(int(lo[1]), int(hi[1]), 8):
                for z in range(int(lo[2]), int(hi[2]), 8):
                    emit(np.array([x, y, z]), blk)
    for o3, vm, vals in leaves:
        emit(o3 - bmin, np.where(vm, vals, 0.0).astype(np.float32).reshape(8, 8, 8))
    if not origins:
        return np.zeros((0, 3), np.int32), np.zeros((0, 8, 8, 8), np.float32)
    return np.array(origins, np.int32).reshape(-1, 3), np.ascontiguousarray(np.stack(bricks), np.float32)


def from_vdb(path, bbox=None):
    """Texture3D::FromVDB semantics: dense volume + the max==1 normalisation check (src/Texture3D.cpp:74); bbox: see read_vdb_dense."""
    vol, info = read_vdb_dense(path, bbox)
    mx = float(vol.max())
    if mx != 0.0 and mx != 1.0:
        raise RuntimeError("SkyRenderer ERROR: VDB is not normalized")
    return vol, info
