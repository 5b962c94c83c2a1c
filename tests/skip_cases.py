"""The volumes, views and frames on which the empty-space skip is compared with tests/skip_reference.py, shared by
test_skip_reference_cpu.py (the reference bites: broken mask rules are rejected on these cases) and test_gpu_empty_skip_geometry.py
(the kernels lie between the bounds on the same cases).  The reference of a case is computed once per session (reference_of)."""
import functools
import math
import os

import numpy as np

import skip_reference as ref
from nrc_hpm_renderer_amd import parallel, scene as sc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------------------------------------------------------------------------------------------------------- volumes
# (b) lone voxels, (x, y, z) in a 44 x 60 x 196 volume (last cells of x, y, z: 40..43, 56..59, 192..195).  Seen from +x (LONE_VIEW) the screen
# shows z across and y up, and the groups lie at least two tiles apart.
LONE_DIMS = (44, 60, 196)      # nx, ny, nz
LONE_VOXELS = {
    "first-voxel": [(0, 0, 0)],
    "far-corner": [(43, 59, 195)],
    "x-mod-8-is-7": [(7, 28, 40)],            # dilates into cell cx = 1: a run of two cells
    "x-mod-8-is-0": [(16, 28, 72)],           # dilates into cell cx = 1
    "last-cell-of-x": [(42, 12, 100)],
    "last-cell-of-y": [(20, 58, 130)],
    "last-cell-of-z": [(20, 30, 194)],
    "y-7-and-z-0": [(20, 15, 24)],            # dilates into cy + 1 and cz - 1: four boxes
    "interior": [(21, 44, 60)],
    "full-width-x-run": [(x, 44, 160) for x in range(44)],
    "bottom-far": [(30, 2, 168)],
}


def lone_volume(without=None):
    nx, ny, nz = LONE_DIMS
    v = np.zeros((nz, ny, nx), np.uint8)
    for k, (name, voxels) in enumerate(LONE_VOXELS.items()):
        if name == without:
            continue
        for x, y, z in voxels:
            v[z, y, x] = 1 + 23 * k
    return v


# (c) many boxes: one voxel in the middle of every second cell (cx even) of slabs cz = 5 .. 21 of a 128 x 128 x 216 volume: 17 x 16 x 8 = 2176
# boxes, more than two chunks of the tile-parallel build's 1024.  The first box (slab 0) and the last box (slab 26) stand alone, four empty
# slabs away from the rest, so that from the side (MANY_VIEW) they project onto tiles of their own.
MANY_DIMS = (128, 128, 216)
MANY_FIRST, MANY_LAST = (68, 60, 4), (60, 68, 212)
MANY_SLABS = range(5, 22)


def many_volume(without=None):
    nx, ny, nz = MANY_DIMS
    v = np.zeros((nz, ny, nx), np.uint8)
    for cz in MANY_SLABS:
        v[8 * cz + 4, 4::8, 4::16] = 100 + cz
    for name, (x, y, z) in (("first", MANY_FIRST), ("last", MANY_LAST)):
        if name != without:
            v[z, y, x] = 255
    return v


@functools.lru_cache(maxsize=None)
def volume(name):
    """[nz][ny][nx] uint8, read-only"""
    if name == "cloud16":
        v = np.load(os.path.join(GOLDEN, "cloud_sixteenth_u8.npz"))["density"]
    elif name == "lone":
        v = lone_volume()
    elif name == "many":
        v = many_volume()
    elif name == "sparse512":
        from volume_common import _sparse_512
        v = _sparse_512()
    else:
        raise KeyError(name)
    v = np.ascontiguousarray(v, np.uint8)
    v.setflags(write=False)
    return v


def size_of(vol):
    nz, ny, nx = vol.shape
    return sc.volume_size((nx, ny, nz))


@functools.lru_cache(maxsize=None)
def boxes_of(name):
    v = volume(name)
    b = ref.boxes(v, size_of(v))
    b.setflags(write=False)
    return b


# ---------------------------------------------------------------------------------------------------------------- frames
FRAMES = {      # name: (W, H, None or (rank, block) of a sharding over three ranks)
    "128x80": (128, 80, None),
    "ragged100x52": (100, 52, None),
    "tiny8x6": (8, 6, None),
    "wide328x88": (328, 88, None),            # 41 tiles across: a mask word lies inside one tile row
    "96x56": (96, 56, None),
    "sharded-128x80-block8": (128, 80, (1, 8)),
    "sharded-128x80-block16": (128, 80, (1, 16)),
    "sharded-128x80-rank0": (128, 80, (0, 8)),
    "sharded-128x80-rank2": (128, 80, (2, 8)),
    "sharded-ragged100x52-rank0": (100, 52, (0, 8)),      # rank 0 holds the frame's last strip, four columns wide
}


def frame(name):
    """(W, H, tile, local width)"""
    W, H, shard = FRAMES[name]
    if shard is None:
        return W, H, None, W
    rank, block = shard
    return W, H, (rank, 3, W, H, block), parallel.local_width(rank, 3, W, block)


# ---------------------------------------------------------------------------------------------------------------- views
def view(name, vol_name, aspect):
    """the views are placed relative to the volume's box, whose extent differs between the volumes"""
    sx, sy, sz = (float(s) for s in size_of(volume(vol_name)))
    origin = np.zeros(3)

    def at(pos, fovy=60.0):
        pos = np.asarray(pos, np.float64)
        return sc.make_camera(pos=pos, view_dir=origin - pos, aspect=aspect, fovy=math.radians(fovy))

    if name == "default":
        return sc.make_camera(aspect=aspect)
    if name == "oblique":
        return at((50.0, 30.0, 45.0))
    if name == "grazing":         # just above the top face, outside the box in x too, looking almost along the face
        return sc.make_camera(pos=(0.9 * sx, 0.5 * sy + 2.0, 0.0), view_dir=(-1.0, -0.05, 0.1), aspect=aspect)
    if name == "wide":
        return at((0.5 * sx + 14.0, 5.0, 10.0), fovy=110.0)
    if name == "narrow":
        return sc.make_camera(view_dir=(-1.0, 0.05, 0.1), aspect=aspect, fovy=math.radians(15.0))
    if name == "orbit":
        return sc.orbit_cameras(5, radius=70.0, height=25.0, aspect=aspect)[1]
    if name == "inside":          # the medium lies on both sides of the eye plane: off
        return sc.make_camera(pos=(0.16 * sx, 0.0, 0.0), aspect=aspect)
    if name == "near-face":       # outside the box, 1.3 in front of its +z face, looking along the face: few rays meet the medium, yet half
        return sc.make_camera(pos=(0.0, 0.0, 0.5 * sz + 1.3), aspect=aspect)      # of it is behind the eye plane: off
    if name == "past":            # far away, looking past the box: every box in front of the eye plane and off screen: all clear
        return sc.make_camera(pos=(200.0, 0.0, 0.0), view_dir=(-1.0, 0.0, 2.5), aspect=aspect)
    if name == "lone-side":       # (b)'s own view: from +x, the volume's y and z extent fills the frame
        return sc.make_camera(pos=(64.0, 0.0, 0.0), aspect=aspect, fovy=math.radians(34.0))
    if name == "many-side":       # (c)'s own view: from +x, far enough for the slabs to keep apart on the screen
        return sc.make_camera(pos=(150.0, 0.0, 0.0), aspect=aspect, fovy=math.radians(33.0), far=400.0)
    raise KeyError(name)


ALL_VIEWS = ["default", "oblique", "grazing", "wide", "narrow", "orbit", "inside", "near-face", "past"]
MUST_BE_OFF = ["inside", "near-face"]
MUST_BE_CLEAR = ["past"]

# (volume, frame, views).  cloud16's ray test costs seconds per view at 128x80, so every view meets it once, at 128x80, and the other frames
# take the views that differ in kind (partly covered, off, clear); the sparse volumes are cheap and take every view at the big frames.
CASES = [
    ("cloud16", "128x80", ALL_VIEWS),
    ("cloud16", "ragged100x52", ["default", "orbit", "inside", "past"]),
    ("cloud16", "tiny8x6", ["default", "narrow", "inside", "past"]),
    ("cloud16", "sharded-128x80-block8", ["default", "oblique", "near-face", "past"]),
    ("cloud16", "sharded-128x80-block16", ["default", "orbit", "inside", "past"]),
    ("lone", "wide328x88", ["lone-side"] + ALL_VIEWS),
    ("lone", "128x80", ["lone-side", "oblique", "grazing", "wide"]),
    ("lone", "ragged100x52", ["lone-side", "orbit"]),
    ("lone", "sharded-128x80-block8", ["lone-side", "oblique", "inside"]),
    ("lone", "sharded-128x80-block16", ["lone-side", "orbit"]),
    ("cloud16", "sharded-128x80-rank0", ["default", "orbit", "past"]),
    ("lone", "sharded-128x80-rank2", ["lone-side", "oblique"]),
    ("lone", "sharded-ragged100x52-rank0", ["lone-side", "grazing"]),
    ("many", "96x56", ["many-side", "oblique", "inside", "past"]),
    ("many", "tiny8x6", ["many-side", "past"]),
]
CASE_IDS = ["%s-%s" % (v, f) for v, f, _ in CASES]
LONE_VIEW = ("lone", "wide328x88", "lone-side")
MANY_VIEW = ("many", "96x56", "many-side")


class Reference:
    """needed / allowed: bool [tiles_y][tiles_x] (allowed None where the upper bound does not apply), off: True / False / None"""

    def __init__(self, vol_name, frame_name, view_name, vol=None):
        W, H, tile, lw = frame(frame_name)
        self.cam = view(view_name, vol_name, W / H)
        self.W, self.H, self.tile, self.lw = W, H, tile, lw
        v = volume(vol_name) if vol is None else vol
        bx = boxes_of(vol_name) if vol is None else ref.boxes(v, size_of(v))
        self.boxes = bx
        self.off = ref.off_expected(bx, self.cam)
        self.needed = ref.needed_tiles(v, size_of(v), self.cam, W, H, tile)
        self.allowed = ref.allowed_tiles(bx, self.cam, W, H, tile)


@functools.lru_cache(maxsize=None)
def reference_of(vol_name, frame_name, view_name):
    return Reference(vol_name, frame_name, view_name)
