"""The media, views and frames of the far cut's tests (tests/test_far_cut_reference_cpu.py, tests/test_gpu_far_cut.py): 32^3 volumes in the
default box -- except the reference's sixteenth cloud --, seen head-on from +x (the default camera) and grazing along the top face."""
import functools
import os

import numpy as np

import far_cut_reference as far
from nrc_hpm_renderer_amd import parallel, scene as sc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FRAME_RANDOM = [0.25, 0.5, 0.75, 1.0]
N = 32
MEDIA = ("sphere", "blobs", "slab", "corner", "cloud16")
VIEWS = ("head-on", "grazing")
FRAMES = {"64x64": (64, 64, None), "72x40": (72, 40, None), "two-strips": (64, 64, (1, 2, 8))}      # (W, H, (rank, world, block))
# blobs, [z][y][x]: seen from +x the near blob stands in front of the far one, 17 empty voxels between them
NEAR_BLOB, FAR_BLOB = (slice(14, 18), slice(14, 18), slice(24, 28)), (slice(13, 19), slice(13, 19), slice(3, 7))


@functools.lru_cache(maxsize=None)
def volume(name):
    """[nz][ny][nx] uint8, read-only"""
    if name == "cloud16":
        v = np.load(os.path.join(GOLDEN, "cloud_sixteenth_u8.npz"))["density"]
    elif name == "sphere":                # centred, radius 6.5 voxels: its dilated cells are the middle 16^3, a quarter of the box behind them
        g = np.arange(N, dtype=np.float64) + 0.5 - N / 2
        r = np.sqrt(g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2)
        v = np.where(r < 6.5, 255.0 * (1.0 - r / 8.0), 0.0).astype(np.uint8)
    else:
        v = np.zeros((N, N, N), np.uint8)
        if name == "blobs":
            v[NEAR_BLOB] = 200
            v[FAR_BLOB] = 120
        elif name == "slab":              # touches the box's far face (x = 0 is the face away from the head-on camera)
            v[:, :, 0:4] = 150
        elif name == "corner":
            v[0, 0, 0] = 255
        else:
            raise KeyError(name)
    v = np.ascontiguousarray(v, np.uint8)
    v.setflags(write=False)
    return v


def size_of(vol):
    nz, ny, nx = vol.shape
    return sc.volume_size((nx, ny, nz))


def view(name, vol, aspect):
    sx, sy, _ = (float(s) for s in size_of(vol))
    if name == "head-on":
        return sc.make_camera(aspect=aspect)
    assert name == "grazing"      # just above the top face, outside the box in x too, looking almost along the face
    return sc.make_camera(pos=(0.9 * sx, 0.5 * sy + 2.0, 0.0), view_dir=(-1.0, -0.05, 0.1), aspect=aspect)


def frame(name):
    """(W, H, tile, local width)"""
    W, H, shard = FRAMES[name]
    if shard is None:
        return W, H, None, W
    rank, world, block = shard
    return W, H, (rank, world, W, H, block), parallel.local_width(rank, world, W, block)


def make_scene(vol):
    return sc.make_scene(vol, scene_id=4, env=sc.procedural_sky(32, 16))


@functools.lru_cache(maxsize=None)
def last_density(medium, view_name, frame_name):
    """far_cut_reference.last_density_distance of a case, computed once per session; read-only"""
    vol = volume(medium)
    W, H, tile, _ = frame(frame_name)
    last = far.last_density_distance(vol, size_of(vol), view(view_name, vol, W / H), W, H, tile)
    last.setflags(write=False)
    return last
