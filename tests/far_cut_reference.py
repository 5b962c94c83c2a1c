"""What the far cut of the camera walk ("Far cut") has to guarantee, stated in numpy and fp64 from the definitions,
not from the kernels' loops:

  last_density_distance   per pixel: the distance from the camera position at which the pixel's camera ray leaves its last non-empty
                          voxel (an exact ray march over the non-empty voxels, as slab tests against their maximal x-runs) -- behind it
                          the ray reads density 0 for good; -inf for a ray that meets no density
  tile_far                per 8x8 tile: the bound the mask build owes the kernels -- over every occupancy box (skip_reference.boxes) whose
                          pixel rectangle touches the tile, the distance from the camera position to the box's farthest corner, grown by
                          2^-16 of itself and a voxel diagonal; 0 for a tile no box touches

The cut is sound when a tile's bound >= last_density_distance for every pixel of the tile.  (The kernels bound a box piece by piece,
cell-long pieces with their own rectangles: a tighter bound than this one, held to the same comparison.)  tile_far's `corner` and `margin` arguments state
deliberately wrong rules (tests/test_far_cut_reference_cpu.py shows that the comparison catches them).  Volumes, cameras and frames as in
tests/skip_reference.py."""
import numpy as np

import skip_reference as ref

RECT_MARGIN_PIXELS = 1.0        # the rule's own: the mask build takes floor - 1 .. ceil + 1 of a box's projected corners
RELATIVE_MARGIN = 2.0 ** -16    # of the distance itself: some hundred fp32 roundings


def voxel_diagonal(vol, size):
    nz, ny, nx = np.asarray(vol).shape
    return float(np.sqrt(sum((float(np.float32(s)) / n) ** 2 for s, n in zip(size, (nx, ny, nz)))))


def voxel_runs(vol, size):
    """fp64 [n][6] = {lo xyz, hi xyz}: the maximal x-runs of NON-EMPTY voxels, with their exact bounds (the union of a run's voxels is a
    box, so a ray leaves the run where it leaves the run's last voxel)"""
    vol = np.asarray(vol)
    nz, ny, nx = vol.shape
    z, y, x0, x1 = ref._x_runs(vol != 0)
    px, py, pz = ref.voxel_planes(nx, size[0]), ref.voxel_planes(ny, size[1]), ref.voxel_planes(nz, size[2])
    return np.stack([px[x0], py[y], pz[z], px[x1], py[y + 1], pz[z + 1]], axis=1).reshape(-1, 6)


def exit_distances(origin, dirs, bx, chunk=128):
    """fp64 [len(dirs)]: the largest t at which the ray origin + t * dir / |dir|, t > 0, is inside one of the boxes; -inf: in none"""
    dirs = np.asarray(dirs, np.float64).reshape(-1, 3)
    dirs = dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
    out = np.full(dirs.shape[0], -np.inf)
    if bx.shape[0] == 0:
        return out
    lo, hi = bx[:, :3] - origin, bx[:, 3:] - origin
    for s in range(0, dirs.shape[0], chunk):
        d = dirs[s:s + chunk]
        t0 = np.full((d.shape[0], bx.shape[0]), -np.inf)
        t1 = np.full((d.shape[0], bx.shape[0]), np.inf)
        for a in range(3):
            da = d[:, a:a + 1]
            along = da != 0.0
            with np.errstate(divide="ignore", invalid="ignore"):
                ta, tb = lo[None, :, a] / da, hi[None, :, a] / da
            near, far = np.minimum(ta, tb), np.maximum(ta, tb)
            if not along.all():      # a ray parallel to the slab is inside it for every t or for none
                inside = (lo[None, :, a] <= 0.0) & (hi[None, :, a] >= 0.0)
                near = np.where(along, near, np.where(inside, -np.inf, np.inf))
                far = np.where(along, far, np.where(inside, np.inf, -np.inf))
            np.maximum(t0, near, out=t0)
            np.minimum(t1, far, out=t1)
        hit = (t1 > 0.0) & (t0 <= t1)
        out[s:s + chunk] = np.where(hit, t1, -np.inf).max(axis=1)
    return out


def last_density_distance(vol, size, cam, W, H, tile=None):
    """fp64 [H][local width]"""
    cols = ref.local_columns(W, tile)
    origin, dirs = ref.camera_rays(cam, W, H, cols)
    return exit_distances(origin, dirs, voxel_runs(vol, size)).reshape(H, cols.size)


def corner_distances(bx, cam):
    """fp64 [n][8]: from the camera position to the boxes' corners"""
    bx = np.asarray(bx, np.float64).reshape(-1, 6)
    k = np.arange(8)
    corners = np.stack([bx[:, np.where(k & 1, 3, 0)], bx[:, np.where(k & 2, 4, 1)], bx[:, np.where(k & 4, 5, 2)]], axis=-1)
    return np.linalg.norm(corners - np.asarray(cam["pos"], np.float64), axis=-1)


def tile_far(bx, cam, W, H, voxel_diag, tile=None, corner="farthest", margin=True):
    """fp64 [tiles_y][tiles_x].  corner = "nearest", margin = False: the wrong rules."""
    d = corner_distances(bx, cam)
    d = d.max(axis=1) if corner == "farthest" else d.min(axis=1)
    if margin:
        d = d * (1.0 + RELATIVE_MARGIN) + voxel_diag
    gx0, gx1, gy0, gy1, _ = ref.pixel_rectangles(bx, cam, W, H, RECT_MARGIN_PIXELS)
    cols = ref.local_columns(W, tile)
    out = np.zeros(ref.tiles_of(cols.size, H))
    for i in range(d.size):
        touched = ref.tiles_of_rectangles(gx0[i:i + 1], gx1[i:i + 1], gy0[i:i + 1], gy1[i:i + 1], W, H, tile)
        out[touched] = np.maximum(out[touched], d[i])
    return out


def per_pixel(tiles, lw, H):
    """[tiles_y][tiles_x] -> [H][lw]: every pixel its tile's value"""
    return np.repeat(np.repeat(tiles, 8, axis=0), 8, axis=1)[:H, :lw]


def violations(far_tiles, last, lw, H):
    """pixels whose ray still meets density behind their tile's bound: (y, x) list"""
    return np.argwhere(last > per_pixel(np.asarray(far_tiles, np.float64), lw, H)).tolist()
