"""What the exact empty-space skip has to compute, stated in numpy and fp64 from the definitions (csrc/nrc_occupancy.hpp and the tile-mask
section of csrc/nrc_integrator.hip), not from the product's loops:

  occupancy_bits   one bit per cubic cell: the cell holds a non-zero voxel
  dilated_cells    8^3 cells that hold a voxel within Chebyshev distance 1 of a non-zero voxel
  boxes            maximal x-runs of dilated cells as world-space boxes (reproducible to the bit)
  needed_tiles     lower bound of a camera's tile mask: tiles with a pixel whose camera ray meets an occupied cell
  allowed_tiles    upper bound: tiles the boxes' projected rectangles, grown by two pixels, touch
  off_expected     must / must not / may the mask be switched off for a camera

A volume is a [nz][ny][nx] array, `size` the world extent (x, y, z) of its box, centred on the origin: voxel i of an axis with n voxels
spans [-size / 2 + size / n * i, -size / 2 + size / n * (i + 1)].  A camera is scene.make_camera's dict.  A frame is (W, H) global pixels
and, when sharded, tile = (rank, world, W, H, block) as the renderers take it: the local frame then holds the columns
parallel.rank_columns(rank, world, W, block).  Tile masks are bool arrays [tiles_y][tiles_x] of the local frame's 8x8 tiles."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RAY_MARGIN_VOXELS = 1.0e-3      # needed_tiles grows a cell by this: 100 x the ~1e-5 voxel a sample position is good to, 1/1000 of the dilation
RECT_MARGIN_PIXELS = 2.0        # allowed_tiles grows a rectangle by this: the kernel takes floor - 1 .. ceil + 1 of an fp32 value that, at w >= 1,
#                                 is far less than a pixel from the fp64 one
W_BOUND = 1.0                   # allowed_tiles holds for views whose every box corner has clip w >= this
W_OFF_NOT = 1.0e-2              # off_expected: every corner at w >= this -> the mask must be on (the kernel's threshold is 1e-3 in fp32)


def _any_per_cell(mask, c):
    """[gz][gy][gx]: does the c^3 cell hold a True voxel (the last cells of an axis may be partial)"""
    nz, ny, nx = mask.shape
    gz, gy, gx = -(-nz // c), -(-ny // c), -(-nx // c)
    padded = np.zeros((gz * c, gy * c, gx * c), bool)
    padded[:nz, :ny, :nx] = mask
    return padded.reshape(gz, c, gy, c, gx, c).any(axis=(1, 3, 5))


def occupancy_bits(vol, max_words=2048):
    """(uint32 words, cell edge): bit (cz * gy + cy) * gx + cx is set iff that cell holds a non-zero voxel.  The cell edge is the smallest
    8 * 2^k whose grid fits max_words words; the word count is padded to a multiple of four."""
    vol = np.asarray(vol)
    c = 8
    while np.prod([-(-n // c) for n in vol.shape], dtype=np.int64) > max_words * 32:
        c *= 2
    flat = _any_per_cell(vol != 0, c).reshape(-1)
    n_words = ((flat.size + 31) // 32 + 3) // 4 * 4
    bits = np.zeros(n_words * 32, np.uint64)
    bits[:flat.size] = flat
    return (bits.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32), c


def near_nonzero(vol):
    """bool [nz][ny][nx]: the voxel is within Chebyshev distance 1 of a non-zero voxel (neighbours outside the volume do not exist)"""
    near = np.asarray(vol) != 0
    for axis in range(3):
        p = np.pad(near, [(1, 1) if a == axis else (0, 0) for a in range(3)])
        n = near.shape[axis]
        near = np.take(p, range(0, n), axis) | np.take(p, range(1, n + 1), axis) | np.take(p, range(2, n + 2), axis)
    return near


def dilated_cells(vol):
    """bool [gz][gy][gx] over 8^3 cells: the cell holds a voxel within Chebyshev distance 1 of a non-zero voxel"""
    return _any_per_cell(near_nonzero(vol), 8)


def voxel_planes(n, size):
    """fp64 world coordinate of the n + 1 voxel boundaries of an axis"""
    size = float(np.float32(size))
    return -0.5 * size + (size / n) * np.arange(n + 1, dtype=np.float64)


def _x_runs(cells):
    """maximal runs of True along x in (cz, cy, cx) order: int arrays cz, cy, first cx, last cx + 1"""
    d = np.diff(np.pad(cells, ((0, 0), (0, 0), (1, 1))).astype(np.int8), axis=2)
    first, behind = np.argwhere(d == 1), np.argwhere(d == -1)      # both in (cz, cy, cx) order, so they pair up
    return first[:, 0], first[:, 1], first[:, 2], behind[:, 2]


def boxes(vol, size):
    """float32 [n][6] = {lo xyz, hi xyz}: the maximal x-runs of dilated cells in (cz, cy, cx) order; a corner is
    float32(-0.5 * size + (size / n) * voxel) evaluated in fp64, the high one clamped to the volume"""
    nz, ny, nx = np.asarray(vol).shape
    cz, cy, cx0, cx1 = _x_runs(dilated_cells(vol))
    px, py, pz = voxel_planes(nx, size[0]), voxel_planes(ny, size[1]), voxel_planes(nz, size[2])
    out = np.stack([px[8 * cx0], py[8 * cy], pz[8 * cz], px[np.minimum(8 * cx1, nx)], py[np.minimum(8 * cy + 8, ny)],
                    pz[np.minimum(8 * cz + 8, nz)]], axis=1)
    return np.ascontiguousarray(out.astype(np.float32)).reshape(-1, 6)


def covering_errors(vol, size, bx):
    """what a box list owes the skip, checked without building runs: every voxel within distance 1 of a non-zero voxel lies (with its
    centre, in fp64 world coordinates) inside exactly one box; the boxes are pairwise disjoint and inside the volume.  Returns a list of
    complaints, empty when all holds."""
    vol = np.asarray(vol)
    nz, ny, nx = vol.shape
    bx = np.asarray(bx, np.float64).reshape(-1, 6)
    planes = [voxel_planes(n, s) for n, s in ((nx, size[0]), (ny, size[1]), (nz, size[2]))]
    centres = [0.5 * (p[:-1] + p[1:]) for p in planes]
    errors = []
    count = np.zeros(vol.shape, np.uint8)
    first = [np.searchsorted(centres[a], bx[:, a], "left") for a in range(3)]
    behind = [np.searchsorted(centres[a], bx[:, 3 + a], "right") for a in range(3)]
    for i in range(bx.shape[0]):
        count[first[2][i]:behind[2][i], first[1][i]:behind[1][i], first[0][i]:behind[0][i]] += 1
    near = near_nonzero(vol)
    if (count[near] != 1).any():
        errors.append("%d voxels near a non-zero voxel are not inside exactly one box" % int((count[near] != 1).sum()))
    if not (bx[:, :3] < bx[:, 3:]).all():
        errors.append("a box is empty")
    half = 0.5 * np.asarray(size, np.float32).astype(np.float64)
    if bx.size and ((bx[:, :3] < -half).any() or (bx[:, 3:] > half).any()):
        errors.append("a box leaves the volume")
    for s in range(0, bx.shape[0], 512):      # pairwise: open boxes that overlap on every axis
        a = bx[s:s + 512, None, :]
        overlap = ((a[..., :3] < bx[None, :, 3:]) & (bx[None, :, :3] < a[..., 3:])).all(axis=2)
        overlap[np.arange(a.shape[0]), s + np.arange(a.shape[0])] = False
        if overlap.any():
            errors.append("boxes overlap (%d pairs with a box of %d..%d)" % (int(overlap.sum()), s, s + a.shape[0] - 1))
    return errors


# ---------------------------------------------------------------------------------------------------------------- frames and cameras
def local_columns(W, tile):
    """the global column of every local column"""
    from nrc_hpm_renderer_amd import parallel
    if tile is None:
        return np.arange(W, dtype=np.int64)
    rank, world, gw, _, block = tile
    assert gw == W
    return parallel.rank_columns(rank, world, W, block)


def tiles_of(lw, H):
    return (H + 7) // 8, (lw + 7) // 8


def _inverse_proj_view(cam):
    """inv_proj_view as an fp64 matrix (the dict holds it column-major in fp32)"""
    return np.asarray(cam["inv_proj_view"], np.float64).reshape(4, 4).T


def camera_rays(cam, W, H, columns):
    """(origin [3], directions [H][len(columns)][3], not normalised): the ray of pixel (gx, y) goes from cam.pos through the world point
    inv_proj_view maps (2 gx / W - 1, 2 y / H - 1, 0, 1) to"""
    m = _inverse_proj_view(cam)
    sx = 2.0 * (np.asarray(columns, np.float64) / W) - 1.0
    sy = 2.0 * (np.arange(H, dtype=np.float64) / H) - 1.0
    screen = np.stack(np.broadcast_arrays(sx[None, :], sy[:, None], 0.0, 1.0), axis=-1)
    p = screen @ m.T
    origin = np.asarray(cam["pos"], np.float64)
    return origin, p[..., :3] / p[..., 3:4] - origin


def corner_clip(bx, cam):
    """clip coordinates [n][8][4] of the boxes' corners, under the fp64 inverse of inv_proj_view"""
    bx = np.asarray(bx, np.float64).reshape(-1, 6)
    fwd = np.linalg.inv(_inverse_proj_view(cam))
    k = np.arange(8)
    corners = np.stack([bx[:, np.where(k & 1, 3, 0)], bx[:, np.where(k & 2, 4, 1)], bx[:, np.where(k & 4, 5, 2)],
                        np.ones((bx.shape[0], 8))], axis=-1)
    return corners @ fwd.T


# ---------------------------------------------------------------------------------------------------------------- the two bounds
def occupied_cell_boxes(vol, size, merge_runs=True):
    """fp64 [n][6]: the 8^3 cells that hold a non-zero voxel (not dilated), each grown by RAY_MARGIN_VOXELS and clipped to the volume.
    merge_runs: adjacent cells of an x-run as one box -- the union of the run's grown cells, which overlap, so no ray test changes."""
    vol = np.asarray(vol)
    nz, ny, nx = vol.shape
    cells = _any_per_cell(vol != 0, 8)
    if merge_runs:
        cz, cy, cx0, cx1 = _x_runs(cells)
    else:
        cz, cy, cx0 = (a for a in np.nonzero(cells))
        cx1 = cx0 + 1
    out = []
    for n, s, c0, c1 in ((nx, size[0], cx0, cx1), (ny, size[1], cy, cy + 1), (nz, size[2], cz, cz + 1)):
        planes = voxel_planes(n, s)
        margin = RAY_MARGIN_VOXELS * float(np.float32(s)) / n
        out.append((np.maximum(planes[8 * c0] - margin, planes[0]), np.minimum(planes[np.minimum(8 * c1, n)] + margin, planes[n])))
    return np.stack([out[0][0], out[1][0], out[2][0], out[0][1], out[1][1], out[2][1]], axis=1).reshape(-1, 6)


def rays_hit(origin, dirs, bx, chunk=2048):
    """bool [len(dirs)]: does the ray origin + t * dir, t > 0, meet one of the boxes (slab test)"""
    dirs = np.asarray(dirs, np.float64).reshape(-1, 3)
    hit = np.zeros(dirs.shape[0], bool)
    if bx.shape[0] == 0:
        return hit
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
            # a ray parallel to the slab is inside it for every t or for none
            inside = (lo[None, :, a] <= 0.0) & (hi[None, :, a] >= 0.0)
            near = np.where(along, np.minimum(ta, tb), np.where(inside, -np.inf, np.inf))
            far = np.where(along, np.maximum(ta, tb), np.where(inside, np.inf, -np.inf))
            t0, t1 = np.maximum(t0, near), np.minimum(t1, far)
        hit[s:s + chunk] = ((t1 > 0.0) & (t0 <= t1)).any(axis=1)
    return hit


def _tiles_with_a_pixel(pixels):
    """bool [H][lw] -> bool [tiles_y][tiles_x]"""
    return _any_per_cell(pixels[None], 8)[0]


def needed_tiles(vol, size, cam, W, H, tile=None, merge_runs=True):
    """the lower bound: a tile is needed iff the camera ray of one of its pixels meets a cell that holds a non-zero voxel"""
    cols = local_columns(W, tile)
    origin, dirs = camera_rays(cam, W, H, cols)
    hit = rays_hit(origin, dirs, occupied_cell_boxes(vol, size, merge_runs))
    return _tiles_with_a_pixel(hit.reshape(H, cols.size))


def pixel_rectangles(bx, cam, W, H, margin):
    """(gx0, gx1, gy0, gy1, w_min): per box, the pixel rectangle around its eight projected corners, grown by `margin`; pixel (gx, y)
    looks along ndc (2 gx / W - 1, 2 y / H - 1).  w_min: the smallest clip w of its corners (the rectangle means nothing unless > 0)."""
    clip = corner_clip(bx, cam)
    w = clip[..., 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        gx = (clip[..., 0] / w + 1.0) * 0.5 * W
        gy = (clip[..., 1] / w + 1.0) * 0.5 * H
    return (np.floor(gx.min(axis=1)) - margin, np.ceil(gx.max(axis=1)) + margin, np.floor(gy.min(axis=1)) - margin,
            np.ceil(gy.max(axis=1)) + margin, w.min(axis=1) if w.size else np.zeros(0))


def tiles_of_rectangles(gx0, gx1, gy0, gy1, W, H, tile=None):
    """the local tiles the global pixel rectangles touch.  Sharded: every local column of every strip of `block` columns a rectangle
    touches counts as touched."""
    cols = local_columns(W, tile)
    block = 1 if tile is None else tile[4]
    strip = cols // block
    rows = np.arange(H)
    out = np.zeros(tiles_of(cols.size, H), bool)
    for x0, x1, y0, y1 in zip(gx0, gx1, gy0, gy1):
        if not (x0 <= x1 and y0 <= y1):
            continue
        c = (strip >= np.floor(x0 / block)) & (strip <= np.floor(x1 / block))
        r = (rows >= y0) & (rows <= y1)
        out |= _tiles_with_a_pixel(r[:, None] & c[None, :])
    return out


def allowed_tiles(bx, cam, W, H, tile=None):
    """the upper bound: the tiles touched by the boxes' rectangles grown by RECT_MARGIN_PIXELS; None for a view with a corner at clip
    w < W_BOUND (there the bound does not apply)"""
    gx0, gx1, gy0, gy1, w_min = pixel_rectangles(bx, cam, W, H, RECT_MARGIN_PIXELS)
    if w_min.size and w_min.min() < W_BOUND:
        return None
    return tiles_of_rectangles(gx0, gx1, gy0, gy1, W, H, tile)


def off_expected(bx, cam):
    """True: a corner has w <= 0, the mask must be off.  False: every corner has w >= W_OFF_NOT, it must be on.  None: either."""
    w = corner_clip(bx, cam)[..., 3]
    if w.size and w.min() <= 0.0:
        return True
    if w.size == 0 or w.min() >= W_OFF_NOT:
        return False
    return None


# ---------------------------------------------------------------------------------------------------------------- reading a TileMask()
def unpack_mask(words, lw, H):
    """TileMask() words -> (bool [tiles_y][tiles_x], bits behind the last tile, off word)"""
    ty, tx = tiles_of(lw, H)
    words = np.asarray(words, np.uint32)
    assert words.size == (ty * tx + 31) // 32 + 1, (words.size, ty, tx)
    bits = ((words[:-1, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(-1)
    return bits[:ty * tx].reshape(ty, tx), bits[ty * tx:], int(words[-1])
