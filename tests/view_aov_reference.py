"""What the view-AOV tests share (test_view_aov_cpu.py, test_gpu_view_aov.py): the fixtures, an fp64 reference of {tau, z_front, z_half}
per camera ray, and the stable-pixel rule.

The reference (aov_reference.reference_segment over the whole ray) knows nothing of a voxel walk: per ray, the parameters of ALL voxel
planes the ray meets inside the box are sorted, and the voxel of every segment between two neighbours is looked up at the segment's
midpoint.  The ray itself is the renderer's fp32 inv_proj_view and position, evaluated in fp64.

Stable pixels.  The fp32 code and the fp64 reference do not follow the same ray to the last bit, and where a ray grazes a voxel's edge the
AOV jumps.  The reference is therefore evaluated on five rays per pixel -- the centre ray d and d + 2e-6 * {+a, -a, +b, -b}, renormalised,
with a = normalize(d x (0, 1, 0)) and b = d x a -- and a pixel is UNSTABLE when, among the five, the finiteness of z_front or of z_half
differs, either z differs from the centre's by more than 1e-3, or tau differs by more than 1e-3 * (1 + tau).  Unstable pixels are left
out of accuracy comparisons; at most 5 % of the pixels that hit the medium (tau > 0 on any of the five rays) may be, which the tests
assert from the reference alone."""
import functools
import math
import os

import numpy as np

import aov_reference as A

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LN2 = math.log(2.0)
W, H = 48, 32
PERTURB = 2e-6
UNSTABLE_CAP = 0.05


# ---------------------------------------------------------------------------------------------------------------- fixtures
@functools.lru_cache(maxsize=None)
def blocks_volume():
    """[nz][ny][nx] = [28][12][20]: no dim is a multiple of 8"""
    rng = np.random.default_rng(7)
    blk = np.zeros((28, 12, 20), np.uint8)
    for _ in range(14):
        c = rng.integers(0, [20, 12, 28])
        r = rng.integers(1, 4)
        x0, y0, z0 = np.maximum(c - r, 0)
        x1, y1, z1 = c + r
        blk[z0:z1, y0:y1, x0:x1] = rng.integers(1, 256)
    blk.setflags(write=False)
    return blk


@functools.lru_cache(maxsize=None)
def cloud_volume():
    v = np.load(os.path.join(GOLDEN, "cloud_sixteenth_u8.npz"))["density"]
    v.setflags(write=False)
    return v


def orbit_view(sc, k, aspect=W / H):
    return sc.orbit_cameras(8, radius=70.0, height=20.0, aspect=aspect)[k]


def inside_view(sc, vol, size, aspect=W / H):
    """a camera inside the box, at the centre of the empty voxel nearest the box's centre, looking off every axis"""
    nz, ny, nx = vol.shape
    zz, yy, xx = np.nonzero(vol == 0)
    d2 = (xx - nx / 2) ** 2 + (yy - ny / 2) ** 2 + (zz - nz / 2) ** 2
    i = int(np.argmin(d2))
    n = np.array([nx, ny, nz], np.float64)
    pos = -0.5 * size.astype(np.float64) + (np.array([xx[i], yy[i], zz[i]], np.float64) + 0.5) * size / n
    return sc.make_camera(pos=pos, view_dir=(0.3, 0.2, 1.0), aspect=aspect)


def cases(sc):
    """{name: (scene, camera)} of the accuracy comparisons, and of the bitwise ones with the default view added"""
    blk = sc.make_scene(blocks_volume(), scene_id=4)
    cld = sc.make_scene(cloud_volume(), scene_id=4)
    return {
        "blocks_v3": (blk, orbit_view(sc, 3)),
        "blocks_v1": (blk, orbit_view(sc, 1)),
        "cloud_v3": (cld, orbit_view(sc, 3)),
        "blocks_inside": (blk, inside_view(sc, blocks_volume(), blk["size"])),
    }


def default_view(sc, aspect=W / H):
    """make_camera's default view: its centre row and column run inside voxel faces (bitwise and range checks only)"""
    return sc.make_camera(aspect=aspect)


# ---------------------------------------------------------------------------------------------------------------- rays
def ray_directions(cam, w, h, columns=None, global_w=None):
    """fp64 directions [h][w][3] of the pixels' camera rays (u = global column / global width, v = row / height: no half-pixel offset)"""
    m = np.asarray(cam["inv_proj_view"], np.float32).astype(np.float64).reshape(4, 4).T      # column-major -> [row][col]
    pos = np.asarray(cam["pos"], np.float32).astype(np.float64)
    cols = np.arange(w, dtype=np.float64) if columns is None else np.asarray(columns, np.float64)
    u = cols / float(global_w if global_w is not None else w)
    v = np.arange(h, dtype=np.float64) / h
    sx, sy = np.meshgrid(2.0 * u - 1.0, 2.0 * v - 1.0)
    clip = np.stack([sx, sy, np.zeros_like(sx), np.ones_like(sx)], axis=-1)
    wp = clip @ m.T
    p = wp[..., :3] / wp[..., 3:4]
    d = p - pos
    return d / np.linalg.norm(d, axis=-1, keepdims=True), pos


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def ray_directions_f32(cam, w, h):
    """the directions as the fp32 code forms them (csrc/nrc_view_aov.hpp: view_aov_camera_ray, the compensated evaluation), operation for
    operation in numpy float32; a fused multiply-add is an exact fp64 product + one fp64 sum rounded to fp32 (exact where the code relies
    on exactness -- the error of a product fits fp32 --, otherwise a double rounding within half an fp32 ulp of the single one)"""
    m = np.asarray(cam["inv_proj_view"], np.float32)
    pos = np.asarray(cam["pos"], np.float32)
    f32 = np.float32

    def fma(a, b, c):
        return _f32(np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64))

    def diff(a, p, q):      # a - p q as (hi, lo)
        ph = f32(p * q)
        pl = f32(fma(p, q, -ph))
        s_ = f32(a - ph)
        bb = f32(s_ - a)
        e = f32(f32(a - f32(s_ - bb)) + f32(-ph - bb))
        return s_, f32(e - pl)
    u = (np.arange(w, dtype=np.float32) * f32(f32(1.0) / f32(w))).astype(np.float32)
    v = (np.arange(h, dtype=np.float32) * f32(f32(1.0) / f32(h))).astype(np.float32)
    sx, sy = np.meshgrid(fma(u, 2.0, -1.0), fma(v, 2.0, -1.0))
    ww = fma(m[7], sy, fma(m[3], sx, m[15]))
    d = []
    for k in range(3):
        A, B, C = diff(m[k], pos[k], m[3]), diff(m[4 + k], pos[k], m[7]), diff(m[12 + k], pos[k], m[15])
        hi, lo = fma(sx, A[0], fma(sy, B[0], C[0])), fma(sx, A[1], fma(sy, B[1], C[1]))
        d.append(((hi + lo).astype(np.float32) / ww).astype(np.float32))
    ll = fma(d[2], d[2], fma(d[1], d[1], (d[0] * d[0]).astype(np.float32)))
    inv = (f32(1.0) / np.sqrt(ll).astype(np.float32)).astype(np.float32)
    return np.stack([(d[k] * inv).astype(np.float32) for k in range(3)], axis=-1)


def perturbed(d):
    """the five rays of a pixel: [5][3], the centre first"""
    a = np.cross(d, (0.0, 1.0, 0.0))
    a /= np.linalg.norm(a)
    b = np.cross(d, a)
    out = [d] + [d + PERTURB * s * e for e in (a, b) for s in (1.0, -1.0)]
    return np.array([x / np.linalg.norm(x) for x in out])


# ---------------------------------------------------------------------------------------------------------------- the fp64 reference
def reference_ray(vol, size, density_factor, ro, rd):
    """(tau, z_front, z_half, crossings, sigma of the voxel where tau reaches ln 2, t1) of one whole ray in fp64; misses: (0, inf, inf, 0, 0, 0)"""
    tau, z_front, z, crossings, s_cross, t1, _ = A.reference_segment(vol, size, density_factor, ro, rd, 0.0, math.inf, (LN2,))
    return tau, z_front, float(z[0]), crossings, float(s_cross[0]), t1


def reference_view(scene, cam, w=W, h=H):
    """the reference of every pixel on its five rays: dict of arrays [h][w][5] (tau, z_front, z_half), [h][w] (crossings, sigma_cross, t1
    of the centre ray) and the derived masks `hit`, `stable` and spreads S_tau, S_zf, S_zh"""
    dirs, pos = ray_directions(cam, w, h)
    records = np.concatenate([np.broadcast_to(pos, (h, w, 3)), np.zeros((h, w, 1)), dirs, np.full((h, w, 1), math.inf)], axis=-1)
    ref = A.reference_records(scene, records.reshape(-1, 8), perturbed, (LN2,))
    # crossings: a whole ray's N is the number of voxel planes it meets (aov_reference.segments_summed: where a ray segment's differs)
    return summarize(dict(tau=ref["tau"].reshape(h, w, 5), z_front=ref["z_front"].reshape(h, w, 5), z_half=ref["z"][0].reshape(h, w, 5),
                          crossings=ref["planes"].reshape(h, w), sigma_cross=ref["sigma_cross"][0].reshape(h, w), t1=ref["t1"].reshape(h, w),
                          dirs=dirs))


def _spread(z):
    """max |z_k - z_0| over the five rays where all are finite, else 0"""
    fin = np.isfinite(z).all(axis=-1)
    out = np.zeros(z.shape[:-1])
    out[fin] = np.abs(z[fin] - z[fin][:, :1]).max(axis=-1)
    return out


def summarize(ref):
    tau, zf, zh = ref["tau"], ref["z_front"], ref["z_half"]
    hit = (tau > 0.0).any(axis=-1)
    unstable = np.zeros(hit.shape, bool)
    for z in (zf, zh):
        fin = np.isfinite(z)
        unstable |= fin.any(axis=-1) != fin.all(axis=-1)
    ref["S_tau"] = np.abs(tau - tau[..., :1]).max(axis=-1)
    ref["S_zf"], ref["S_zh"] = _spread(zf), _spread(zh)
    unstable |= (ref["S_zf"] > 1e-3) | (ref["S_zh"] > 1e-3) | (ref["S_tau"] > 1e-3 * (1.0 + tau[..., 0]))
    ref["hit"], ref["stable"] = hit, ~unstable
    return ref


def unstable_share(ref):
    """(unstable pixels, hit pixels) -- every unstable pixel is a hit pixel"""
    return int((~ref["stable"]).sum()), int(ref["hit"].sum())


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def tolerances(ref, sigma_max):
    """the per-pixel bounds of the fp32 code against the centre ray's reference (test_view_aov_cpu.py states where they come from)"""
    tau, zf, zh = ref["tau"][..., 0], ref["z_front"][..., 0], ref["z_half"][..., 0]
    N = ref["crossings"].astype(np.float64)
    tol_tau = ref["S_tau"] + 8.0 * N * sigma_max * ulp32(ref["t1"]) + N * ulp32(tau)
    with np.errstate(invalid="ignore", divide="ignore"):
        tol_zf = ref["S_zf"] + 8.0 * ulp32(np.where(np.isfinite(zf), zf, 0.0))
        tol_zh = ref["S_zh"] + np.where(ref["sigma_cross"] > 0.0, tol_tau / ref["sigma_cross"], 0.0) + 8.0 * ulp32(np.where(np.isfinite(zh), zh, 0.0))
    tol_alpha = tol_tau + 4.0 * ulp32(1.0)
    return dict(tau=tol_tau, z_front=tol_zf, z_half=tol_zh, alpha=tol_alpha)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def chi2_against_alpha(a_mc, alpha, frames):
    """(chi2, n, bound) over the pixels with alpha in (0.05, 0.95): sum (a_mc - alpha)^2 / (alpha (1 - alpha) / frames) <= n + 6 sqrt(2 n)"""
    a_mc, alpha = np.asarray(a_mc, np.float64), np.asarray(alpha, np.float64)
    m = (alpha > 0.05) & (alpha < 0.95)
    chi2 = float((((a_mc[m] - alpha[m]) ** 2) / (alpha[m] * (1.0 - alpha[m]) / frames)).sum())
    n = int(m.sum())
    return chi2, n, n + 6.0 * math.sqrt(2.0 * n)
