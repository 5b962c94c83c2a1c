"""What the denoise tests share (test_denoise_cpu.py, test_gpu_denoise.py): the numpy fp64 statement of the filter (include/nrc_hpm.h,
"Denoise"), the error bound of the fp32 code against it, and the cases.

The fp64 statement follows the contract's rule with real arithmetic in place of fp32's: the same taps in the same roles, the weight
k exp(-d), the normalised sum formed around the centre pixel.  What the contract fixes in fp32 is taken over as it stands: the pass
constants inv_sa, inv_sz, inv_sc (1.0f / sigma; the colour sigma of pass p by p fp32 multiplications) and the luminance coefficients
(.299f, .587f, .114f) are the fp32 numbers, widened."""
import functools
import math

import numpy as np

import view_aov_reference as V

H_TAPS = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
DEFAULTS = dict(passes=3, sigma_alpha=0.1, sigma_depth=4.0, sigma_color=math.inf, color_decay=0.5)
LUM = tuple(float(np.float32(x)) for x in (0.299, 0.587, 0.114))
U = 2.0 ** -24      # fp32's unit roundoff


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def pass_constants(p, k):
    """(stride, inv_sa, inv_sz, inv_sc) of pass k, the inverses as the fp32 numbers the contract defines"""
    f32 = np.float32
    sc = f32(p["sigma_color"])
    for _ in range(k):
        sc = f32(sc * f32(p["color_decay"]))
    with np.errstate(divide="ignore"):
        return 1 << k, float(f32(1.0) / f32(p["sigma_alpha"])), float(f32(1.0) / f32(p["sigma_depth"])), float(f32(1.0) / sc)


def _lum(c):
    return LUM[0] * c[..., 0] + LUM[1] * c[..., 1] + LUM[2] * c[..., 2]


def pass_fp64(c, guide, stride, inv_sa, inv_sz, inv_sc, terms=("alpha", "depth", "color")):
    """One pass in fp64.  c [h][w][4] (any float dtype), guide [h][w][4] = {alpha, tau, z_front, z_half}.  Returns (out [h][w][4] fp64,
    aux) with aux = dict(filtered [h][w] bool, D [h][w] the sum of the weights, C [h][w] the largest |component| among the kept taps,
    L [h][w] the largest |lum| among them).  terms: the terms of d that are formed at all (the sigma = +inf test leaves one out)."""
    c = np.asarray(c, np.float64)
    g = np.asarray(guide, np.float64)
    h, w = c.shape[:2]
    alpha, z = g[..., 0], g[..., 2]
    finite = np.isfinite(c[..., :3]).all(axis=-1)
    usable = (alpha != 0.0) & finite
    lum = np.where(usable, _lum(np.where(usable[..., None], c, 0.0)), 0.0)
    zz = np.where(usable, z, 0.0)
    cc = np.where(usable[..., None], c[..., :3], 0.0)
    acc = np.zeros((h, w, 3))
    D = np.zeros((h, w))
    Cmax = np.zeros((h, w))
    Lmax = np.zeros((h, w))
    ys, xs = np.mgrid[0:h, 0:w]
    for j in range(-2, 3):
        for i in range(-2, 3):
            qy, qx = ys + j * stride, xs + i * stride
            inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
            qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
            keep = inside & usable[qy, qx] & usable
            d = np.zeros((h, w))
            if "alpha" in terms:
                d = d + np.abs(alpha[qy, qx] - alpha) * inv_sa
            if "depth" in terms:
                d = d + np.abs(zz[qy, qx] - zz) * inv_sz
            if "color" in terms:
                d = d + np.abs(lum[qy, qx] - lum) * inv_sc
            wgt = np.where(keep, H_TAPS[i + 2] * H_TAPS[j + 2] * np.exp(-d), 0.0)
            acc += wgt[..., None] * (cc[qy, qx] - cc)      # (around the centre, as the contract forms the mean)
            D += wgt
            Cmax = np.maximum(Cmax, np.where(keep, np.abs(cc[qy, qx]).max(axis=-1), 0.0))
            Lmax = np.maximum(Lmax, np.where(keep, np.abs(lum[qy, qx]), 0.0))
    out = c.copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        out[..., :3] = np.where(usable[..., None], cc + acc / D[..., None], c[..., :3])
    return out, dict(filtered=usable, D=D, C=Cmax, L=Lmax)


def filter_fp64(c, guide, p):
    """every pass in fp64"""
    cur = np.asarray(c, np.float64)
    for k in range(p["passes"]):
        cur, _ = pass_fp64(cur, guide, *pass_constants(p, k))
    return cur


def pass_bound(aux, inv_sc):
    """The bound of one fp32 pass against pass_fp64 on the same input, per pixel (test_denoise_cpu.py derives it):
        |out32 - out64| <= U C ((16 + 12 L inv_sc) / D + 53)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(aux["filtered"], U * aux["C"] * ((16.0 + 12.0 * aux["L"] * inv_sc) / aux["D"] + 53.0), 0.0)


# ---------------------------------------------------------------------------------------------------------------- synthetic images
@functools.lru_cache(maxsize=None)
def synthetic(w, h, seed=5):
    """(rgba, aov) float32 [h][w][4]: seeded random colour in [0, 4); a guide with alpha == 0 holes (isolated pixels and blocks), an alpha
    ramp in x, z_front steps, all inside the view AOV's contract (alpha == 0 <=> {0, 0, +inf, +inf}); one NaN and one +inf colour pixel."""
    rng = np.random.default_rng(seed)
    rgba = (rng.random((h, w, 4)) * 4.0).astype(np.float32)
    x = np.arange(w, dtype=np.float64)[None, :].repeat(h, 0)
    y = np.arange(h, dtype=np.float64)[:, None].repeat(w, 1)
    alpha = 0.05 + 0.9 * x / max(w - 1, 1)                                   # a ramp ...
    alpha[h // 2:, :] = 0.8 - 0.6 * (x[h // 2:, :] / max(w - 1, 1)) ** 2      # ... and another, against it, below
    z = 50.0 + 0.125 * x + 0.0625 * y
    z[:, w // 3:] += 6.0                                                     # steps in z_front
    z[h // 4:h // 2, 2 * w // 3:] += 11.5
    hole = rng.random((h, w)) < 0.06                                         # isolated holes
    hole[3:9, 5:14] = True                                                   # blocks of them, one at the image's edge
    hole[h - 7:, w - 11:w - 2] = True
    hole[h // 2 - 1:h // 2 + 2, :4] = True
    alpha[hole], z[hole] = 0.0, np.inf
    tau = np.where(hole, 0.0, -np.log1p(-np.minimum(alpha, 0.999)))
    aov = np.stack([alpha, tau, z, np.where(tau >= math.log(2.0), z + 1.0, np.inf)], axis=-1).astype(np.float32)
    solid = np.argwhere(~hole)
    nan_yx, inf_yx = solid[len(solid) // 3], solid[2 * len(solid) // 3]
    rgba[nan_yx[0], nan_yx[1], 1] = np.nan
    rgba[inf_yx[0], inf_yx[1], 2] = np.inf
    rgba.setflags(write=False)
    aov.setflags(write=False)
    return rgba, aov


def nonfinite_pixels(rgba):
    return np.argwhere(~np.isfinite(np.asarray(rgba)[..., :3]).all(axis=-1))


SYNTHETIC_SIZES = ((48, 32), (44, 36), (97, 41))      # (w, h): whole tiles, ragged, more than one 32 x 8 tile both ways with odd sizes

# ---------------------------------------------------------------------------------------------------------------- rendered cases
RENDERED = ("cloud_v3", "blocks_v3")
W, H = V.W, V.H
PATH_LENGTH = 32
QUALITY_FRAMES = (1, 4, 16)
QUALITY_SEEDS = (3, 4)
TRUTH_FRAMES, TRUTH_SEED = 1024, 99
QUALITY_BOUND = 0.5


def reference_guide(sc, name):
    """the case's guide [h][w][4] float32 from the fp64 reference of the view AOV (view_aov_reference.reference_view)"""
    scene, cam = V.cases(sc)[name]
    ref = V.reference_view(scene, cam)
    tau, zf, zh = ref["tau"][..., 0], ref["z_front"][..., 0], ref["z_half"][..., 0]
    return np.stack([-np.expm1(-tau), tau, zf, zh], axis=-1).astype(np.float32)


def mse(img, truth):
    """mean squared error over R, G, B of every pixel, fp64"""
    a, b = np.asarray(img, np.float64)[..., :3], np.asarray(truth, np.float64)[..., :3]
    return float(((a - b) ** 2).mean())


def same_bits(a, b):
    return V.same_bits(a, b)
