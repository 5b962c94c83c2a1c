"""What the reproject tests share (test_reproject_cpu.py, test_gpu_reproject.py): the numpy fp64 statement of the rule (include/nrc_hpm.h,
"Reproject"), the synthetic images, the cases and the error bound of the fp32 code against the statement.

The fp64 statement follows the contract's rule with real arithmetic in place of fp32's: the same ray (the fp32 inv_proj_view and position,
evaluated in fp64 at u = x / w, v = y / h), the same four taps in the same roles, the weight b exp(-d), the mean formed around the centre.
What the contract fixes in fp32 is taken over as it stands: N (the fp64 inverse rounded to fp32) and the inverse sigmas (1.0f / sigma)."""
import functools
import math

import numpy as np

import denoise_reference as D
import view_aov_reference as V

DEFAULTS = dict(max_history=64.0, sigma_alpha=0.1, sigma_depth=4.0)
U = 2.0 ** -24      # fp32's unit roundoff
# What the bound assumes of the fp32 solve (steps 3 - 5 of the rule) against the fp64 one on the tests' cameras.  They stand at most 73 from
# the origin (radius 70, height 20) and the medium lies within half the box's diagonal, 53.75, of it (scene.volume_size: the box's extent
# has length 107.5), so a depth is at most 73 + 54 and L = |ro| + z <= SCALE = 200.  The reprojected position is within eps_pos(w, h)
# pixels per axis, |D| within EPS_DIST.  test_reproject_cpu.py derives both, measures them with solve_f32 and asserts them.
SCALE = 200.0
EPS_DIST = 9.0 * U * SCALE


def eps_pos(w, h):
    return 45.0 * U * max(w, h)


SYNTHETIC_SIZES = D.SYNTHETIC_SIZES
SMALL = (9, 7)
RENDERED = D.RENDERED
W, H = V.W, V.H
PATH_LENGTH = D.PATH_LENGTH
ORBIT_VIEWS, ORBIT_FRAMES = 8, 4
QUALITY_SEEDS = (3, 4)
TRUTH_FRAMES, TRUTH_SEED = D.TRUTH_FRAMES, D.TRUTH_SEED
# MSE(accumulated) / MSE(raw) at the orbit's last view, with the fp64 statement chained view to view (test_reproject_cpu.py's docstring and
# DESIGN.md section 4.20): cloud_v3 seed 3, seed 4; blocks_v3 seed 3, seed 4.  The tests assert <= 1.5 x the largest.
MEASURED_RATIOS = {("cloud_v3", 3): 0.162, ("cloud_v3", 4): 0.106, ("blocks_v3", 3): 0.229, ("blocks_v3", 4): 0.371}
QUALITY_BOUND = 1.5 * max(MEASURED_RATIOS.values())
NO_HISTORY_CAP = 0.02


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def inverse_sigmas(p):
    """(inv_sa, inv_sz) as the fp32 numbers the contract defines"""
    f32 = np.float32
    with np.errstate(divide="ignore"):
        return float(f32(1.0) / f32(p["sigma_alpha"])), float(f32(1.0) / f32(p["sigma_depth"]))


def camera_f64(cam):
    """(m [16] column-major, pos [3]): the camera's fp32 numbers, widened"""
    return np.asarray(cam["inv_proj_view"], np.float32).astype(np.float64).reshape(16), np.asarray(cam["pos"], np.float32).astype(np.float64)


def solve_matrix(cam):
    """[A B C] of the camera in fp64 ([k][0 .. 2] = A_k, B_k, C_k) -- a pixel's ray direction is ~ sx A + sy B + C"""
    m, pos = camera_f64(cam)
    return np.array([[m[k] - pos[k] * m[3], m[4 + k] - pos[k] * m[7], m[12 + k] - pos[k] * m[15]] for k in range(3)])


def solve_n(cam):
    """N = [A B C]^-1, inverted in fp64 and rounded to fp32 (row-major [9], widened again): None for a singular camera"""
    M = solve_matrix(cam)
    det = float(np.linalg.det(M))
    if det == 0.0 or not math.isfinite(det):
        return None
    N = np.linalg.inv(M).astype(np.float32)
    return N.astype(np.float64).reshape(9) if np.isfinite(N).all() else None


def representative_depth(g):
    """z = finite(z_half) ? z_half : z_front of a guide [..][4]"""
    return np.where(np.isfinite(g[..., 3]), g[..., 3], g[..., 2])


def solve_f64(cam, hist_cam, z, w, h):
    """steps 3 - 5 in fp64 for depths z [h][w] (finite): dict(fx, fy, dist, front)"""
    dirs, pos = V.ray_directions(cam, w, h)
    hm, hpos = camera_f64(hist_cam)
    N = solve_n(hist_cam).reshape(3, 3)
    Dv = pos + z[..., None] * dirs - hpos
    q = Dv @ N.T
    with np.errstate(invalid="ignore", divide="ignore"):
        sx, sy = q[..., 0] / q[..., 2], q[..., 1] / q[..., 2]
        ww = hm[7] * sy + hm[3] * sx + hm[15]
        front = q[..., 2] * ww > 0.0
        return dict(fx=(sx + 1.0) * 0.5 * w, fy=(sy + 1.0) * 0.5 * h, dist=np.linalg.norm(Dv, axis=-1), front=front)


def solve_f32(cam, hist_cam, z, w, h):
    """steps 3 - 5 as the fp32 code forms them (csrc/nrc_reproject.hpp), operation for operation in numpy float32; a fused multiply-add is
    an exact fp64 product + one fp64 sum rounded to fp32 (view_aov_reference.ray_directions_f32 has the argument)"""
    f32 = np.float32

    def r(x):
        return np.asarray(x, np.float64).astype(f32)

    def fma(a, b, c):
        return r(np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64))
    rd = V.ray_directions_f32(cam, w, h)
    pos = np.asarray(cam["pos"], f32)
    hm, hpos = np.asarray(hist_cam["inv_proj_view"], f32).reshape(16), np.asarray(hist_cam["pos"], f32)
    N = solve_n(hist_cam).astype(f32)
    z = r(z)
    Dv = [r(fma(z, rd[..., k], pos[k]) - hpos[k]) for k in range(3)]
    q = [fma(N[3 * k + 2], Dv[2], fma(N[3 * k + 1], Dv[1], r(N[3 * k] * Dv[0]))) for k in range(3)]
    with np.errstate(invalid="ignore", divide="ignore"):
        sx, sy = r(q[0] / q[2]), r(q[1] / q[2])
        ww = fma(hm[7], sy, fma(hm[3], sx, hm[15]))
        dist = r(np.sqrt(fma(Dv[2], Dv[2], fma(Dv[1], Dv[1], r(Dv[0] * Dv[0]))).astype(np.float64)))
        fx, fy = r(r(r(sx + f32(1.0)) * f32(0.5)) * f32(w)), r(r(r(sy + f32(1.0)) * f32(0.5)) * f32(h))
        return dict(fx=fx.astype(np.float64), fy=fy.astype(np.float64), dist=dist.astype(np.float64), front=r(q[2] * ww) > 0.0)


def reproject_fp64(hist, rgba, frames, aov, cam, p, terms=("alpha", "depth")):
    """The rule in fp64.  hist: None or (rgba [h][w][4], count [h][w], aov [h][w][4], camera); rgba, aov [h][w][4]; frames > 0.  Returns
    (out [h][w][4] fp64, out_n [h][w] fp64, aux) with aux = dict(blended [h][w] bool: the pixel did not pass through; Wsum [h][w]: acc_w;
    and, over the usable history pixels of the 4 x 4 window around the reprojected position -- every tap either code can reach when the
    positions differ by less than a pixel --, Cd: the largest |c_Q - c_P| of a component, C: the largest |component| of them and of c_P,
    Nmax: the largest count).  terms: the terms of d that are formed at all (the sigma = +inf tests leave one out)."""
    c = np.asarray(rgba, np.float64)
    g = np.asarray(aov, np.float64)
    h, w = c.shape[:2]
    out, out_n = c.copy(), np.full((h, w), float(frames))
    zero = np.zeros((h, w))
    aux = dict(blended=np.zeros((h, w), bool), Wsum=zero.copy(), Cd=zero.copy(), C=zero.copy(), Nmax=zero.copy())
    if hist is None:
        return out, out_n, aux
    hc, hn, hg, hcam = np.asarray(hist[0], np.float64), np.asarray(hist[1], np.float64), np.asarray(hist[2], np.float64), hist[3]
    inv_sa, inv_sz = inverse_sigmas(p)
    usable = (g[..., 0] != 0.0) & np.isfinite(c[..., :3]).all(axis=-1)
    cc = np.where(usable[..., None], c[..., :3], 0.0)
    alpha = g[..., 0]
    s = solve_f64(cam, hcam, np.where(usable, representative_depth(g), 0.0), w, h)
    with np.errstate(invalid="ignore"):
        inside = usable & s["front"] & (s["fx"] >= -1.0) & (s["fx"] < w) & (s["fy"] >= -1.0) & (s["fy"] < h)
    fx, fy, dist = np.where(inside, s["fx"], 0.0), np.where(inside, s["fy"], 0.0), np.where(inside, s["dist"], 0.0)
    x0, y0 = np.floor(fx), np.floor(fy)
    tx, ty = fx - x0, fy - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    husable = (hg[..., 0] != 0.0) & np.isfinite(hc[..., :3]).all(axis=-1)
    hcc = np.where(husable[..., None], hc[..., :3], 0.0)
    hnn = np.where(husable, hn, 0.0)
    hz = np.where(husable, representative_depth(hg), 0.0)
    ha = hg[..., 0]
    acc_c, acc_w, acc_n = np.zeros((h, w, 3)), zero.copy(), zero.copy()
    for j in (-1, 0, 1, 2):
        for i in (-1, 0, 1, 2):
            qx, qy = x0 + i, y0 + j
            ok = inside & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            ok &= husable[qy, qx]
            aux["Cd"] = np.maximum(aux["Cd"], np.where(ok, np.abs(hcc[qy, qx] - cc).max(axis=-1), 0.0))
            aux["C"] = np.maximum(aux["C"], np.where(ok, np.maximum(np.abs(hcc[qy, qx]).max(axis=-1), np.abs(cc).max(axis=-1)), 0.0))
            aux["Nmax"] = np.maximum(aux["Nmax"], np.where(ok, np.abs(hnn[qy, qx]), 0.0))
            if i not in (0, 1) or j not in (0, 1):
                continue
            b = (tx if i else 1.0 - tx) * (ty if j else 1.0 - ty)
            d = zero.copy()
            if "alpha" in terms:
                d = d + np.abs(ha[qy, qx] - alpha) * inv_sa
            if "depth" in terms:
                d = d + np.abs(hz[qy, qx] - dist) * inv_sz
            wgt = np.where(ok, b * np.exp(-d), 0.0)
            acc_c += wgt[..., None] * (hcc[qy, qx] - cc)      # (around the centre, as the contract forms the mean)
            acc_w += wgt
            acc_n += wgt * hnn[qy, qx]
    blended = inside & (acc_w > 0.0)
    n_h = np.minimum(acc_n, float(np.float32(p["max_history"])))
    with np.errstate(invalid="ignore", divide="ignore"):
        a = n_h / (n_h + float(frames))
        out[..., :3] = np.where(blended[..., None], cc + a[..., None] * acc_c / acc_w[..., None], c[..., :3])
    out_n = np.where(blended, n_h + float(frames), float(frames))
    aux.update(blended=blended, Wsum=acc_w)
    return out, out_n, aux


def bounds(aux, frames, p):
    """(bound of a colour component, bound of the count) of the fp32 code against reproject_fp64, per pixel (test_reproject_cpu.py derives
    them):  with E_w = 4 eps_pos + EPS_DIST inv_sz + 48 U,
        |out32 - out64|     <= E_w Cd (2 min(1 / W, Nmax / n) + Nmax / n) + U (3 C + 12 Cd + 5 Cd Nmax W / n)
        |out_n32 - out_n64| <= Nmax (E_w + 5 U W) + U (max_history + n)"""
    _, inv_sz = inverse_sigmas(p)
    n = float(frames)
    h, w = aux["Wsum"].shape
    e_w = 4.0 * eps_pos(w, h) + EPS_DIST * inv_sz + 48.0 * U
    W, Cd, C, Nmax = aux["Wsum"], aux["Cd"], aux["C"], aux["Nmax"]
    with np.errstate(divide="ignore"):
        lever = np.minimum(np.where(W > 0.0, 1.0 / np.where(W > 0.0, W, 1.0), np.inf), Nmax / n)
    bc = e_w * Cd * (2.0 * lever + Nmax / n) + U * (3.0 * C + 12.0 * Cd + 5.0 * Cd * Nmax * W / n)
    bn = Nmax * (e_w + 5.0 * U * W) + U * (float(p["max_history"]) + n)
    return bc, bn


# ---------------------------------------------------------------------------------------------------------------- synthetic images
HISTORY_SEED = 11


@functools.lru_cache(maxsize=None)
def synthetic(w, h):
    """(rgba, aov, hist_rgba, hist_count, hist_aov): the current view is denoise_reference.synthetic(w, h); the history image and guide are
    the same construction from another seed (other holes, another NaN and +inf pixel); the counts are random in [1, 40], so that a
    max_history below 40 bites"""
    rgba, aov = D.synthetic(w, h)
    hist_rgba, hist_aov = D.synthetic(w, h, seed=HISTORY_SEED)
    counts = np.random.default_rng(HISTORY_SEED + 1).uniform(1.0, 40.0, (h, w)).astype(np.float32)
    counts.setflags(write=False)
    return rgba, aov, hist_rgba, counts, hist_aov


def camera_pairs(sc, w, h):
    """{name: (history camera, current camera)}: orbit steps of 0, 2 and 5 degrees from view_aov_reference's orbit view 3, and a dolly of 6
    along the view direction"""
    aspect = w / h
    start = 2.0 * math.pi * 3 / 8
    base = V.orbit_view(sc, 3, aspect=aspect)
    two = sc.orbit_cameras(180, radius=70.0, height=20.0, aspect=aspect, start_angle=start)[1]
    five = sc.orbit_cameras(72, radius=70.0, height=20.0, aspect=aspect, start_angle=start)[1]
    pos = np.asarray(base["pos"], np.float64)
    toward = -pos / np.linalg.norm(pos)
    dolly = sc.make_camera(pos=pos + 6.0 * toward, view_dir=toward, aspect=aspect)
    return {"same": (base, base), "orbit2": (base, two), "orbit5": (base, five), "dolly": (base, dolly)}


def orbit(sc, w=W, h=H):
    """the quality tests' orbit: 8 views 2 degrees apart, the first of them view_aov_reference's orbit view 3"""
    return sc.orbit_cameras(180, radius=70.0, height=20.0, aspect=w / h, start_angle=2.0 * math.pi * 3 / 8)[:ORBIT_VIEWS]


def chain(step, frames_of, guides, cams, n_frames, p):
    """accum, counts of the last view: step(hist, rgba, frames, aov, camera, params) -> (out, count), chained view to view"""
    hist = None
    for i, cam in enumerate(cams):
        out, cnt = step(hist, frames_of[i], n_frames, guides[i], cam, p)
        hist = (np.asarray(out, np.float32), np.asarray(cnt, np.float32), guides[i], cam)
    return hist[0], hist[1]


def step_fp64(hist, rgba, frames, aov, cam, p):
    out, cnt, _ = reproject_fp64(hist, rgba, frames, aov, cam, p)
    return out, cnt


mse = D.mse
same_bits = V.same_bits
