"""What the ray-AOV tests share (test_ray_aov_cpu.py, test_gpu_ray_aov.py): the ray sets, an fp64 reference of {tau, z_front, z_half} over a
ray SEGMENT, and the stable-ray rule -- view_aov_reference's, applied to records {ox, oy, oz, t_min, dx, dy, dz, t_max}.

The reference is of the range: the ray is the fp32 record taken exactly, the range [t0, t1] = [max(box entry, t_min, 0), min(box exit,
t_max)], the parameters of all voxel planes inside it are sorted and every segment's voxel is looked up at its midpoint (what
view_aov_reference.reference_ray does for the whole ray).  The five rays of the stable rule share the record's origin and range and
differ in direction alone; they keep the record's |d|, so that t means the same on all five."""
import functools
import math

import numpy as np

import view_aov_reference as R

W, H = R.W, R.H
LIGHT = 32                      # light_view images are LIGHT x LIGHT
OTHER_LIGHT = (0.4, -0.7, 0.59)


# ---------------------------------------------------------------------------------------------------------------- ray sets
def scene_diagonal(scene):
    return float(np.linalg.norm(np.asarray(scene["size"], np.float64)))


def sphere_depths(rays, radius, far=False):
    """fp32 [...] depth image of a sphere of `radius` at the origin: the parameter of the near (far: the far) root along each record's
    ray, +inf where the ray misses the sphere or the root lies behind the origin"""
    r = np.asarray(rays, np.float64)
    o, d = r[..., 0:3], r[..., 4:7]
    a = (d * d).sum(-1)
    b = (o * d).sum(-1)
    c = (o * o).sum(-1) - radius * radius
    disc = b * b - a * c
    with np.errstate(invalid="ignore"):
        root = np.sqrt(np.where(disc >= 0.0, disc, np.nan))
        t = (-b + (root if far else -root)) / a
    return np.where(np.isfinite(t) & (t > 0.0), t, np.inf).astype(np.float32)


def with_depth(rays, depth):
    """the records with t_max replaced by the depth"""
    out = np.array(rays, np.float32, copy=True)
    out[..., 7] = depth
    return out


def holdout_rays(api, sc, name):
    """(scene, camera, depth [H][W], records [H][W][8]) of view `name` held out to a sphere of radius 0.2 |size| at the origin; the camera
    inside the box sits inside the sphere too and is held out to the sphere's far root"""
    scene, cam = R.cases(sc)[name]
    rays = api.camera_rays(cam, W, H)
    depth = sphere_depths(rays, 0.2 * scene_diagonal(scene), far=(name == "blocks_inside"))
    return scene, cam, depth, with_depth(rays, depth)


def volume_scene(sc, volume):
    return sc.make_scene(R.blocks_volume() if volume == "blocks" else R.cloud_volume(), scene_id=4)


def light_rays(api, sc, volume, light_dir=None, w=LIGHT, h=LIGHT):
    """(scene, view, records [h][w][8]) of scene.light_view"""
    scene = volume_scene(sc, volume)
    view = sc.light_view(scene, w, h, light_dir=light_dir)
    return scene, view, api.ortho_rays(view, w, h)


@functools.lru_cache(maxsize=None)
def _random_segments(size_key):
    size = np.array(size_key, np.float64)
    L = float(np.linalg.norm(size))
    rng = np.random.default_rng(11)
    n = 1024
    p = rng.standard_normal((n, 3))
    o = 0.75 * L * p / np.linalg.norm(p, axis=-1, keepdims=True)
    target = (rng.random((n, 3)) - 0.5) * size * 0.8
    d = target - o
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    t = np.sort(rng.random((n, 2)) * 1.6 * L, axis=-1)
    rays = np.concatenate([o, t[:, :1], d, t[:, 1:]], axis=-1).astype(np.float32)
    rays.setflags(write=False)
    return rays


def random_segments(scene):
    """1024 records: ray i runs from a point of the sphere of radius 0.75 |size| towards a uniform point of the box scaled by 0.8, with
    t_min < t_max the sorted pair of two uniform draws in [0, 1.6 |size|] (default_rng(11))"""
    return _random_segments(tuple(float(x) for x in np.asarray(scene["size"], np.float32)))


def degenerate_records():
    """(records [n][8], what each is): every one must give the empty result"""
    inf, nan = np.inf, np.nan
    good = [60.0, 3.0, -2.0, 0.0, -1.0, 0.0, 0.0, inf]      # a ray along -x through the box
    recs, what = [], []

    def add(name, **kw):
        r = list(good)
        for k, v in kw.items():
            r[int(k[1:])] = v
        recs.append(r)
        what.append(name)
    add("t_max = 0", _7=0.0)
    add("t_max < 0", _7=-5.0)
    add("t_max = t_min", _3=20.0, _7=20.0)
    add("t_max < t_min", _3=30.0, _7=20.0)
    add("t_min = +inf", _3=inf)
    add("t_max = -inf", _7=-inf)
    for k in range(8):
        add("NaN in number %d" % k, **{"_%d" % k: nan})
    add("zero direction", _4=0.0, _5=0.0, _6=0.0)
    for k in (4, 5, 6):
        add("+inf direction %d" % k, **{"_%d" % k: inf})
        add("-inf direction %d" % k, **{"_%d" % k: -inf})
    for k in (0, 1, 2):
        add("+inf origin %d" % k, **{"_%d" % k: inf})
        add("-inf origin %d" % k, **{"_%d" % k: -inf})
    add("a range in front of the box", _3=0.0, _7=1.0)
    add("a range behind the box", _3=500.0, _7=600.0)
    add("pointing away", _4=1.0)
    return np.array(recs, np.float32), what


EMPTY = np.array([0.0, 0.0, np.inf, np.inf], np.float32)


def is_empty(a):
    """per record: the empty result's bits"""
    a = np.ascontiguousarray(a, np.float32)
    return (a.view(np.uint32) == EMPTY.view(np.uint32)).all(axis=-1)


# ---------------------------------------------------------------------------------------------------------------- the fp64 reference
def reference_segment(vol, size, density_factor, ro, rd, t_min, t_max):
    """(tau, z_front, z_half, crossings, sigma of the voxel where tau reaches ln 2, the range's end) over t in [max(t_min, 0), t_max] of
    one ray in fp64; nothing there: (0, inf, inf, 0, 0, 0)"""
    none = (0.0, math.inf, math.inf, 0, 0.0, 0.0)
    nz, ny, nx = vol.shape
    n = np.array([nx, ny, nz])
    size = np.asarray(size, np.float64)
    lo, hi = -0.5 * size, 0.5 * size
    if not (np.isfinite(ro).all() and np.isfinite(rd).all()) or math.isnan(t_min) or math.isnan(t_max):
        return none
    t0, t1 = max(0.0, t_min), math.inf
    for a in range(3):
        if rd[a] == 0.0:
            if not (lo[a] < ro[a] < hi[a]):
                return none
            continue
        ta, tb = (lo[a] - ro[a]) / rd[a], (hi[a] - ro[a]) / rd[a]
        t0, t1 = max(t0, min(ta, tb)), min(t1, max(ta, tb))
    if not math.isfinite(t1):
        return none
    t1 = min(t1, t_max)
    if not (t0 < t1):
        return none
    ts = [np.array([t0, t1])]
    for a in range(3):
        if rd[a] != 0.0:
            t = (lo[a] + np.arange(1, n[a]) * (size[a] / n[a]) - ro[a]) / rd[a]
            ts.append(t[(t > t0) & (t < t1)])
    t = np.sort(np.concatenate(ts))
    mid = 0.5 * (t[1:] + t[:-1])
    p = ro[None, :] + mid[:, None] * rd[None, :]
    idx = np.clip(np.floor((p - lo) / (size / n)).astype(np.int64), 0, n - 1)
    sigma = density_factor * vol[idx[:, 2], idx[:, 1], idx[:, 0]].astype(np.float64) / 255.0
    seg = t[1:] - t[:-1]
    cum = np.concatenate([[0.0], np.cumsum(sigma * seg)])
    tau = float(cum[-1])
    lit = np.nonzero((sigma > 0.0) & (seg > 0.0))[0]
    z_front = float(t[lit[0]]) if lit.size else math.inf
    z_half, s_cross = math.inf, 0.0
    if tau >= R.LN2:
        k = int(np.searchsorted(cum, R.LN2, side="left")) - 1      # cum[k] < ln 2 <= cum[k + 1]
        s_cross = float(sigma[k])
        z_half = float(t[k] + (R.LN2 - cum[k]) / sigma[k])
    return tau, z_front, z_half, int(t.size - 2), s_cross, float(t1)


def perturbed(d):
    """view_aov_reference's five directions of a ray, at the record's own length (the centre is d itself)"""
    d = np.asarray(d, np.float64)
    length = float(np.linalg.norm(d))
    out = R.perturbed(d / length) * length
    out[0] = d
    return out


def reference_rays(scene, rays, centre_only=False):
    """the reference of every record on its five rays, as view_aov_reference.reference_view returns it: arrays [...][5] (tau, z_front,
    z_half), [...] (crossings, sigma_cross, t1 of the centre ray) and the masks and spreads of summarize().  centre_only: the centre ray
    alone is evaluated (for its crossings and t1; the other four columns repeat it, so nothing is unstable)"""
    vol = np.asarray(scene["density"])
    size = np.asarray(scene["size"], np.float32).astype(np.float64)
    rho = float(np.float32(scene["density_factor"]))
    recs = np.asarray(rays, np.float32).astype(np.float64)
    shape = recs.shape[:-1]
    flat = recs.reshape(-1, 8)
    n = flat.shape[0]
    tau = np.zeros((n, 5))
    zf = np.full((n, 5), math.inf)
    zh = np.full((n, 5), math.inf)
    crossings = np.zeros(n, np.int64)
    s_cross = np.zeros(n)
    t1 = np.zeros(n)
    for i in range(n):
        q = flat[i]
        if not np.isfinite(q[4:7]).all() or not q[4:7].any():
            continue
        for k, d in enumerate(perturbed(q[4:7])):
            r = reference_segment(vol, size, rho, q[0:3], d, q[3], q[7])
            tau[i, k], zf[i, k], zh[i, k] = r[0], r[1], r[2]
            if k == 0:
                # N of view_aov_reference.tolerances counts the roundings of a walk, one per segment summed.  A whole ray sums N + 1 segments
                # for its N planes and N is large; a range inside ONE voxel crosses no plane and still sums one segment, whose product no
                # fp32 walk gets exactly: N = 1 there.  With a plane inside the range N is the planes' number, as for the whole ray.
                crossings[i], s_cross[i], t1[i] = (max(r[3], 1) if r[5] > 0.0 else 0), r[4], r[5]
                if centre_only:
                    tau[i, :], zf[i, :], zh[i, :] = r[0], r[1], r[2]
                    break
    return R.summarize(dict(tau=tau.reshape(shape + (5,)), z_front=zf.reshape(shape + (5,)), z_half=zh.reshape(shape + (5,)),
                            crossings=crossings.reshape(shape), sigma_cross=s_cross.reshape(shape), t1=t1.reshape(shape)))
