"""What the ray-AOV tests share (test_ray_aov_cpu.py, test_gpu_ray_aov.py): the ray sets, an fp64 reference of {tau, z_front, z_half} over a
ray SEGMENT, and the stable-ray rule -- view_aov_reference's, applied to records {ox, oy, oz, t_min, dx, dy, dz, t_max}.

The reference is of the range (aov_reference.reference_segment): the ray is the fp32 record taken exactly, the range [t0, t1] =
[max(box entry, t_min, 0), min(box exit, t_max)], the parameters of all voxel planes inside it are sorted and every segment's voxel is
looked up at its midpoint (what view_aov_reference.reference_ray asks of the whole ray).  The five rays of the stable rule share the record's origin and range and
differ in direction alone; they keep the record's |d|, so that t means the same on all five."""
import functools

import numpy as np

import aov_reference as A
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
    tau, z_front, z, crossings, s_cross, t1, _ = A.reference_segment(vol, size, density_factor, ro, rd, t_min, t_max, (R.LN2,))
    return tau, z_front, float(z[0]), crossings, float(s_cross[0]), t1


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
    recs = np.asarray(rays, np.float32).astype(np.float64)
    shape = recs.shape[:-1]
    ref = A.reference_records(scene, recs.reshape(-1, 8), perturbed, (R.LN2,), centre_only)
    # crossings: a segment's N, not the whole ray's number of planes (aov_reference.segments_summed)
    return R.summarize(dict(tau=ref["tau"].reshape(shape + (5,)), z_front=ref["z_front"].reshape(shape + (5,)),
                            z_half=ref["z"][0].reshape(shape + (5,)), crossings=A.segments_summed(ref).reshape(shape),
                            sigma_cross=ref["sigma_cross"][0].reshape(shape), t1=ref["t1"].reshape(shape)))
