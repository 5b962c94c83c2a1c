"""What the deep-AOV tests share (test_deep_aov_cpu.py, test_gpu_deep_aov.py): the level sets, the ray sets (ray_aov_reference's, and the
blocks volume with a dense block), and an fp64 reference of the depths at which a ray SEGMENT reaches given optical depths.

The reference is ray_aov_reference.reference_segment's construction with a level in place of ln 2: the ray is the fp32 record taken
exactly, the parameters of all voxel planes inside its range are sorted, every segment's voxel is looked up at its midpoint, and level L is
crossed in the segment k with cum[k] < L <= cum[k + 1], at t[k] + (L - cum[k]) / sigma[k].  One pass over a ray serves every level of every
level set, so a ray set is walked once."""
import functools
import math

import numpy as np

import ray_aov_reference as Q
import view_aov_reference as R

LN2_F32 = np.float32(float.fromhex("0x1.62e430p-1"))      # NRC_AOV_LN2


def level_sets(sc):
    """{name: fp32 levels}: K = 1 (z_half's level), 2, 7, 32 (fine enough that one dense voxel crosses several), and a set whose top level
    no ray of the fixtures reaches (their largest optical depth is about 21)"""
    return {
        "ln2": np.array([LN2_F32], np.float32),
        "k2": np.array([0.25, 2.0], np.float32),
        "k7": sc.deep_levels(7, 3.0),
        "k32": sc.deep_levels(32, 1.6),
        "beyond": np.array([0.5, 5.0, 1000.0], np.float32),
    }


LEVEL_SET_NAMES = ("ln2", "k2", "k7", "k32", "beyond")


@functools.lru_cache(maxsize=None)
def dense_blocks_volume():
    """the blocks volume with a block of byte 255 in its middle: sigma = density_factor there, 1.77 of optical depth per voxel"""
    v = np.array(R.blocks_volume(), copy=True)
    v[10:18, 3:9, 6:14] = 255
    v.setflags(write=False)
    return v


def volume_scene(sc, volume):
    return sc.make_scene(dense_blocks_volume(), scene_id=4) if volume == "dense" else Q.volume_scene(sc, volume)


VIEWS = ("blocks_v3", "blocks_v1", "cloud_v3", "blocks_inside")
LIGHTS = (("blocks", None), ("cloud", None), ("blocks", Q.OTHER_LIGHT), ("cloud", Q.OTHER_LIGHT))
SET_NAMES = tuple("holdout_" + v for v in VIEWS) + tuple("light_%s_%s" % (v, "scene" if l is None else "other") for v, l in LIGHTS) + \
    ("random_blocks", "random_dense", "random_cloud")
ACCURACY_SETS = SET_NAMES[:-1]      # (the cloud's random list is over the unstable cap, as for the ray AOV: bitwise checks only)
_SETS = {}


def ray_sets(api, sc):
    """{name: (scene, records)}: the ray AOV's sets and the random segments through the dense blocks volume"""
    if not _SETS:
        for name in VIEWS:
            scene, _, _, rays = Q.holdout_rays(api, sc, name)
            _SETS["holdout_" + name] = (scene, rays)
        for volume, light in LIGHTS:
            scene, _, rays = Q.light_rays(api, sc, volume, light)
            _SETS["light_%s_%s" % (volume, "scene" if light is None else "other")] = (scene, rays)
        for volume in ("blocks", "dense", "cloud"):
            scene = volume_scene(sc, volume)
            _SETS["random_" + volume] = (scene, Q.random_segments(scene))
    return _SETS


# ---------------------------------------------------------------------------------------------------------------- the fp64 reference
def reference_segment(vol, size, density_factor, ro, rd, t_min, t_max, levels):
    """(tau, z_front, z [K], crossings, sigma of the voxel where tau reaches each level [K], the range's end, index of that voxel's segment
    [K]) over t in [max(t_min, 0), t_max] of one ray in fp64; nothing there: (0, inf, inf.., 0, 0.., 0, -1..)"""
    K = len(levels)
    none = (0.0, math.inf, np.full(K, math.inf), 0, np.zeros(K), 0.0, np.full(K, -1))
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
    z, s_cross, where = np.full(K, math.inf), np.zeros(K), np.full(K, -1)
    for i, L in enumerate(levels):
        if tau >= L:
            k = int(np.searchsorted(cum, L, side="left")) - 1      # cum[k] < L <= cum[k + 1]
            s_cross[i] = sigma[k]
            z[i] = t[k] + (L - cum[k]) / sigma[k]
            where[i] = k
    return tau, z_front, z, int(t.size - 2), s_cross, float(t1), where


def all_levels(sc):
    """every level of every level set, in LEVEL_SET_NAMES' order, as exact fp64 values of the fp32 levels; and each set's slice of them"""
    sets = level_sets(sc)
    cat = np.concatenate([sets[n].astype(np.float64) for n in LEVEL_SET_NAMES])
    at, where = 0, {}
    for n in LEVEL_SET_NAMES:
        where[n] = slice(at, at + sets[n].size)
        at += sets[n].size
    return cat, where


_REF = {}


def reference(api, sc, name):
    """The reference of ray set `name` on its five rays (view_aov_reference's stable rule, ray_aov_reference.perturbed), once per session:
    dict of tau, z_front [...][5]; z [A][...][5] and sigma_cross [A][...] for the A levels of all_levels; crossings, t1 [...];
    same_voxel [A][...]: the centre ray reaches level a in the same voxel segment as level a - 1 of its own level set"""
    if name in _REF:
        return _REF[name]
    scene, rays = ray_sets(api, sc)[name]
    levels, where = all_levels(sc)
    A = levels.size
    vol = np.asarray(scene["density"])
    size = np.asarray(scene["size"], np.float32).astype(np.float64)
    rho = float(np.float32(scene["density_factor"]))
    recs = np.asarray(rays, np.float32).astype(np.float64)
    shape = recs.shape[:-1]
    flat = recs.reshape(-1, 8)
    n = flat.shape[0]
    tau = np.zeros((n, 5))
    zf = np.full((n, 5), math.inf)
    z = np.full((A, n, 5), math.inf)
    s_cross = np.zeros((A, n))
    seg_of = np.full((A, n), -1)
    crossings = np.zeros(n, np.int64)
    t1 = np.zeros(n)
    for i in range(n):
        q = flat[i]
        if not np.isfinite(q[4:7]).all() or not q[4:7].any():
            continue
        for k, d in enumerate(Q.perturbed(q[4:7])):
            r = reference_segment(vol, size, rho, q[0:3], d, q[3], q[7], levels)
            tau[i, k], zf[i, k], z[:, i, k] = r[0], r[1], r[2]
            if k == 0:
                crossings[i], s_cross[:, i], t1[i], seg_of[:, i] = (max(r[3], 1) if r[5] > 0.0 else 0), r[4], r[5], r[6]      # (N: ray_aov_reference.reference_rays)
    same = np.zeros((A, n), bool)
    for sl in where.values():
        same[sl.start + 1:sl.stop] = (seg_of[sl.start + 1:sl.stop] >= 0) & (seg_of[sl.start + 1:sl.stop] == seg_of[sl.start:sl.stop - 1])
    _REF[name] = dict(tau=tau.reshape(shape + (5,)), z_front=zf.reshape(shape + (5,)), z=z.reshape((A,) + shape + (5,)),
                      sigma_cross=s_cross.reshape((A,) + shape), crossings=crossings.reshape(shape), t1=t1.reshape(shape),
                      same_voxel=same.reshape((A,) + shape), where=where)
    return _REF[name]


def level_reference(ref, a):
    """level a of all_levels as a reference of view_aov_reference's shape: that level's depth stands where z_half stands, with its own
    crossing voxel's sigma, so that summarize / unstable_share / tolerances apply as they are"""
    return R.summarize(dict(tau=ref["tau"], z_front=ref["z_front"], z_half=ref["z"][a], crossings=ref["crossings"],
                            sigma_cross=ref["sigma_cross"][a], t1=ref["t1"]))
