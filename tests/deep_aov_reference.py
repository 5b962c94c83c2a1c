"""What the deep-AOV tests share (test_deep_aov_cpu.py, test_gpu_deep_aov.py): the level sets, the ray sets (ray_aov_reference's, and the
blocks volume with a dense block), and an fp64 reference of the depths at which a ray SEGMENT reaches given optical depths.

The reference (aov_reference.reference_segment) is ray_aov_reference.reference_segment's with a level in place of ln 2: the ray is the fp32 record taken
exactly, the parameters of all voxel planes inside its range are sorted, every segment's voxel is looked up at its midpoint, and level L is
crossed in the segment k with cum[k] < L <= cum[k + 1], at t[k] + (L - cum[k]) / sigma[k].  One pass over a ray serves every level of every
level set, so a ray set is walked once."""
import functools

import numpy as np

import aov_reference as A
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
reference_segment = A.reference_segment      # (vol, size, density_factor, ro, rd, t_min, t_max, levels): the shared reference as it is


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
    recs = np.asarray(rays, np.float32).astype(np.float64)
    shape = recs.shape[:-1]
    ref = A.reference_records(scene, recs.reshape(-1, 8), Q.perturbed, levels)
    seg_of = ref["segment"]
    same = np.zeros(seg_of.shape, bool)
    for sl in where.values():
        same[sl.start + 1:sl.stop] = (seg_of[sl.start + 1:sl.stop] >= 0) & (seg_of[sl.start + 1:sl.stop] == seg_of[sl.start:sl.stop - 1])
    K = (levels.size,)
    _REF[name] = dict(tau=ref["tau"].reshape(shape + (5,)), z_front=ref["z_front"].reshape(shape + (5,)), z=ref["z"].reshape(K + shape + (5,)),
                      sigma_cross=ref["sigma_cross"].reshape(K + shape), crossings=A.segments_summed(ref).reshape(shape),      # (N: a segment's)
                      t1=ref["t1"].reshape(shape), same_voxel=same.reshape(K + shape), where=where)
    return _REF[name]


def level_reference(ref, a):
    """level a of all_levels as a reference of view_aov_reference's shape: that level's depth stands where z_half stands, with its own
    crossing voxel's sigma, so that summarize / unstable_share / tolerances apply as they are"""
    return R.summarize(dict(tau=ref["tau"], z_front=ref["z_front"], z_half=ref["z"][a], crossings=ref["crossings"],
                            sigma_cross=ref["sigma_cross"][a], t1=ref["t1"]))
