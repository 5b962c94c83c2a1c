"""The one fp64 reference of the AOV tests: what view_aov_reference, ray_aov_reference and deep_aov_reference evaluate (they keep the
fixtures, the ray sets, the stable rule and the tolerances; this module knows none of them).

The reference knows nothing of a voxel walk: the ray is taken exactly as given, its range is [max(box entry, t_min, 0), min(box exit,
t_max)], the parameters of ALL voxel planes inside the range are sorted, and the voxel of every segment between two neighbours is looked
up at the segment's midpoint.  Level L of the optical depth is crossed in the segment k with cum[k] < L <= cum[k + 1], at
t[k] + (L - cum[k]) / sigma[k]: z_half is the level ln 2, the deep AOV's planes are the caller's levels."""
import math

import numpy as np


def reference_segment(vol, size, density_factor, ro, rd, t_min, t_max, levels=()):
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


def reference_records(scene, records, perturbed, levels, centre_only=False):
    """The reference of n fp64 records {ox, oy, oz, t_min, dx, dy, dz, t_max} on five rays each: perturbed(d) gives a record's five
    directions [5][3], the centre first; they share the record's origin and range.  Dict of tau, z_front [n][5]; z [K][n][5]; and of the
    centre ray sigma_cross, segment [K][n] (reference_segment's), planes (the voxel planes inside its range) and t1 [n].  A record whose
    direction is zero or not finite keeps the empty result.  centre_only: the centre ray alone is evaluated and the other four columns
    repeat it."""
    vol = np.asarray(scene["density"])
    size = np.asarray(scene["size"], np.float32).astype(np.float64)
    rho = float(np.float32(scene["density_factor"]))
    n, K = records.shape[0], len(levels)
    tau = np.zeros((n, 5))
    zf = np.full((n, 5), math.inf)
    z = np.full((K, n, 5), math.inf)
    s_cross = np.zeros((K, n))
    segment = np.full((K, n), -1)
    planes = np.zeros(n, np.int64)
    t1 = np.zeros(n)
    for i in range(n):
        q = records[i]
        if not np.isfinite(q[4:7]).all() or not q[4:7].any():
            continue
        for k, d in enumerate(perturbed(q[4:7])):
            r = reference_segment(vol, size, rho, q[0:3], d, q[3], q[7], levels)
            tau[i, k], zf[i, k], z[:, i, k] = r[0], r[1], r[2]
            if k == 0:
                planes[i], s_cross[:, i], t1[i], segment[:, i] = r[3], r[4], r[5], r[6]
                if centre_only:
                    tau[i, :], zf[i, :], z[:, i, :] = r[0], r[1], r[2][:, None]
                    break
    return dict(tau=tau, z_front=zf, z=z, sigma_cross=s_cross, segment=segment, planes=planes, t1=t1)


def segments_summed(ref):
    """N of view_aov_reference.tolerances for a ray SEGMENT.  N counts the roundings of a walk, one per segment summed.  A whole ray sums
    N + 1 segments for its N planes and N is large: the view AOV takes the planes' number as it is.  A range inside ONE voxel crosses no
    plane and still sums one segment, whose product no fp32 walk gets exactly: N = 1 there.  With a plane inside the range N is the
    planes' number, as for the whole ray; an empty range sums nothing."""
    return np.where(ref["t1"] > 0.0, np.maximum(ref["planes"], 1), 0)
