"""Plain statements of the two operations at the image end of the frame, for the tests to compare the kernels with.  Nothing of the
product or of the oracle is imported here.

metrics_exact    ref/cmp1.comp, norm.comp, cmp2.comp (Reference::Result) with exact sums: every term formed in fp64, every sum math.fsum
composite_fp32   nrc/render.comp as k_composite states it: every operation a separately rounded fp32 operation

and the bound the metric tests hold the kernels to (metric_violations): each real metric within ONE fp32 ulp of the exact value rounded to
fp32, the valid count equal.  The kernels sum non-negative fp64 terms in a fixed tree: a relative error of at most n_terms * 2^-53 (7e-11 at
196 729 x 3 terms) against an fp32 half-ulp of 6e-8, so the rounded result differs only where the exact value sits on a rounding boundary,
and then by one ulp; own_var depends on the 1e-10 error of the mean in second order."""
import math

import numpy as np

METRICS = ("mse", "ref_mean", "own_mean", "own_var")
ULP_BOUND = 1


def valid_pixels(ref):
    """the pixels cmp1.comp:32 does not skip: NOT (ref.w == 0), an fp32 compare -- -0.0 is skipped; denormals, NaN and negative alphas count"""
    a = np.ascontiguousarray(ref, np.float32).reshape(-1, 4)[:, 3]
    return ~(a == np.float32(0.0))


def metrics_exact(ref, own):
    """{mse, ref_mean, own_mean, own_var, valid} of two RGBA32F images as Python floats (fp64); no valid pixel: all zeros"""
    r = np.ascontiguousarray(ref, np.float32).reshape(-1, 4)
    o = np.ascontiguousarray(own, np.float32).reshape(-1, 4)
    assert r.shape == o.shape
    v = valid_pixels(r)
    n = int(v.sum())
    if n == 0:
        return dict(mse=0.0, ref_mean=0.0, own_mean=0.0, own_var=0.0, valid=0.0)
    r3, o3 = r[v, :3].astype(np.float64), o[v, :3].astype(np.float64)
    inv = 1.0 / (3.0 * n)
    d = o3 - r3
    own_mean = math.fsum(o3.ravel()) * inv
    e = o3 - own_mean
    return dict(mse=math.fsum((d * d).ravel()) * inv, ref_mean=math.fsum(r3.ravel()) * inv, own_mean=own_mean,
                own_var=math.fsum((e * e).ravel()) * inv, valid=float(n))


def ulp_distance(a, b):
    """number of fp32 values between two fp32 numbers (0: the same value; +0 and -0 are the same); a NaN is infinitely far from anything"""
    a, b = np.float32(a), np.float32(b)
    if np.isnan(a) or np.isnan(b):
        return float("inf")

    def ordered(x):
        i = int(np.array(x, np.float32).view(np.int32))
        return i if i >= 0 else -(i & 0x7fffffff)
    return abs(ordered(a) - ordered(b))


def metric_ulps(got, exact):
    """{metric: ulp distance of got[metric] from float32(exact[metric])}"""
    return {k: ulp_distance(got[k], np.float32(exact[k])) for k in METRICS}


def metric_violations(got, exact):
    """what of a Result breaks the bound, as a list of strings (empty: within the bound)"""
    bad = ["%s: %.9g is %s ulp from %.9g" % (k, got[k], u, np.float32(exact[k])) for k, u in metric_ulps(got, exact).items() if u > ULP_BOUND]
    if float(got["valid"]) != float(exact["valid"]):
        bad.append("valid: %r, not %r" % (got["valid"], exact["valid"]))
    return bad


def composite_fp32(primary, info, infer_output_xH_y, prev, blend_factor, show_nrc):
    """the framebuffer after one frame's compositing: primary [H][W][4] (rgb = radiance up to the NRC vertex, w = throughput), info [H][W]
    (1 = the pixel scattered), infer_output_xH_y [W * H][3] (the cache's radiance, entry x * H + y), prev [H][W][4]

        c   = p.rgb (+ fmax(0, y) * p.w   where show_nrc == 1 and info == 1)
        out = bf * {c, 1} + (1 - bf) * prev

    each product, sum and difference rounded to fp32 on its own (no fused multiply-add); fmax drops a NaN radiance"""
    f32 = np.float32
    prev = np.ascontiguousarray(prev, f32)
    H, W = prev.shape[:2]
    p = np.ascontiguousarray(primary, f32).reshape(H, W, 4)
    live = np.ascontiguousarray(info, f32).reshape(H, W) == f32(1.0)
    y = np.ascontiguousarray(infer_output_xH_y, f32).reshape(W, H, 3).transpose(1, 0, 2)
    c = np.empty((H, W, 4), f32)
    c[..., :3] = p[..., :3]
    c[..., 3] = f32(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        if int(show_nrc) == 1:
            add = np.fmax(f32(0.0), y) * p[..., 3:4]
            c[..., :3] = np.where(live[..., None], p[..., :3] + add, p[..., :3])
        bf = f32(blend_factor)
        ib = f32(1.0) - bf
        out = bf * c + ib * prev
    assert out.dtype == f32
    return out


def same_bits(a, b):
    """bit-identical images (a NaN on both sides counts as equal)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
