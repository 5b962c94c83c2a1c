"""What the ray AOV (RayAov / ViewAovToDepth / OrthoAov: k_ray_aov) costs, on the bench scene (fBm cloud 256^3, scene 4) at 1920 x 1080.

  rocprofv3 --kernel-trace -d <dir> -- python tools/ray_aov_rate.py --trace [--views 16]
      per view of an orbit, in this order: ViewAov (k_view_aov), ViewAovToDepth with depth +inf (k_ray_aov<ViewDepth>: the same walk),
      ViewAovToDepth to a sphere of radius 0.2 |size| at the origin (the holdout), RayAov on the view's camera rays in pixel-row order
      and again in 8x8-tile order (k_ray_aov<RayList>: what an incoherent list costs); behind the views one 1024^2 scene.light_view
      (k_ray_aov<OrthoView>).  One warm-up view runs in front.
  python tools/ray_aov_rate.py --trace-csv <dir>/.../..._kernel_trace.csv [--views 16]      (a second step, no GPU)
      the mean duration of each of those launches from the trace's rows, told apart by kernel name and by their order, and the ratios
      to k_view_aov of the same views.

docs/MEASUREMENT_LOG.md holds the record of a run."""
import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H = 1920, 1080
LIGHT = 1024


def tile_order(w, h):
    """pixel indices of a w x h image, 8x8 tile by tile (row-major tiles, row-major inside a tile)"""
    import numpy as np
    y, x = np.mgrid[0:h, 0:w]
    key = ((y >> 3) * ((w + 7) >> 3) + (x >> 3)) * 64 + (y & 7) * 8 + (x & 7)
    return np.argsort(key.reshape(-1), kind="stable")


def trace(args):
    import numpy as np
    import torch
    from nrc_hpm_renderer_amd import api, cli, scene as sc
    scene = sc.make_scene(sc.cached_volume("cloud", 256, seed=1337), scene_id=4)
    views = sc.orbit_cameras(args.views, aspect=W / H)
    cfg = api.AppConfig()
    nrc = api.NeuralRadianceCache(cfg)
    ren = api.NrcHpmRenderer(W, H, False, views[0], cfg, scene, nrc)
    radius = 0.2 * float(np.linalg.norm(np.asarray(scene["size"], np.float64)))
    order = torch.from_numpy(tile_order(W, H)).cuda()
    whole = torch.full((H, W), float("inf"), device="cuda")
    out = torch.empty((H, W, 4), device="cuda")
    out_list = torch.empty((H * W, 4), device="cuda")
    hit = held = 0
    for i, v in enumerate([views[0]] + list(views)):      # (the first pass is the warm-up)
        rays = api.camera_rays(v, W, H)
        d_rays = torch.from_numpy(rays.reshape(-1, 8)).cuda()
        d_tiled = d_rays[order].contiguous()
        d_depth = torch.from_numpy(cli.sphere_depth(rays, radius)).cuda()
        torch.cuda.synchronize()
        ren.SetCamera(None, v)
        a = ren.ViewAov()
        ren.ViewAovToDepth(whole, out=out)
        same = bool((a.view(torch.int32) == out.view(torch.int32)).all().item())
        ren.ViewAovToDepth(d_depth, out=out)
        ren.RayAov(d_rays, out=out_list)
        ren.RayAov(d_tiled, out=out_list)
        torch.cuda.synchronize()
        if not same:
            raise SystemExit("ViewAovToDepth(+inf) differs from ViewAov on view %d" % i)
        if i:
            hit += int((a[..., 1] > 0).sum().item())
            held += int(torch.isfinite(d_depth).sum().item())
    shadow = ren.OrthoAov(sc.light_view(scene, LIGHT, LIGHT), LIGHT, LIGHT)
    torch.cuda.synchronize()
    n = args.views * W * H
    print(json.dumps(dict(what="ray_aov_trace", views=args.views, size=[W, H], pixels_that_hit=hit / n, pixels_behind_the_sphere=held / n,
                          light_view=[LIGHT, LIGHT], light_rays_that_hit=float((shadow[..., 1] > 0).float().mean().item()))))
    ren.Destroy()
    nrc.Destroy()


def trace_csv(path, views):
    names = None
    rows = {"k_view_aov": [], "ViewDepth": [], "RayList": [], "OrthoView": []}
    with open(path) as f:
        for r in csv.DictReader(f):
            if names is None:
                cols = {c.lower(): c for c in r}
                names = (cols["kernel_name"], cols["start_timestamp"], cols["end_timestamp"])
            name = r[names[0]]
            ns = float(r[names[2]]) - float(r[names[1]])
            start = float(r[names[1]])
            if "k_view_aov" in name:
                rows["k_view_aov"].append((start, ns))
            elif "k_ray_aov" in name:
                for key in ("ViewDepth", "RayList", "OrthoView"):
                    if key in name:
                        rows[key].append((start, ns))
    for v in rows.values():
        v.sort()

    def mean(key, per_view, which):
        d = [ns for _, ns in rows[key]][per_view:]      # (without the warm-up view's launches)
        if len(d) != per_view * views:
            raise SystemExit("%s: %d launches in the trace behind the warm-up, %d expected" % (key, len(d), per_view * views))
        d = d[which::per_view]
        return sum(d) / len(d) * 1e-6

    res = dict(what="ray_aov_kernels", views=views, k_view_aov_ms=mean("k_view_aov", 1, 0), view_depth_inf_ms=mean("ViewDepth", 2, 0),
               view_depth_sphere_ms=mean("ViewDepth", 2, 1), ray_list_rows_ms=mean("RayList", 2, 0), ray_list_tiles_ms=mean("RayList", 2, 1),
               ortho_1024_ms=rows["OrthoView"][-1][1] * 1e-6)
    base = res["k_view_aov_ms"]
    for k in ("view_depth_inf_ms", "view_depth_sphere_ms", "ray_list_rows_ms", "ray_list_tiles_ms"):
        res[k.replace("_ms", "_over_view_aov")] = res[k] / base
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-csv", default=None)
    ap.add_argument("--views", type=int, default=16)
    args = ap.parse_args()
    if args.trace_csv:
        return trace_csv(args.trace_csv, args.views)
    if not args.trace:
        raise SystemExit("give --trace (under rocprofv3 --kernel-trace) or --trace-csv <kernel_trace.csv>")
    return trace(args)


if __name__ == "__main__":
    main()
