"""What the deep AOV (DeepViewAov / DeepOrthoAov: k_ray_aov<Src, DeepOut>) costs beside the flat kernel of the same rays, on the bench scene
(fBm cloud 256^3, scene 4) at 1920 x 1080.

  rocprofv3 --kernel-trace -d <dir> -- python tools/deep_aov_rate.py --trace [--views 16]
      per view of an orbit, in this order: ViewAovToDepth with depth +inf (k_ray_aov<ViewDepth, FlatOut>, the flat kernel), DeepViewAov with
      the flat result at K = 1 (ln 2), K = 8 and K = 32 (scene.deep_levels(K, 3.0)) (k_ray_aov<ViewDepth, DeepOut>), and the flat kernel once
      more: the difference between a view's two flat launches is the trace's run-to-run spread.  Behind the views a 1024^2 scene.light_view
      the same way, five times (k_ray_aov<OrthoView, FlatOut | DeepOut>).  One warm-up pass runs in front of each.
  python tools/deep_aov_rate.py --trace-csv <dir>/.../..._kernel_trace.csv [--views 16]      (a second step, no GPU)
      the mean duration of each of those launches from the trace's rows, told apart by kernel name and by their order; the ratios to the
      flat kernel of the same trace; the spread; and K flat walks -- what the one deep launch replaces -- against it.

docs/MEASUREMENT_LOG.md holds the record of a run."""
import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H = 1920, 1080
LIGHT = 1024
LIGHT_REPEATS = 5
KS = (1, 8, 32)
TAU_MAX = 3.0


def level_sets():
    import numpy as np
    from nrc_hpm_renderer_amd import scene as sc
    return [np.array([float.fromhex("0x1.62e430p-1")], np.float32)] + [sc.deep_levels(k, TAU_MAX) for k in KS[1:]]


def trace(args):
    import torch
    from nrc_hpm_renderer_amd import api, scene as sc
    scene = sc.make_scene(sc.cached_volume("cloud", 256, seed=1337), scene_id=4)
    views = sc.orbit_cameras(args.views, aspect=W / H)
    cfg = api.AppConfig()
    nrc = api.NeuralRadianceCache(cfg)
    ren = api.NrcHpmRenderer(W, H, False, views[0], cfg, scene, nrc)
    sets = level_sets()
    whole = torch.full((H, W), float("inf"), device="cuda")
    flat = torch.empty((H, W, 4), device="cuda")
    deep_flat = torch.empty((H, W, 4), device="cuda")
    planes = torch.empty((max(KS), H, W), device="cuda")
    reached = [0] * len(KS)
    for i, v in enumerate([views[0]] + list(views)):      # (the first pass is the warm-up)
        ren.SetCamera(None, v)
        torch.cuda.synchronize()
        ren.ViewAovToDepth(whole, out=flat)
        for j, levels in enumerate(sets):
            ren.DeepViewAov(levels, out=planes[:levels.size], flat=deep_flat)
            if not bool((flat.view(torch.int32) == deep_flat.view(torch.int32)).all().item()):
                raise SystemExit("the deep call's flat result differs from ViewAovToDepth(+inf) on view %d, K = %d" % (i, levels.size))
            if i:
                reached[j] += int(torch.isfinite(planes[levels.size - 1]).sum().item())
        ren.ViewAovToDepth(whole, out=flat)
        torch.cuda.synchronize()
    light = sc.light_view(scene, LIGHT, LIGHT)
    s_flat = torch.empty((LIGHT, LIGHT, 4), device="cuda")
    s_planes = torch.empty((max(KS), LIGHT, LIGHT), device="cuda")
    for i in range(LIGHT_REPEATS + 1):
        ren.OrthoAov(light, LIGHT, LIGHT, out=s_flat)
        for levels in sets:
            ren.DeepOrthoAov(light, LIGHT, LIGHT, levels, out=s_planes[:levels.size], flat=True)
        ren.OrthoAov(light, LIGHT, LIGHT, out=s_flat)
        torch.cuda.synchronize()
    n = args.views * W * H
    print(json.dumps(dict(what="deep_aov_trace", views=args.views, size=[W, H], levels=[[float(x) for x in s] for s in sets],
                          pixels_that_reach_the_top_level={str(k): r / n for k, r in zip(KS, reached)}, light_view=[LIGHT, LIGHT])))
    ren.Destroy()
    nrc.Destroy()


def trace_csv(path, views):
    names = None
    # k_ray_aov<source, output>: the flat kernel and the deep one differ in the output's name
    rows = {("FlatOut", "ViewDepth"): [], ("DeepOut", "ViewDepth"): [], ("FlatOut", "OrthoView"): [], ("DeepOut", "OrthoView"): []}
    with open(path) as f:
        for r in csv.DictReader(f):
            if names is None:
                cols = {c.lower(): c for c in r}
                names = (cols["kernel_name"], cols["start_timestamp"], cols["end_timestamp"])
            name = r[names[0]]
            for key in rows:
                if "k_ray_aov" in name and key[0] in name and key[1] in name:
                    rows[key].append((float(r[names[1]]), float(r[names[2]]) - float(r[names[1]])))
    for v in rows.values():
        v.sort()

    def series(key, per_pass, passes, which):
        d = [ns * 1e-6 for _, ns in rows[key]][per_pass:]      # (without the warm-up pass's launches)
        if len(d) != per_pass * passes:
            raise SystemExit("%s: %d launches in the trace behind the warm-up, %d expected" % (key, len(d), per_pass * passes))
        return d[which::per_pass]

    def mean(x):
        return sum(x) / len(x)

    res = dict(what="deep_aov_kernels", views=views)
    for tag, src, passes in (("view", "ViewDepth", views), ("light_1024", "OrthoView", LIGHT_REPEATS)):
        first, last = series(("FlatOut", src), 2, passes, 0), series(("FlatOut", src), 2, passes, 1)
        flat = mean(first + last)
        res[tag + "_flat_ms"] = flat
        # run-to-run: a pass's two flat launches walk the same rays
        res[tag + "_flat_spread"] = mean([abs(a - b) for a, b in zip(first, last)]) / flat
        for j, k in enumerate(KS):
            d = series(("DeepOut", src), len(KS), passes, j)
            per_pass = [x / (0.5 * (a + b)) for x, a, b in zip(d, first, last)]
            res["%s_deep_k%d_ms" % (tag, k)] = mean(d)
            res["%s_deep_k%d_over_flat" % (tag, k)] = mean(d) / flat
            res["%s_deep_k%d_over_flat_range" % (tag, k)] = [min(per_pass), max(per_pass)]
            res["%s_k%d_flat_walks_over_deep" % (tag, k)] = k * flat / mean(d)
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
