"""What the view AOV (NrcHpmRenderer.ViewAov / RenderPath(aov_out=)) costs, on the bench scene (fBm cloud 256^3, scene 4) at 1920 x 1080.

  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/view_aov_rate.py --trace [--views 16]
      per view of an orbit: SetCamera, one frame (k_gen_rays of that view) and ViewAov (k_view_aov of the same view).  The trace's
      k_view_aov and k_gen_rays rows hold the same number of calls over the same views: their ratio of total times is the kernel's cost
      in units of one frame's camera kernel.  `--stats-csv <file>` (a second step, no GPU) prints that ratio from the trace's
      kernel_stats.csv.
  python tools/view_aov_rate.py [--views 64] [--frames-per-view 4] [--reps 7]
      a 64-view orbit through RenderPath with and without an AOV target, training on: every repetition renders the whole orbit and is
      timed by the wall clock around it with a device synchronisation before and after; the two are interleaved on one renderer.  One JSON line each
      (median ms per view, min, max, spread) and the verdict: the target's cost per view and whether it exceeds the spread.

docs/MEASUREMENT_LOG.md holds the record of a run."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H = 1920, 1080


def make(api, scene, cam):
    cfg = api.AppConfig()
    nrc = api.NeuralRadianceCache(cfg)
    return api.NrcHpmRenderer(W, H, False, cam, cfg, scene, nrc), nrc


def trace(args):
    import torch
    from nrc_hpm_renderer_amd import api, scene as sc
    scene = sc.make_scene(sc.cached_volume("cloud", 256, seed=1337), scene_id=4)
    views = sc.orbit_cameras(args.views, aspect=W / H)
    ren, nrc = make(api, scene, views[0])
    hit = 0
    for v in views:
        ren.SetCamera(None, v)
        ren.Render(None, False)
        hit += int((ren.ViewAov()[..., 1] > 0).sum().item())
    torch.cuda.synchronize()
    print(json.dumps(dict(what="view_aov_trace", views=args.views, size=[W, H], pixels_that_hit=hit / (args.views * W * H))))
    ren.Destroy()
    nrc.Destroy()


def stats(path):
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            for key in ("k_view_aov", "k_gen_rays"):
                if key in r["Name"]:
                    rows[key] = dict(calls=int(r["Calls"]), total_ns=float(r["TotalDurationNs"]))
    a, g = rows["k_view_aov"], rows["k_gen_rays"]
    print(json.dumps(dict(what="view_aov_kernel_ratio", k_view_aov_ms=a["total_ns"] / a["calls"] * 1e-6, k_gen_rays_ms=g["total_ns"] / g["calls"] * 1e-6,
                          calls=[a["calls"], g["calls"]], ratio=(a["total_ns"] / a["calls"]) / (g["total_ns"] / g["calls"]))))


def orbit(args):
    import torch
    from nrc_hpm_renderer_amd import api, scene as sc
    if args.reps < 5:
        raise SystemExit("at least 5 repetitions: the verdict rests on their spread")
    scene = sc.make_scene(sc.cached_volume("cloud", 256, seed=1337), scene_id=4)
    views = sc.orbit_cameras(args.views, aspect=W / H)
    aovs = torch.empty((args.views, H, W, 4), device="cuda")
    # ONE renderer for both: the frames of a process's second renderer are slower whatever it is asked to do (docs/MEASUREMENT_LOG.md,
    # "View AOV": its inference and training streams were seen on one hardware queue)
    ren, nrc = make(api, scene, views[0])
    hows = ("plain", "aov")

    def run(how, vs):
        ren.RenderPath(vs, args.frames_per_view, None, train=True, out=False, aov_out=aovs[:len(vs)] if how == "aov" else None)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for how in hows:      # warm-up: allocations, the flight selection, clocks
        run(how, views[:4])
    ms = {how: [] for how in hows}
    for _ in range(args.reps):
        for how in hows:
            ms[how].append(timed(lambda: run(how, views)) / args.views)
    res = {}
    for how, v in ms.items():
        med = statistics.median(v)
        res[how] = dict(what="view_aov_orbit", how=how, views=args.views, frames_per_view=args.frames_per_view, reps=len(v), median_ms_per_view=med,
                        min=min(v), max=max(v), spread=(max(v) - min(v)) / med)
        print(json.dumps(res[how]), flush=True)
    a, b = res["aov"]["median_ms_per_view"], res["plain"]["median_ms_per_view"]
    print(json.dumps(dict(what="view_aov_orbit_verdict", cost_ms_per_view=a - b, aov_over_plain=a / b, plain_spread=res["plain"]["spread"],
                          within_spread=bool(a <= b * (1.0 + res["plain"]["spread"])))), flush=True)
    ren.Destroy()
    nrc.Destroy()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--stats-csv", default=None)
    ap.add_argument("--views", type=int, default=None)
    ap.add_argument("--frames-per-view", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if args.stats_csv:
        return stats(args.stats_csv)
    if args.views is None:
        args.views = 16 if args.trace else 64
    return trace(args) if args.trace else orbit(args)


if __name__ == "__main__":
    main()
